"""Golden fixture of the top-k cross-entropy kernels (cbim_topk_fwd / cbim_topk_bwd).   python tests/golden/make_golden_topk.py

The top-k term is evaluated here in float64 with torch from its definition:
    nll_i = w[y_i] (logsumexp(z_i) - z_i[y_i])  over all voxels of the batch,  K = int(N S k / 100),
    topk = (sum of the K largest nll) / K
and its gradient by autograd through torch.topk.  The Dice term and its gradient come from the live reference's DiceLoss (loaded the
way make_golden_focal.py loads it); nothing of the reference is copied, only what it computes is stored.  Logits are float32 values
(randn * 2) evaluated in float64; labels are unbalanced (the first two slices along the first spatial axis are class 0).

A float32 nll can fall on the other side of the threshold tau (the K-th largest value) when its float64 value lies within
1e-5 * max(1, tau) of it; the tests leave such voxels out of the gradient comparison, at most 0.2 % of a case's voxels.  This script
asserts that bound in float64 and draws the next seed if a case misses it.

  topk.npz   per input: <input>_logits float32 [N, C, ...], <input>_labels int16 [N, ...], <input>_dice float64,
             <input>_dice_grad float64;  per case: <case>_input (name), <case>_k float64, <case>_K int64, <case>_weight float32 [C]
             (empty: none), <case>_topk float64, <case>_tau float64, <case>_near int64 (voxels in the band, the threshold included),
             <case>_topk_grad float64 [N, C, ...]
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_focal import reference_losses  # noqa: E402

# input -> (N, C, spatial, first seed)                                 the smallest shapes that reach each kernel path
INPUTS = {
    "line": (1, 2, (5,), 41),                  # one spatial axis, odd: one voxel per thread
    "v4": (2, 3, (4, 6, 8), 42),               # four voxels per thread, batch > 1
    "c17": (1, 17, (6, 6, 6), 43),             # class bound 32, two voxels per thread
    "multi": (1, 3, (17, 19, 23), 44),         # 7429 voxels: several workgroup records, odd (one voxel per thread, a tail in the select)
}
# case -> (input, k percent, weighted?)
CASES = {
    "line_k100": ("line", 100.0, False),
    "line_k50": ("line", 50.0, False),
    "line_one": ("line", 20.0, False),         # K = 1
    "v4_k100": ("v4", 100.0, False),
    "v4_k50": ("v4", 50.0, False),
    "v4_k10_w": ("v4", 10.0, True),
    "c17_k10": ("c17", 10.0, False),
    "multi_k10": ("multi", 10.0, False),
    "multi_k50_w": ("multi", 50.0, True),
}
BAND, CAP = 1e-5, 0.002


def nll_f64(z, lab, weight):
    """per-voxel weighted cross entropy [N*S] of float64 logits [N, C, ...]"""
    N, C = int(z.shape[0]), int(z.shape[1])
    zf, y = z.reshape(N, C, -1), lab.reshape(N, -1)
    lse = torch.logsumexp(zf, 1)
    zy = torch.gather(zf, 1, y[:, None, :]).squeeze(1)
    w = torch.ones_like(lse) if weight is None else weight.double()[y]
    return (w * (lse - zy)).reshape(-1)


def band(nll, tau):
    """voxels a float32 evaluation may put on the other side of tau; a threshold with no neighbour in the band is unambiguous"""
    near = (nll - tau).abs() <= BAND * max(1.0, tau)
    return near if int(near.sum()) > 1 else torch.zeros_like(near)


def draw(N, C, sp, seed):
    torch.manual_seed(seed)
    z32 = torch.randn(N, C, *sp) * 2.0
    lab = torch.randint(0, C, (N,) + sp)
    lab[:, :2] = 0
    return z32, lab


def case_weight(C):
    g = torch.Generator().manual_seed(7 + C)
    return torch.rand(C, generator=g) + 0.5


def evaluate(z32, lab, k, weight):
    z = z32.double().requires_grad_(True)
    nll = nll_f64(z, lab, weight)
    K = int(nll.numel() * k / 100)
    top = torch.topk(nll, K).values
    loss = top.sum() / K
    (g,) = torch.autograd.grad(loss, z)
    tau = float(top.min().detach())
    near = band(nll.detach(), tau)
    return K, float(loss.detach()), tau, int(near.sum()), g


def build():
    ref = reference_losses()
    out = {}
    for iname, (N, C, sp, seed) in INPUTS.items():
        mine = {c: v for c, v in CASES.items() if v[0] == iname}
        while True:
            z32, lab = draw(N, C, sp, seed)
            res = {c: evaluate(z32, lab, k, case_weight(C) if wt else None) for c, (_, k, wt) in mine.items()}
            if all(r[3] <= CAP * lab.numel() for r in res.values()):
                break
            print(f"  {iname}: seed {seed} leaves {[r[3] for r in res.values()]} voxels in the band: next seed")
            seed += 100
        zd = z32.double().requires_grad_(True)
        dl = ref.DiceLoss()(zd, lab.unsqueeze(1))
        (gd,) = torch.autograd.grad(dl, zd)
        assert bool(torch.isfinite(gd).all()) and dl.dtype == torch.float64
        out[f"{iname}_logits"], out[f"{iname}_labels"] = z32.numpy(), lab.numpy().astype(np.int16)
        out[f"{iname}_dice"], out[f"{iname}_dice_grad"] = np.float64(dl.item()), gd.numpy()
        for c, (K, loss, tau, near, g) in res.items():
            _, k, wt = mine[c]
            out[f"{c}_input"], out[f"{c}_k"], out[f"{c}_K"] = np.str_(iname), np.float64(k), np.int64(K)
            out[f"{c}_weight"] = case_weight(C).numpy() if wt else np.zeros(0, np.float32)
            out[f"{c}_topk"], out[f"{c}_tau"], out[f"{c}_near"] = np.float64(loss), np.float64(tau), np.int64(near)
            out[f"{c}_topk_grad"] = g.numpy()
            print(f"  {c}: {N}x{C}x{sp} seed {seed} k {k} K {K} weighted {wt}: topk {loss:.9g} tau {tau:.9g} in band {near} dice {dl.item():.9g}")
    return out


def main():
    out = build()
    path = os.path.join(HERE, "topk.npz")
    np.savez_compressed(path, **out)
    print(f"  topk.npz {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 700 * 1024


if __name__ == "__main__":
    main()
