"""Checks of the top-k cross-entropy kernels (csrc/topk_kernels.hip) and their surfaces: ops.topk_fwd / topk_bwd,
functional.TopKCEFn, training.losses.TopKLoss / DiceTopKLoss.

Shared by tests/test_topk_emu.py (CPU: the kernels on the host-side executor of tests/emu) and tests/test_gpu_topk.py (-m gpu).
Expectations: tests/golden/topk.npz holds the float64 top-k term (torch.topk of the per-voxel cross entropy) and the reference's
DiceLoss on each case (tests/golden/make_golden_topk.py); on shapes outside the fixture the float64 formulation below, with the
tie rule written out:  tau = K-th largest nll, n_gt = #{nll > tau}, n_eq = #{nll == tau},
    topk = (sum_{nll > tau} nll + (K - n_gt) tau) / K,   a voxel's share: 1/K above tau, (K - n_gt) / (n_eq K) at tau, 0 below.
Tolerances are those of the focal family on the same arithmetic (tests/focal_checks.py): a loss within 2e-6 relative, a gradient
with relerr < 2e-5, against float64 values.  A float32 nll may fall on the other side of tau where its float64 value lies within
1e-5 * max(1, tau) of it: such voxels (never more than 0.2 % of a case, none if the threshold has no neighbour there) are left out
of the gradient comparison.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cbim_amd import _lib, ops
from cbim_amd import functional as Fn
from cbim_amd.training.losses import DiceCELoss, DiceLoss, DiceTopKLoss, TopKLoss, check_labels
from tests.op_checks import relerr

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_RTOL, GRAD_TOL = 2e-6, 2e-5
BAND, CAP = 1e-5, 0.002
CASES = ("line_k100", "line_k50", "line_one", "v4_k100", "v4_k50", "v4_k10_w", "c17_k10", "multi_k10", "multi_k50_w")
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = np.load(os.path.join(HERE, "golden", "topk.npz"))
    return _golden


def case(name):
    g = golden()
    i = str(g[f"{name}_input"])
    w = torch.from_numpy(g[f"{name}_weight"])
    return {"z": torch.from_numpy(g[f"{i}_logits"]), "lab": torch.from_numpy(g[f"{i}_labels"].astype(np.int64)),
            "weight": w if w.numel() else None, "k": float(g[f"{name}_k"]), "K": int(g[f"{name}_K"]),
            "topk": float(g[f"{name}_topk"]), "tau": float(g[f"{name}_tau"]),
            "topk_grad": torch.from_numpy(g[f"{name}_topk_grad"]),
            "dice": float(g[f"{i}_dice"]), "dice_grad": torch.from_numpy(g[f"{i}_dice_grad"])}


def close(got, want, rtol=LOSS_RTOL):
    print(f"    loss {got!r} against {want!r}: relative {abs(got - want) / max(abs(want), 1e-300):.2e}")
    return abs(got - want) <= rtol * abs(want)


def grad_close(got, want, keep=None, tol=GRAD_TOL):
    """keep: bool [N*S], False where a voxel is left out of the comparison"""
    if keep is not None:
        N, C = int(want.shape[0]), int(want.shape[1])
        m = keep.reshape(N, 1, -1).double()
        got, want = got.reshape(N, C, -1).double() * m, want.reshape(N, C, -1).double() * m
    e = relerr(got, want)
    print(f"    gradient relerr {e:.2e}" + ("" if keep is None else f" ({int((~keep).sum())} voxels left out)"))
    return e < tol


def to(dev, t):
    return None if t is None else t.to(dev)


def f64_nll(z, lab, weight):
    """per-voxel weighted cross entropy [N*S] of float64 logits; a label outside [0, C) gives 0"""
    N, C = int(z.shape[0]), int(z.shape[1])
    zf, y = z.reshape(N, C, -1), lab.reshape(N, -1)
    ok = (y >= 0) & (y < C)
    yc = y.clamp(0, C - 1)
    lse = torch.logsumexp(zf, 1)
    zy = torch.gather(zf, 1, yc[:, None, :]).squeeze(1)
    w = ok.double() if weight is None else weight.double()[yc] * ok.double()
    return (w * (lse - zy)).reshape(-1)


def f64_losses(z32, lab, weight, K, w_tk=0.0, w_dice=0.0):
    """float64 (top-k term, Dice, tau, keep mask) with the tie rule of the module docstring, and the gradient of
    w_tk * topk + w_dice * Dice."""
    z = z32.double().requires_grad_(True)
    N, C = int(z.shape[0]), int(z.shape[1])
    nll = f64_nll(z, lab, weight)
    v = nll.detach()
    tau = float(torch.sort(v, descending=True).values[K - 1])
    gt, eq = v > tau, v == tau
    n_gt, n_eq = int(gt.sum()), int(eq.sum())
    share = gt.double() / K + eq.double() * ((K - n_gt) / (n_eq * K))
    tk = (share * nll).sum()
    zf, y = z.reshape(N, C, -1), lab.reshape(N, -1)
    onehot = (torch.arange(C)[None, :, None] == y[:, None, :]).double()
    P = torch.softmax(zf, 1)
    eps = float(np.float32(1e-5))
    TP, SP, CNT = (P * onehot).sum((0, 2)), P.sum((0, 2)), onehot.sum((0, 2))
    FP, FN = SP - TP, CNT - TP
    al = torch.clamp(FP / (FP + FN + eps), 0.2, 0.8)
    dice = (1.0 - TP / (TP + al * FP + (1.0 - al) * FN + eps)).mean()
    (w_tk * tk + w_dice * dice + 0.0 * z.sum()).backward()
    near = ((v - tau).abs() <= BAND * max(1.0, tau)) & ~eq
    keep = ~(near | eq) if bool(near.any()) else torch.ones_like(near)
    return float(tk.detach()), float(dice.detach()), tau, keep, z.grad


def capped(keep):
    left = int((~keep).sum())
    print(f"    {left} of {keep.numel()} voxels next to the threshold")
    return left <= CAP * keep.numel()


def run_fn(dev, z32, lab, weight, k, with_dice, w_tk=0.0, w_dice=0.0):
    z = z32.to(dev).clone().requires_grad_(True)
    out = Fn.TopKCEFn.apply(z, lab.to(dev), to(dev, weight), k, with_dice)
    loss = w_tk * out[1] + w_dice * out[2]
    loss.backward()
    return out.detach().cpu(), float(loss.detach()), z.grad.cpu()


# ---- 1. the fixture cases ------------------------------------------------------------------------------------------------------------

def check_fixture_case(dev, name):
    c = case(name)
    crit = TopKLoss(weight=c["weight"], k=c["k"]).to(dev)
    z = c["z"].to(dev).clone().requires_grad_(True)
    loss = crit(z, c["lab"].to(dev))
    loss.backward()
    loss = loss.detach()
    # the float64 formulation of this file gives what torch.topk gave (it stands in for it on the shapes outside the fixture)
    tk, dl, tau, keep, g = f64_losses(c["z"], c["lab"], c["weight"], c["K"], w_tk=1.0)
    assert Fn.topk_count(c["lab"].numel(), c["k"]) == c["K"] and abs(tau - c["tau"]) <= 1e-12 * abs(c["tau"]) and capped(keep)
    assert abs(tk - c["topk"]) <= 1e-12 * abs(c["topk"]) and abs(dl - c["dice"]) <= 2e-7
    assert relerr(g, c["topk_grad"]) < 1e-11
    assert loss.dim() == 0 and close(float(loss), c["topk"])
    assert grad_close(z.grad.cpu(), c["topk_grad"], keep)


def check_dice_topk(dev, name):
    c = case(name)
    lab1 = c["lab"].unsqueeze(1)
    _, _, _, keep, _ = f64_losses(c["z"], c["lab"], c["weight"], c["K"])
    out, loss, g = run_fn(dev, c["z"], lab1, c["weight"], c["k"], True, w_tk=0.7, w_dice=1.3)
    assert close(float(out[1]), c["topk"]) and close(float(out[2]), c["dice"])
    assert close(loss, 0.7 * c["topk"] + 1.3 * c["dice"])
    assert close(float(out[0]), c["topk"] + c["dice"]) and float(out[4]) == float(out[1] + out[2])
    assert grad_close(g, 0.7 * c["topk_grad"] + 1.3 * c["dice_grad"], keep)
    crit = DiceTopKLoss(weight=c["weight"], k=c["k"]).to(dev)
    z = c["z"].to(dev).clone().requires_grad_(True)
    v = crit(z, lab1.to(dev))
    v.backward()
    assert close(float(v.detach()), c["topk"] + c["dice"]) and grad_close(z.grad.cpu(), c["topk_grad"] + c["dice_grad"], keep)


# ---- 2. k = 100 is the mean cross entropy ----------------------------------------------------------------------------------------------

def check_k100_is_mean_ce(dev):
    for name in ("v4_k100", "c17_k10", "multi_k10", "line_k100"):
        c = case(name)
        z, lab1 = c["z"].to(dev), c["lab"].unsqueeze(1).to(dev)
        za = z.clone().requires_grad_(True)
        a = TopKLoss(k=100).to(dev)(za, lab1)
        a.backward()
        zb = z.clone().requires_grad_(True)
        b = Fn.DiceCEFn.apply(zb, lab1, None)[0]            # the CE term of DiceCELoss(weight=None)
        b.backward()
        assert close(float(a.detach()), float(b.detach().double()), 1e-6)
        assert grad_close(za.grad.cpu(), zb.grad.cpu(), tol=1e-6)
        ce = F.cross_entropy(c["z"].double(), c["lab"])
        assert close(float(a.detach()), float(ce))


# ---- 3. / 4. the Dice term -------------------------------------------------------------------------------------------------------------

def check_dice_bits(dev):
    for name in ("v4_k50", "c17_k10", "multi_k10", "line_k50"):
        c = case(name)
        C = int(c["z"].shape[1])
        z, lab = c["z"].to(dev), c["lab"].to(dev)
        out, coef, _ = ops.topk_fwd(z, lab, to(dev, c["weight"]), c["K"], True)
        out0, coef0 = ops.dice_ce_fwd(z, lab, None)
        assert torch.equal(out[2], out0[1])
        assert torch.equal(coef[:2 * C], coef0[:2 * C])
        assert torch.equal(coef[2 * C + 1:], coef0[2 * C + 1:])          # the per-class terms 1 - dice_c
        assert float(coef[2 * C]) == float(np.float32(1.0 / c["K"]))


def check_two_modules_agree(dev):
    """DiceTopKLoss against the engine's own TopKLoss + DiceLoss as two modules."""
    for name in ("multi_k50_w", "v4_k10_w"):
        c = case(name)
        z, lab1 = c["z"].to(dev), c["lab"].unsqueeze(1).to(dev)
        one = DiceTopKLoss(weight=c["weight"], k=c["k"]).to(dev)(z, lab1)
        tk = TopKLoss(weight=c["weight"], k=c["k"]).to(dev)(z, lab1.squeeze(1))
        dl = DiceLoss()(z, lab1)
        assert torch.equal(one, tk + dl)
        za, zb = z.clone().requires_grad_(True), z.clone().requires_grad_(True)
        DiceTopKLoss(weight=c["weight"], k=c["k"]).to(dev)(za, lab1).backward()
        (TopKLoss(weight=c["weight"], k=c["k"]).to(dev)(zb, lab1) + DiceLoss()(zb, lab1)).backward()
        assert grad_close(za.grad.cpu(), zb.grad.cpu(), tol=1e-6)      # the same float32 terms, added in another order


# ---- 5. ties ---------------------------------------------------------------------------------------------------------------------------

def check_ties(dev):
    # all-zero logits: nll = ln C at every voxel, every voxel ties at the threshold
    N, C, sp = 2, 5, (3, 4, 6)
    z32 = torch.zeros(N, C, *sp)
    torch.manual_seed(51)
    lab = torch.randint(0, C, (N,) + sp)
    n = lab.numel()
    for k in (50.0, 10.0, 100.0):
        out, loss, g = run_fn(dev, z32, lab, None, k, False, w_tk=1.0)
        assert close(float(out[1]), math.log(C))
        zr = z32.double().requires_grad_(True)
        F.cross_entropy(zr, lab, reduction="sum").backward()
        assert grad_close(g, zr.grad / n)
    # mixed: a block of exactly equal values straddles rank K.  Logits (a, 0) with label 1 give nll = log(1 + e^a): three levels
    z32 = torch.zeros(1, 2, 40)
    z32[0, 0, :6] = 3.0                 # 6 voxels well above
    z32[0, 0, 6:20] = 1.0               # 14 equal voxels: the tie block
    z32[0, 0, 20:] = -2.0               # 20 voxels below
    z32 = z32[:, :, torch.randperm(40)].contiguous()
    lab = torch.ones(1, 40, dtype=torch.int64)
    K = 10                              # 6 above + 4 of the 14 tied
    out, coef, ws = ops.topk_fwd(z32.to(dev), lab.to(dev), None, K, False)
    a = z32[0, 0].double().numpy()
    nll = np.log1p(np.exp(a))
    hi, mid = nll[a == 3.0][0], nll[a == 1.0][0]
    assert close(float(out[1]), (6 * hi + 4 * mid) / K)
    share = np.where(a == 3.0, 1.0 / K, np.where(a == 1.0, 4.0 / (14 * K), 0.0))
    p0 = 1.0 / (1.0 + np.exp(-a))       # softmax of class 0; d nll / dz = (p0, -p0) for label 1
    want = torch.from_numpy(np.stack([share * p0, -share * p0])[None])
    dz = ops.topk_bwd(z32.to(dev), lab.to(dev), None, None, torch.tensor([1.0, 0.0]).to(dev), ws, False)
    assert grad_close(dz.cpu(), want) and bool((dz.cpu()[0][:, torch.from_numpy(a == -2.0)] == 0).all())
    tk, _, _, _, g = f64_losses(z32, lab, None, K, w_tk=1.0)
    assert close(float(out[1]), tk) and grad_close(dz.cpu(), g)


# ---- 6. saturation ---------------------------------------------------------------------------------------------------------------------

def check_saturation(dev):
    z32 = torch.full((1, 4, 64), -1e4)
    lab = torch.zeros(1, 64, dtype=torch.int64)
    z32[0, 0, :48] = 1e4                 # 48 confident and right: nll exactly 0
    z32[0, 1, 48:] = 1e4                 # 16 confident and wrong: nll = 2e4
    for with_dice in (False, True):
        zt = z32.to(dev).clone().requires_grad_(True)
        out = Fn.TopKCEFn.apply(zt, lab.to(dev), None, 50.0, with_dice)    # K = 32: 16 at 2e4, 16 of the 48 zeros
        (out[1] + out[2]).backward()
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(zt.grad).all())
        assert close(float(out[1].detach()), 16 * 2e4 / 32)
    out, coef, ws = ops.topk_fwd(z32.to(dev), lab.to(dev), None, 32, False)
    nll = ws[:64 * 4].view(torch.float32).cpu()                             # the workspace begins with the per-voxel terms
    assert bool((nll[:48] == 0).all()) and bool((nll[48:] == 2e4).all())


# ---- 7. labels outside [0, C) ------------------------------------------------------------------------------------------------------------

def _bad(lab, C):
    lab2 = lab.clone()
    lab2[0, -1, -1, -3:] = C + 5
    lab2[-1, 0, 0, 0] = -1
    return lab2


def check_bad_labels(dev):
    c = case("v4_k50")
    C, n = 3, c["lab"].numel()
    weight = case("v4_k10_w")["weight"]
    lab2 = _bad(c["lab"], C)
    bad = ((lab2 < 0) | (lab2 >= C)).reshape(2, -1)
    z = c["z"].to(dev)
    g2 = torch.tensor([0.7, 1.3], device=dev)
    for K in (n // 2, n // 10, n):
        out, coef, ws = ops.topk_fwd(z, lab2.to(dev), weight.to(dev), K, True)
        assert float(out[3]) == 4.0 and all(bool(torch.isfinite(t).all()) for t in (out, coef))
        dz = ops.topk_bwd(z, lab2.to(dev), weight.to(dev), coef, g2, ws, True)
        assert bool(torch.isfinite(dz).all())
        tk, dl, tau, keep, g = f64_losses(c["z"], lab2, weight, K, w_tk=0.7, w_dice=1.3)    # K still comes from N * S
        assert capped(keep) and close(float(out[1]), tk) and close(float(out[2]), dl) and grad_close(dz.cpu(), g, keep)
        out1, _, ws1 = ops.topk_fwd(z, lab2.to(dev), weight.to(dev), K, False)
        assert float(out1[3]) == 4.0 and torch.equal(out1[1], out[1]) and torch.equal(out[4], out[1] + out[2])
        dz1 = ops.topk_bwd(z, lab2.to(dev), weight.to(dev), None, g2, ws1, False).cpu().reshape(2, C, -1)
        assert bool((dz1.permute(0, 2, 1)[bad] == 0).all())                  # no gradient of the top-k term at those voxels
    assert float(ops.topk_fwd(z, c["lab"].to(dev), None, n // 2, False)[0][3]) == 0.0


def check_bad_labels_through_modules(dev):
    """The first calls raise on the spot; later ones are counted on the device and check_labels() reports them, for the new modules
    as for DiceCELoss."""
    c = case("v4_k50")
    z, lab2 = c["z"].to(dev), _bad(c["lab"], 3).to(dev)
    tk, dtk, dce = TopKLoss().to(dev), DiceTopKLoss().to(dev), DiceCELoss().to(dev)
    mode = Fn._CHECK_LABELS
    Fn._CHECK_LABELS = "first"
    try:
        try:
            check_labels()                    # re-arm the on-the-spot checks, whatever ran before
        except IndexError:
            pass
        with pytest.raises(IndexError, match="4 label"):
            tk(z, lab2)
        with pytest.raises(IndexError, match="4 label"):
            dtk(z, lab2.unsqueeze(1))
        assert check_labels() == 0
        for _ in range(4):                    # use up the on-the-spot checks on clean labels
            tk(z, c["lab"].to(dev))
        assert bool(torch.isfinite(tk(z, lab2)))
        assert bool(torch.isfinite(dtk(z, lab2.unsqueeze(1))))
        assert bool(torch.isfinite(dce(z, lab2.unsqueeze(1))))
        with pytest.raises(IndexError, match="12 label"):
            check_labels()
        assert check_labels() == 0
    finally:
        Fn._CHECK_LABELS = mode
        try:
            check_labels()
        except IndexError:
            pass


# ---- 8. misaligned base pointer ----------------------------------------------------------------------------------------------------------

def check_misaligned(dev):
    for name in ("v4_k50", "c17_k10"):
        c = case(name)
        z = c["z"].to(dev)
        buf = torch.empty(z.numel() + 1, dtype=torch.float32, device=dev)
        zm = buf[1:].view(z.shape)
        zm.copy_(z)
        assert zm.data_ptr() % 8 == 4 and zm.is_contiguous()
        lab = c["lab"].to(dev)
        g2 = torch.tensor([0.7, 1.3], device=dev)
        _, _, _, keep, _ = f64_losses(c["z"], c["lab"], None, c["K"])
        for with_dice in (False, True):
            out_a, coef_a, ws_a = ops.topk_fwd(z, lab, None, c["K"], with_dice)
            out_m, coef_m, ws_m = ops.topk_fwd(zm, lab, None, c["K"], with_dice)
            assert torch.equal(out_m[1], out_a[1]) and close(float(out_m[1]), c["topk"])      # the per-voxel terms are the same bits
            if with_dice:
                assert close(float(out_m[2]), float(out_a[2].double())) and close(float(out_m[2]), c["dice"])
            dz_a = ops.topk_bwd(z, lab, None, coef_a, g2, ws_a, with_dice)
            dz_m = ops.topk_bwd(zm, lab, None, coef_m, g2, ws_m, with_dice)
            assert grad_close(dz_m.cpu(), dz_a.cpu(), tol=1e-6)
            assert grad_close(dz_m.cpu(), 0.7 * c["topk_grad"] + (1.3 * c["dice_grad"] if with_dice else 0.0), keep)


# ---- 9. reproducibility ------------------------------------------------------------------------------------------------------------------

def check_reproducible(dev):
    c = case("multi_k50_w")
    z, lab, w = c["z"].to(dev), c["lab"].to(dev), to(dev, c["weight"])
    g2 = torch.tensor([0.7, 1.3], device=dev)
    for K, with_dice in ((c["K"], True), (c["K"], False), (1, True), (743, True)):
        runs = []
        for _ in range(2):
            out, coef, ws = ops.topk_fwd(z, lab, w, K, with_dice)
            runs.append((out, coef, ops.topk_bwd(z, lab, w, coef, g2, ws, with_dice)))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
        if with_dice:
            assert torch.equal(runs[0][1], runs[1][1])


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------------------

def check_bad_arguments(dev):
    L = _lib.lib()
    N, C, S = 2, 4, 64
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    z, lab = torch.randn(N, 33, S).to(dev), torch.zeros(N, S, dtype=torch.int64).to(dev)
    out, coef = torch.full((5,), -7.0).to(dev), torch.full((3 * 33 + 1,), -7.0).to(dev)
    dz, g2 = torch.full((N, 33, S), -7.0).to(dev), torch.ones(2).to(dev)
    nbytes = L.cbim_topk_workspace(N, C, S)
    assert nbytes >= N * S * 4 and L.cbim_topk_workspace(N, 33, S) == 0
    ws = torch.zeros(nbytes + 16, dtype=torch.uint8).to(dev)
    st = ops._stream(z)

    def fwd(zt=z, labt=lab, K=16, Cc=C, outt=out, coeft=coef, wst=ws, wb=nbytes, dice=1):
        return L.cbim_topk_fwd(p(zt), p(labt), None, K, dice, N, Cc, S, p(outt), p(coeft), p(wst), wb, st)

    def bwd(zt=z, Cc=C, coeft=coef, g2t=g2, dzt=dz, wst=ws, dice=1):
        return L.cbim_topk_bwd(p(zt), p(lab), None, p(coeft), p(g2t), p(dzt), dice, N, Cc, S, p(wst), st)

    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    assert fwd(Cc=33) == EUNSUPPORTED and bwd(Cc=33) == EUNSUPPORTED
    assert fwd(zt=None) == EINVAL and fwd(labt=None) == EINVAL and fwd(outt=None) == EINVAL and fwd(coeft=None) == EINVAL
    assert bwd(zt=None) == EINVAL and bwd(g2t=None) == EINVAL and bwd(dzt=None) == EINVAL and bwd(coeft=None) == EINVAL
    assert bwd(wst=None) == EINVAL
    assert fwd(K=-3) == EINVAL and fwd(K=N * S + 1) == EINVAL and fwd(K=0) == EINVAL
    assert b"K = 0" in L.cbim_last_error_string()
    assert fwd(wb=nbytes - 1) == EWORKSPACE and fwd(wst=None) == EWORKSPACE
    assert fwd(wst=ws[4:]) == EINVAL and bwd(wst=ws[4:]) == EINVAL                                     # not 16-byte aligned
    if dev == "cuda":
        torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((coef == -7.0).all()) and bool((dz == -7.0).all())      # nothing was launched
    assert fwd(coeft=None, dice=0) == 0 and bwd(coeft=None, dice=0) == 0                               # coef is optional without Dice
    with pytest.raises(RuntimeError, match="up to 32 classes"):
        ops.topk_fwd(z, lab, None, 16, False)
    z4 = z[:, :4].contiguous()
    o, cf, w4 = ops.topk_fwd(z4, lab, None, 16, True)
    with pytest.raises(ValueError, match="workspace"):
        ops.topk_bwd(z4, lab, None, cf, g2, w4[:-16], True)
    for bad_call in (lambda: ops.topk_fwd(z4.double(), lab, None, 16, False), lambda: ops.topk_fwd(z4, lab.int(), None, 16, False),
                     lambda: ops.topk_fwd(z4, lab, torch.ones(4, dtype=torch.float64).to(dev), 16, False),
                     lambda: ops.topk_bwd(z4, lab, None, cf, g2.double(), w4, True)):
        with pytest.raises(TypeError):
            bad_call()
    for k in (0, -1.0, 100.5, float("nan")):
        with pytest.raises(ValueError):
            TopKLoss(k=k)
        with pytest.raises(ValueError):
            DiceTopKLoss(k=k)
    with pytest.raises(ValueError, match="keeps no voxel"):           # K = int(128 * 0.5 / 100) = 0
        TopKLoss(k=0.5).to(dev)(z4, lab)
    with pytest.raises(ValueError, match="labels for"):
        TopKLoss().to(dev)(z4, lab[:, :32].contiguous())
    crit = TopKLoss(weight=[0.25, 0.5, 1.0])
    assert "weight" in dict(crit.named_buffers()) and crit.weight.dtype == torch.float32      # .to(device) moves the table


# ---- target shapes, spatial ranks ----------------------------------------------------------------------------------------------------------

def check_target_shapes_and_ranks(dev):
    torch.manual_seed(21)
    for C, sp in ((5, (37,)), (3, (9, 11)), (4, (3, 4, 5)), (3, (2, 3, 2, 4))):
        z32 = torch.randn(2, C, *sp) * 2
        lab = torch.randint(0, C, (2,) + sp)
        weight = torch.rand(C) + 0.5
        K = Fn.topk_count(lab.numel(), 25)
        tk, dl, tau, keep, g = f64_losses(z32, lab, weight, K, w_tk=1.0, w_dice=1.0)
        crit = DiceTopKLoss(weight=weight, k=25).to(dev)
        vals = []
        for t in (lab.unsqueeze(1), lab, lab.unsqueeze(1).int()):
            z = z32.to(dev).clone().requires_grad_(True)
            v = crit(z, t.to(dev))
            v.backward()
            vals.append((v.detach(), z.grad))
        assert close(float(vals[0][0]), tk + dl) and grad_close(vals[0][1].cpu(), g, keep)
        assert all(torch.equal(vals[0][0], v) and torch.equal(vals[0][1], gz) for v, gz in vals[1:])
    # under autocast (disabled inside the modules: the loss stays float32)
    z32, lab = torch.randn(2, 4, 6, 8) * 2, torch.randint(0, 4, (2, 6, 8))
    tk, dl, tau, keep, g = f64_losses(z32, lab, None, Fn.topk_count(96, 50), w_tk=1.0)
    z = z32.to(dev).clone().requires_grad_(True)
    with torch.autocast(device_type="cuda" if dev == "cuda" else "cpu", dtype=torch.bfloat16):
        v = TopKLoss(k=50).to(dev)(z, lab.to(dev))
    v.backward()
    assert v.dtype == torch.float32 and close(float(v.detach()), tk) and grad_close(z.grad.cpu(), g, keep)


# ---- 11. GPU: a benchmark-like size, graph capture ------------------------------------------------------------------------------------------

def torch_composition(z, lab1, weight, K):
    """what the kernels replace, from stock torch ops in the logits' precision: cross_entropy(reduction="none") + topk, and the
    Dice formula; z [N, C, ...] requires grad, lab1 [N, 1, ...]"""
    nll = F.cross_entropy(z, lab1.squeeze(1), weight=weight, reduction="none").reshape(-1)
    tk = torch.topk(nll, K, sorted=False).values.sum() / K
    N, C = int(z.shape[0]), int(z.shape[1])
    P = torch.softmax(z, 1).reshape(N, C, -1)
    onehot = torch.zeros_like(P).scatter_(1, lab1.reshape(N, 1, -1), 1.0)
    TP, SP, CNT = (P * onehot).sum((0, 2)), P.sum((0, 2)), onehot.sum((0, 2))
    FP, FN = SP - TP, CNT - TP
    al = torch.clamp(FP / (FP + FN + 1e-5), 0.2, 0.8)
    dice = (1.0 - TP / (TP + al * FP + (1.0 - al) * FN + 1e-5)).mean()
    return tk, dice


def check_size(dev, N=1, C=16, dhw=(32, 32, 32)):
    """Against float64 at the fixture's bars, and against the float32 torch composition on the device at twice those bars: each
    of the two float32 evaluations may sit one bar away from the float64 value."""
    torch.manual_seed(31)
    z32 = torch.randn(N, C, *dhw) * 2
    lab = torch.randint(0, C, (N,) + dhw)
    lab[:, :2] = 0
    weight = torch.rand(C) + 0.5
    K = Fn.topk_count(lab.numel(), 10)
    tk, dl, tau, keep, g = f64_losses(z32, lab, weight, K, w_tk=0.7, w_dice=1.3)
    assert capped(keep)
    out, loss, gz = run_fn(dev, z32, lab.unsqueeze(1), weight, 10, True, w_tk=0.7, w_dice=1.3)
    assert close(float(out[1]), tk) and close(float(out[2]), dl) and close(loss, 0.7 * tk + 1.3 * dl) and grad_close(gz, g, keep)
    out0 = ops.dice_ce_fwd(z32.to(dev), lab.to(dev), None)[0]
    assert torch.equal(out[2].cpu(), out0[1].cpu())
    zc = z32.to(dev).clone().requires_grad_(True)
    ctk, cdl = torch_composition(zc, lab.unsqueeze(1).to(dev), weight.to(dev), K)
    (0.7 * ctk + 1.3 * cdl).backward()
    assert close(float(out[1]), float(ctk.detach().double()), 2 * LOSS_RTOL)
    assert close(float(out[2]), float(cdl.detach().double()), 2 * LOSS_RTOL)
    assert grad_close(gz, zc.grad.cpu().double(), keep, 2 * GRAD_TOL)


def check_graph_capture(dev):
    c = case("multi_k50_w")
    crit = DiceTopKLoss(weight=c["weight"], k=c["k"]).to(dev)
    z, lab1 = c["z"].to(dev).clone().requires_grad_(True), c["lab"].unsqueeze(1).to(dev)

    def step():
        z.grad = None
        loss = crit(z, lab1)
        loss.backward()
        return loss.detach()

    eager_loss = step().clone()                       # eager warm-up call
    eager_grad = z.grad.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
        z.grad = None
        with torch.cuda.graph(g, stream=side):
            loss = step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        loss.zero_()
        z.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager_loss) and torch.equal(z.grad, eager_grad)
