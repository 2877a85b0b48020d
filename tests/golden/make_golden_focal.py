"""Golden fixture of the focal loss kernels (cbim_focal_fwd / cbim_focal_bwd).   python tests/golden/make_golden_focal.py

The REAL reference modules (/root/reference/training/losses.py: FocalLoss :60-98, DiceLoss :8-58) run on the CPU on float64
logits under fixed seeds; nothing of the reference is copied, only what it computes is stored.  Logits are float32 values
(randn * scale), evaluated in float64; labels follow tests/op_checks.check_loss (unbalanced: the first two slices are class 0).
  focal.npz   per case: logits float32 [N, C, ...], labels int16 [N, ...], alpha float32 [C] (empty: none), gamma float64,
              mean bool (size_average), focal float64 + focal_grad float64 [N, C, ...] (FocalLoss and its gradient),
              dice float64 + dice_grad float64 (DiceLoss() on the same logits and labels[:, None])
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
# name -> (N, C, spatial, gamma, alpha table?, mean?, logit scale, seed)      the smallest shapes that reach each kernel path
CASES = {
    "v4": (2, 6, (6, 7, 8), 2.0, False, True, 2.0, 5),               # four voxels per thread, one workgroup
    "multi": (2, 6, (8, 12, 12), 2.0, True, True, 2.0, 6),           # 2304 voxels: several workgroups, cross-workgroup reduce
    "c20": (2, 20, (3, 5, 6), 3.0, True, True, 2.0, 7),              # class bound 32, two voxels per thread
    "c20_odd": (2, 20, (3, 5, 7), 2.0, False, True, 2.0, 8),         # odd plane: one voxel per thread
    "plane": (2, 10, (12, 12), 2.0, False, True, 2.0, 9),            # 2-D, as the reference's own __main__
    "half_sum": (2, 6, (6, 7, 8), 0.5, True, False, 2.0, 10),        # non-integer gamma, summed
    "gamma0": (2, 4, (4, 8, 8), 0.0, False, True, 2.0, 11),          # must equal the unweighted mean CE
    "sat_g2": (2, 4, (4, 8, 8), 2.0, False, True, 30.0, 12),         # saturated softmax
    "sat_g15": (2, 4, (4, 8, 8), 1.5, False, True, 30.0, 12),
}


def reference_losses():
    spec = importlib.util.spec_from_file_location("reference_losses", os.path.join(REF, "training", "losses.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build():
    ref = reference_losses()
    out = {}
    for name, (N, C, sp, gamma, has_alpha, mean, scale, seed) in CASES.items():
        torch.manual_seed(seed)
        z32 = torch.randn(N, C, *sp) * scale
        lab = torch.randint(0, C, (N,) + sp)
        lab[:, :2] = 0
        alpha = torch.rand(C) + 0.5 if has_alpha else None
        z = z32.double().requires_grad_(True)
        fl = ref.FocalLoss(C, alpha=None if alpha is None else alpha.double(), gamma=gamma, size_average=mean)(z, lab)
        (gf,) = torch.autograd.grad(fl, z)
        zd = z32.double().requires_grad_(True)
        dl = ref.DiceLoss()(zd, lab.unsqueeze(1))
        (gd,) = torch.autograd.grad(dl, zd)
        assert bool(torch.isfinite(gf).all()) and bool(torch.isfinite(gd).all()) and fl.dtype == torch.float64 and dl.dtype == torch.float64
        out[f"{name}_logits"], out[f"{name}_labels"] = z32.numpy(), lab.numpy().astype(np.int16)
        out[f"{name}_alpha"] = np.zeros(0, np.float32) if alpha is None else alpha.numpy()
        out[f"{name}_gamma"], out[f"{name}_mean"] = np.float64(gamma), np.bool_(mean)
        out[f"{name}_focal"], out[f"{name}_focal_grad"] = np.float64(fl.item()), gf.numpy()
        out[f"{name}_dice"], out[f"{name}_dice_grad"] = np.float64(dl.item()), gd.numpy()
        print(f"  {name}: {N}x{C}x{sp} gamma {gamma} alpha {has_alpha} {'mean' if mean else 'sum'}: focal {fl.item():.9g} dice {dl.item():.9g}")
    return out


def main():
    out = build()
    path = os.path.join(HERE, "focal.npz")
    np.savez_compressed(path, **out)
    print(f"  focal.npz {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 900 * 1024


if __name__ == "__main__":
    main()
