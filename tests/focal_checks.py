"""Checks of the focal loss kernels (csrc/focal_kernels.hip) and their surfaces: ops.focal_fwd / focal_bwd, functional.FocalFn,
training.losses.FocalLoss / DiceFocalLoss.

Shared by tests/test_focal_emu.py (CPU: the kernels on the host-side executor of tests/emu) and tests/test_gpu_focal.py (-m gpu).
Expectations: tests/golden/focal.npz holds what the reference's FocalLoss and DiceLoss give in float64 on each case
(tests/golden/make_golden_focal.py); on shapes outside the fixture the float64 formulation below, written from the formula
    L = -a q^g log p,   p = softmax(z)[y],  q = sum_{c != y} softmax(z)[c],  a = alpha[y]
and the Dice definition in the header of csrc/loss_kernels.hip.  Tolerances are the ones check_loss (tests/op_checks.py) holds the
CE + Dice kernels to on both back ends: a loss within 2e-6 relative, a gradient with relerr < 2e-5, against float64 values.
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cbim_amd import _lib, ops
from cbim_amd import functional as Fn
from cbim_amd.training.losses import DiceCELoss, DiceFocalLoss, DiceLoss, FocalLoss, check_labels
from tests.op_checks import relerr

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_RTOL, GRAD_TOL = 2e-6, 2e-5
CASES = ("v4", "multi", "c20", "c20_odd", "plane", "half_sum", "gamma0", "sat_g2", "sat_g15")
_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = np.load(os.path.join(HERE, "golden", "focal.npz"))
    return _golden


def case(name):
    g = golden()
    alpha = torch.from_numpy(g[f"{name}_alpha"])
    return {"z": torch.from_numpy(g[f"{name}_logits"]), "lab": torch.from_numpy(g[f"{name}_labels"].astype(np.int64)),
            "alpha": alpha if alpha.numel() else None, "gamma": float(g[f"{name}_gamma"]), "mean": bool(g[f"{name}_mean"]),
            "focal": float(g[f"{name}_focal"]), "focal_grad": torch.from_numpy(g[f"{name}_focal_grad"]),
            "dice": float(g[f"{name}_dice"]), "dice_grad": torch.from_numpy(g[f"{name}_dice_grad"])}


def close(got, want):
    print(f"    loss {got!r} against {want!r}: relative {abs(got - want) / abs(want):.2e}")
    return abs(got - want) <= LOSS_RTOL * abs(want)


def grad_close(got, want):
    e = relerr(got, want)
    print(f"    gradient relerr {e:.2e}")
    return e < GRAD_TOL


def to(dev, t):
    return None if t is None else t.to(dev)


def f64_losses(z32, lab, alpha, gamma, wf_sum=0.0, wf_mean=0.0, wd=0.0):
    """float64 (focal sum, focal mean, Dice) from the formulas, and the gradient of wf_sum * sum + wf_mean * mean + wd * Dice.  A
    label outside [0, C) has an all-zero one-hot row and weight 0: it adds nothing but its softmax to SP; the mean divides by
    all N * S voxels."""
    z = z32.double().requires_grad_(True)
    N, C = int(z.shape[0]), int(z.shape[1])
    zf, y = z.reshape(N, C, -1), lab.reshape(N, -1)
    onehot = (torch.arange(C)[None, :, None] == y[:, None, :]).double()
    ok = ((y >= 0) & (y < C)).double()
    P, logP = torch.softmax(zf, 1), torch.log_softmax(zf, 1)
    logp = (logP * onehot).sum(1)
    q = (P * (1.0 - onehot)).sum(1)
    a = ok if alpha is None else alpha.double()[y.clamp(0, C - 1)] * ok
    fsum = (-a * q.pow(gamma) * logp).sum() if gamma != 0 else (-a * logp).sum()
    fmean = fsum / y.numel()
    eps = float(np.float32(1e-5))
    TP, SP, CNT = (P * onehot).sum((0, 2)), P.sum((0, 2)), onehot.sum((0, 2))
    FP, FN = SP - TP, CNT - TP
    al = torch.clamp(FP / (FP + FN + eps), 0.2, 0.8)
    dice = (1.0 - TP / (TP + al * FP + (1.0 - al) * FN + eps)).mean()
    (wf_sum * fsum + wf_mean * fmean + wd * dice).backward()
    return float(fsum.detach()), float(fmean.detach()), float(dice.detach()), z.grad


def run_fn(dev, z32, lab, alpha, gamma, with_dice, wf_sum=0.0, wf_mean=0.0, wd=0.0):
    z = z32.to(dev).clone().requires_grad_(True)
    out = Fn.FocalFn.apply(z, lab.to(dev), to(dev, alpha), gamma, with_dice)
    loss = wf_sum * out[0] + wf_mean * out[1] + wd * out[2]
    loss.backward()
    return out.detach().cpu(), float(loss.detach()), z.grad.cpu()


# ---- 1. the fixture cases through FocalLoss ----------------------------------------------------------------------------------------

def check_fixture_case(dev, name):
    c = case(name)
    C = int(c["z"].shape[1])
    crit = FocalLoss(C, alpha=c["alpha"], gamma=c["gamma"], size_average=c["mean"]).to(dev)
    z = c["z"].to(dev).clone().requires_grad_(True)
    loss = crit(z, c["lab"].to(dev))
    loss.backward()
    loss = loss.detach()
    assert loss.dim() == 0 and close(float(loss), c["focal"])
    assert grad_close(z.grad.cpu(), c["focal_grad"])
    if c["gamma"] == 0 and c["alpha"] is None and c["mean"]:
        zr = c["z"].double().requires_grad_(True)
        ce = F.cross_entropy(zr, c["lab"])
        ce.backward()
        assert close(float(loss), float(ce.detach())) and grad_close(z.grad.cpu(), zr.grad)
    # the float64 formulation of this file gives what the reference gave (it stands in for it on the shapes outside the fixture)
    fs, fm, dl, g = f64_losses(c["z"], c["lab"], c["alpha"], c["gamma"], wf_mean=float(c["mean"]), wf_sum=float(not c["mean"]))
    # (the reference's DiceLoss rounds its three class sums to float32, losses.py:43-44, whatever the logits' type: 3 * 2^-24)
    assert abs((fm if c["mean"] else fs) - c["focal"]) <= 1e-12 * abs(c["focal"]) and abs(dl - c["dice"]) <= 2e-7
    assert relerr(g, c["focal_grad"]) < 1e-11


# ---- 2. focal + Dice in one pass -----------------------------------------------------------------------------------------------------

def check_dice_focal(dev, name):
    c = case(name)
    C = int(c["z"].shape[1])
    lab1 = c["lab"].unsqueeze(1)
    wf = {"wf_mean": 0.7} if c["mean"] else {"wf_sum": 0.7}
    out, loss, g = run_fn(dev, c["z"], lab1, c["alpha"], c["gamma"], True, wd=1.3, **wf)
    assert close(float(out[1 if c["mean"] else 0]), c["focal"]) and close(float(out[2]), c["dice"])
    assert close(loss, 0.7 * c["focal"] + 1.3 * c["dice"])
    assert grad_close(g, 0.7 * c["focal_grad"] + 1.3 * c["dice_grad"])
    if c["mean"]:       # the module: FocalLoss(...)(logits, label.squeeze(1)) + DiceLoss()(logits, label)
        crit = DiceFocalLoss(C, alpha=c["alpha"], gamma=c["gamma"]).to(dev)
        z = c["z"].to(dev).clone().requires_grad_(True)
        v = crit(z, lab1.to(dev))
        v.backward()
        v = v.detach()
        assert close(float(v), c["focal"] + c["dice"]) and grad_close(z.grad.cpu(), c["focal_grad"] + c["dice_grad"])


def check_two_modules_agree(dev):
    """DiceFocalLoss against the engine's own FocalLoss + DiceLoss as two modules (the Dice term bit for bit)."""
    c = case("multi")
    z, lab1 = c["z"].to(dev), c["lab"].unsqueeze(1).to(dev)
    one = DiceFocalLoss(6, alpha=c["alpha"], gamma=2).to(dev)(z, lab1)
    fl = FocalLoss(6, alpha=c["alpha"], gamma=2).to(dev)(z, lab1.squeeze(1))
    dl = DiceLoss()(z, lab1)
    assert torch.equal(one, fl + dl)


# ---- 3. bit equality with the CE + Dice kernels --------------------------------------------------------------------------------------

def check_dice_bits(dev):
    for name in ("multi", "c20", "c20_odd"):
        c = case(name)
        C = int(c["z"].shape[1])
        z, lab = c["z"].to(dev), c["lab"].to(dev)
        out, coef = ops.focal_fwd(z, lab, to(dev, c["alpha"]), c["gamma"], True)
        out0, coef0 = ops.dice_ce_fwd(z, lab, None)
        assert torch.equal(out[2], out0[1])
        assert torch.equal(coef[:2 * C], coef0[:2 * C])
        assert torch.equal(coef[2 * C + 1:], coef0[2 * C + 1:])          # the per-class terms 1 - dice_c


# ---- 4. saturation -------------------------------------------------------------------------------------------------------------------

def check_saturation(dev):
    c = case("sat_g15")
    assert float(c["z"].abs().max()) > 60
    for with_dice in (False, True):
        out, loss, g = run_fn(dev, c["z"], c["lab"], None, 0.5, with_dice, wf_mean=1.0, wd=1.0)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all()) and float(out[1]) > 0
    # q = 0 exactly (every other class underflows): loss 0 and gradient 0 at that voxel for gamma > 0, plain CE for gamma = 0
    z = torch.zeros(1, 4, 8)
    z[0, 1] = 200.0
    lab = torch.ones(1, 8, dtype=torch.int64)
    for gamma in (0.5, 1.0, 1.5, 2.0, 3.0):
        out, loss, g = run_fn(dev, z, lab, None, gamma, False, wf_sum=1.0)
        assert float(out[0]) == 0.0 and bool((g == 0).all())
    # p -> 0 (the labelled class far below the maximum): q = 1, the loss is -log p = 200 per voxel
    lab0 = torch.zeros(1, 8, dtype=torch.int64)
    for gamma in (0.0, 0.5, 2.0):
        out, loss, g = run_fn(dev, z, lab0, None, gamma, False, wf_mean=1.0)
        assert bool(torch.isfinite(g).all()) and abs(float(out[1]) - 200.0) <= 200.0 * LOSS_RTOL


# ---- 5. misaligned base pointer -------------------------------------------------------------------------------------------------------

def check_misaligned(dev):
    for name in ("v4", "c20"):
        c = case(name)
        z = c["z"].to(dev)
        buf = torch.empty(z.numel() + 1, dtype=torch.float32, device=dev)
        zm = buf[1:].view(z.shape)
        zm.copy_(z)
        assert zm.data_ptr() % 8 == 4 and zm.is_contiguous()
        lab, alpha = c["lab"].to(dev), to(dev, c["alpha"])
        g2 = torch.tensor([0.7 / c["lab"].numel(), 1.3], device=dev)
        for with_dice in (False, True):
            out_a, coef_a = ops.focal_fwd(z, lab, alpha, c["gamma"], with_dice)
            out_m, coef_m = ops.focal_fwd(zm, lab, alpha, c["gamma"], with_dice)
            assert close(float(out_m[1]), float(out_a[1].double()))
            assert close(float(out_m[1]), c["focal"])
            if with_dice:
                assert close(float(out_m[2]), float(out_a[2].double())) and close(float(out_m[2]), c["dice"])
            dz_a = ops.focal_bwd(z, lab, alpha, coef_a, g2, c["gamma"], with_dice)
            dz_m = ops.focal_bwd(zm, lab, alpha, coef_m, g2, c["gamma"], with_dice)
            assert grad_close(dz_m.cpu(), dz_a.cpu())
            assert grad_close(dz_m.cpu(), 0.7 * c["focal_grad"] + (1.3 * c["dice_grad"] if with_dice else 0.0))


# ---- 6. labels outside [0, C) ---------------------------------------------------------------------------------------------------------

def _bad(lab, C):
    lab2 = lab.clone()
    lab2[0, -1, -1, -3:] = C + 5
    lab2[-1, 0, 0, 0] = -1
    return lab2


def check_bad_labels(dev):
    c = case("v4")
    C, n = 6, c["lab"].numel()
    torch.manual_seed(3)
    alpha = torch.rand(C) + 0.5
    lab2 = _bad(c["lab"], C)
    z = c["z"].to(dev)
    for gamma in (2.0, 0.0, 1.5):
        out, coef = ops.focal_fwd(z, lab2.to(dev), alpha.to(dev), gamma, True)
        assert float(out[3]) == 4.0 and all(bool(torch.isfinite(t).all()) for t in (out, coef))
        g2 = torch.tensor([0.7 / n, 1.3], device=dev)
        dz = ops.focal_bwd(z, lab2.to(dev), alpha.to(dev), coef, g2, gamma, True)
        assert bool(torch.isfinite(dz).all())
        fs, fm, dl, g = f64_losses(c["z"], lab2, alpha, gamma, wf_mean=0.7, wd=1.3)   # those voxels' contribution removed
        assert close(float(out[0]), fs) and close(float(out[1]), fm) and close(float(out[2]), dl)
        assert grad_close(dz.cpu(), g)
        out1, _ = ops.focal_fwd(z, lab2.to(dev), alpha.to(dev), gamma, False)
        assert float(out1[3]) == 4.0 and torch.equal(out1[:2], out[:2]) and torch.equal(out[4], out[1] + out[2])
    assert float(ops.focal_fwd(z, c["lab"].to(dev), None, 2.0, False)[0][3]) == 0.0


def check_bad_labels_through_modules(dev):
    """The first calls raise on the spot; later ones are counted on the device and check_labels() reports them, for the new modules
    as for DiceCELoss."""
    c = case("v4")
    z, lab2 = c["z"].to(dev), _bad(c["lab"], 6).to(dev)
    fl, dfl, dce = FocalLoss(6).to(dev), DiceFocalLoss().to(dev), DiceCELoss().to(dev)
    mode = Fn._CHECK_LABELS
    Fn._CHECK_LABELS = "first"
    try:
        try:
            check_labels()                    # re-arm the on-the-spot checks, whatever ran before
        except IndexError:
            pass
        with pytest.raises(IndexError, match="4 label"):
            fl(z, lab2)
        with pytest.raises(IndexError, match="4 label"):
            dfl(z, lab2.unsqueeze(1))
        assert check_labels() == 0
        for _ in range(4):                    # use up the on-the-spot checks on clean labels
            fl(z, c["lab"].to(dev))
        assert bool(torch.isfinite(fl(z, lab2)))
        assert bool(torch.isfinite(dfl(z, lab2.unsqueeze(1))))
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


# ---- 7. reproducibility -----------------------------------------------------------------------------------------------------------------

def check_reproducible(dev):
    c = case("multi")
    z, lab, alpha = c["z"].to(dev), c["lab"].to(dev), to(dev, c["alpha"])
    g2 = torch.tensor([0.7 / c["lab"].numel(), 1.3], device=dev)
    for gamma, with_dice in ((2.0, True), (2.0, False), (1.5, True)):
        runs = []
        for _ in range(2):
            out, coef = ops.focal_fwd(z, lab, alpha, gamma, with_dice)
            runs.append((out, coef, ops.focal_bwd(z, lab, alpha, coef, g2, gamma, with_dice)))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][2], runs[1][2])
        if with_dice:
            assert torch.equal(runs[0][1], runs[1][1])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------

def check_bad_arguments(dev):
    L = _lib.lib()
    N, C, S = 2, 4, 64
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    z, lab = torch.randn(N, 33, S).to(dev), torch.zeros(N, S, dtype=torch.int64).to(dev)
    out, coef = torch.full((5,), -7.0).to(dev), torch.full((3 * 33 + 1,), -7.0).to(dev)
    dz, g2 = torch.full((N, 33, S), -7.0).to(dev), torch.ones(2).to(dev)
    nbytes = L.cbim_focal_workspace(N, 33, S)
    ws = torch.empty(nbytes, dtype=torch.uint8).to(dev)
    st = ops._stream(z)

    def fwd(zt=z, labt=lab, gamma=2.0, Cc=C, outt=out, coeft=coef, wst=ws, wb=nbytes, dice=1):
        return L.cbim_focal_fwd(p(zt), p(labt), None, gamma, dice, N, Cc, S, p(outt), p(coeft), p(wst), wb, st)

    def bwd(zt=z, gamma=2.0, Cc=C, coeft=coef, g2t=g2, dzt=dz, dice=1):
        return L.cbim_focal_bwd(p(zt), p(lab), None, p(coeft), p(g2t), p(dzt), gamma, dice, N, Cc, S, st)

    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    assert fwd(Cc=33) == EUNSUPPORTED and bwd(Cc=33) == EUNSUPPORTED
    assert fwd(zt=None) == EINVAL and fwd(labt=None) == EINVAL and fwd(outt=None) == EINVAL and fwd(coeft=None) == EINVAL
    assert bwd(zt=None) == EINVAL and bwd(g2t=None) == EINVAL and bwd(dzt=None) == EINVAL and bwd(coeft=None) == EINVAL
    assert fwd(gamma=-0.5) == EINVAL and bwd(gamma=-0.5) == EINVAL and fwd(gamma=float("nan")) == EINVAL
    assert fwd(wb=L.cbim_focal_workspace(N, C, S) - 1) == EWORKSPACE and fwd(wst=None) == EWORKSPACE
    if dev == "cuda":
        torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((coef == -7.0).all()) and bool((dz == -7.0).all())      # nothing was launched
    assert fwd(coeft=None, dice=0) == 0 and bwd(coeft=None, dice=0) == 0                               # coef is optional without Dice
    with pytest.raises(RuntimeError, match="up to 32 classes"):
        ops.focal_fwd(z, lab, None, 2.0, False)
    with pytest.raises(ValueError):
        FocalLoss(3, gamma=-1)
    with pytest.raises(ValueError):
        FocalLoss(3, alpha=[1.0, 2.0])
    with pytest.raises(ValueError):
        DiceFocalLoss(3, alpha=[1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError):
        DiceFocalLoss(alpha=[1.0, 2.0, 3.0])            # a table needs the class count it is checked against
    with pytest.raises(ValueError):
        DiceFocalLoss(gamma=float("nan"))
    with pytest.raises(ValueError):
        FocalLoss(3).to(dev)(torch.zeros(1, 4, 8).to(dev), torch.zeros(1, 8, dtype=torch.int64).to(dev))
    crit = FocalLoss(3, alpha=[0.25, 0.5, 1.0])
    assert "alpha" in dict(crit.named_buffers()) and crit.alpha.dtype == torch.float32      # .to(device) moves the table


# ---- 9. target shapes, spatial ranks ----------------------------------------------------------------------------------------------------

def check_target_shapes_and_ranks(dev):
    torch.manual_seed(21)
    for C, sp in ((5, (37,)), (3, (9, 11)), (4, (3, 4, 5)), (3, (2, 3, 2, 4))):
        z32 = torch.randn(2, C, *sp) * 2
        lab = torch.randint(0, C, (2,) + sp)
        alpha = torch.rand(C) + 0.5
        fs, fm, dl, g = f64_losses(z32, lab, alpha, 2.0, wf_mean=1.0)
        crit = FocalLoss(C, alpha=alpha, gamma=2).to(dev)
        vals = []
        for t in (lab, lab.unsqueeze(1), lab.int()):
            z = z32.to(dev).clone().requires_grad_(True)
            v = crit(z, t.to(dev))
            v.backward()
            vals.append((v.detach(), z.grad))
        assert close(float(vals[0][0]), fm) and grad_close(vals[0][1].cpu(), g)
        assert all(torch.equal(vals[0][0], v) and torch.equal(vals[0][1], gz) for v, gz in vals[1:])
        fs, fm, dl, g = f64_losses(z32, lab, alpha, 2.0, wf_mean=1.0, wd=1.0)
        z = z32.to(dev).clone().requires_grad_(True)
        v = DiceFocalLoss(C, alpha=alpha).to(dev)(z, lab.unsqueeze(1).to(dev))
        v.backward()
        assert close(float(v.detach()), fm + dl) and grad_close(z.grad.cpu(), g)
    # summed, and under autocast (disabled inside the modules: bf16 logits are taken to float32, the loss stays float32)
    z32, lab = torch.randn(2, 4, 6, 8) * 2, torch.randint(0, 4, (2, 6, 8))
    fs, fm, dl, g = f64_losses(z32, lab, None, 1.0, wf_sum=1.0)
    z = z32.to(dev).clone().requires_grad_(True)
    with torch.autocast(device_type="cuda" if dev == "cuda" else "cpu", dtype=torch.bfloat16):
        v = FocalLoss(4, gamma=1, size_average=False).to(dev)(z, lab.to(dev))
    v.backward()
    assert v.dtype == torch.float32 and close(float(v.detach()), fs) and grad_close(z.grad.cpu(), g)


# ---- 10. GPU: a benchmark-like size -----------------------------------------------------------------------------------------------------

def check_size(dev, N=1, C=16, dhw=(32, 32, 32)):
    torch.manual_seed(31)
    z32 = torch.randn(N, C, *dhw) * 2
    lab = torch.randint(0, C, (N,) + dhw)
    lab[:, :2] = 0
    alpha = torch.rand(C) + 0.5
    fs, fm, dl, g = f64_losses(z32, lab, alpha, 2.0, wf_mean=0.7, wd=1.3)
    out, loss, gz = run_fn(dev, z32, lab.unsqueeze(1), alpha, 2.0, True, wf_mean=0.7, wd=1.3)
    assert close(float(out[1]), fm) and close(float(out[2]), dl) and close(loss, 0.7 * fm + 1.3 * dl) and grad_close(gz, g)
    out0 = ops.dice_ce_fwd(z32.to(dev), lab.to(dev), None)[0]
    assert torch.equal(out[2].cpu(), out0[1].cpu())


# ---- 11. GPU: graph capture -------------------------------------------------------------------------------------------------------------

def check_graph_capture(dev):
    c = case("multi")
    crit = DiceFocalLoss(6, alpha=c["alpha"], gamma=2).to(dev)
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
    for _ in range(2):
        loss.zero_()
        z.grad.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss, eager_loss) and torch.equal(z.grad, eager_grad)
