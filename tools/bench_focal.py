"""Timing of the one-pass Dice + focal loss (cbim_focal_fwd / cbim_focal_bwd) on the GPU next to its yardstick and its alternatives:
    python tools/bench_focal.py [--reps 30] [--warmup 5] [--out profiles/focal.json]
Sizes: logits 1x16x128^3 and 2x4x16x192x192 (the ACDC shape), float32, labels int64 [N,1,...].  Each variant is one forward and one
backward of a scalar loss, timed with HIP events around both; the four variants alternate inside every repetition (same process,
same tensors), each timed call right after an untimed call of the same variant (otherwise the variant that follows torch_ops finds
the logits evicted from the Infinity Cache and the one after it finds them warm), and the figure is the median of --reps repetitions
after --warmup:
  dice_focal   DiceFocalLoss(C, alpha, gamma=2)                                    one pass forward, one backward
  dice_ce      DiceCELoss(weight) on the same tensors: THE YARDSTICK, the kernels that move the same bytes
  two_modules  FocalLoss(C, alpha, 2)(z, y.squeeze(1)) + DiceLoss()(z, y)          the engine's kernels, two passes each way
  torch_ops    focal + Dice written from their formulas with torch ops on the device (softmax, log-softmax, one-hot, products)
Bytes are what the one-pass algorithm has to move, computed from the shapes: forward C * 4 + 8 per voxel, backward 2 * C * 4 + 8;
bytes/s is that over the time of forward + backward, launches and the autograd glue included — not a kernel's rate.  At these sizes
a single forward + backward leaves the device waiting for the host between launches, so the kernels of dice_focal and dice_ce are
also timed alone (ops_*): 10 forward + backward pairs through ops between one pair of events, per pair.
The values of the variants are compared at the timed size before timing."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402,F401
from cbim_amd import ops  # noqa: E402
from cbim_amd.training.losses import DiceCELoss, DiceFocalLoss, DiceLoss, FocalLoss  # noqa: E402

SIZES = {"1x16x128x128x128": (1, 16, (128, 128, 128)), "2x4x16x192x192": (2, 4, (16, 192, 192))}
GAMMA = 2.0
BATCH = 10


def torch_ops_loss(z, y1, alpha):
    """Focal (mean) + Dice from the formulas, as a composition of full-size torch ops."""
    C = z.shape[1]
    P, logP = torch.softmax(z, 1), torch.log_softmax(z, 1)
    mask = torch.zeros_like(z).scatter_(1, y1, 1.0)
    p, logp = (P * mask).sum(1), (logP * mask).sum(1)
    focal = (-alpha[y1.squeeze(1)] * (1 - p).pow(GAMMA) * logp).mean()
    dims = [0] + list(range(2, z.dim()))
    TP, SP, CNT = (P * mask).sum(dims), P.sum(dims), mask.sum(dims)
    FP, FN = SP - TP, CNT - TP
    a = torch.clamp(FP / (FP + FN + 1e-5), 0.2, 0.8)
    return focal + (1 - TP / (TP + a * FP + (1 - a) * FN + 1e-5)).sum() / C


def one_size(name, N, C, sp, reps, warmup):
    gen = torch.Generator(device="cuda").manual_seed(17)
    z = (2 * torch.randn((N, C) + sp, generator=gen, device="cuda")).requires_grad_(True)
    y1 = torch.randint(0, C, (N, 1) + sp, generator=gen, device="cuda")
    y1[:, :, :2] = 0
    alpha = torch.rand(C, generator=gen, device="cuda") + 0.5
    dfl, dce = DiceFocalLoss(C, alpha=alpha, gamma=GAMMA).cuda(), DiceCELoss(alpha).cuda()
    fl, dl = FocalLoss(C, alpha=alpha, gamma=GAMMA).cuda(), DiceLoss()
    variants = {"dice_focal": lambda: dfl(z, y1), "dice_ce": lambda: dce(z, y1),
                "two_modules": lambda: fl(z, y1.squeeze(1)) + dl(z, y1), "torch_ops": lambda: torch_ops_loss(z, y1, alpha)}
    values = {k: float(f().detach()) for k, f in variants.items()}
    ms = {k: [] for k in variants}
    for it in range(reps + warmup):
        for k, f in variants.items():
            z.grad = None
            f().backward()          # untimed: every timed call follows a call of its own variant (same cache state for all four)
            z.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f().backward()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    # the kernels alone: BATCH forward + backward pairs through ops between one pair of events, so the queue stays full and the
    # launches' host side hides behind the kernels; per pair, alternating the two families
    zd, y = z.detach(), y1.squeeze(1).contiguous()
    g2 = torch.tensor([1.0 / y.numel(), 1.0], device="cuda")

    def pair_focal():
        out, coef = ops.focal_fwd(zd, y, alpha, GAMMA, True)
        return ops.focal_bwd(zd, y, alpha, coef, g2, GAMMA, True)

    def pair_ce():
        out, coef = ops.dice_ce_fwd(zd, y, alpha)
        return ops.dice_ce_bwd(zd, y, alpha, coef, g2)

    kms = {"ops_dice_focal": [], "ops_dice_ce": []}
    for it in range(reps + warmup):
        for k, f in (("ops_dice_focal", pair_focal), ("ops_dice_ce", pair_ce)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                f()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                kms[k].append(e0.elapsed_time(e1) / BATCH)
    kmed = {k: statistics.median(v) for k, v in kms.items()}
    voxels = N * sp[0] * sp[1] * sp[2]
    nbytes = voxels * ((C * 4 + 8) + (2 * C * 4 + 8))
    res = {"classes": C, "voxels": voxels, "one_pass_algorithm_bytes": nbytes, "values": {k: round(v, 7) for k, v in values.items()}}
    for k in variants:
        res[f"{k}_ms"] = round(med[k], 4)
        res[f"{k}_min_max_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    for k in kms:
        res[f"{k}_pair_ms"] = round(kmed[k], 4)
        res[f"{k}_pair_min_max_ms"] = [round(min(kms[k]), 4), round(max(kms[k]), 4)]
    res["ops_dice_focal_over_ops_dice_ce"] = round(kmed["ops_dice_focal"] / kmed["ops_dice_ce"], 4)
    res["ops_dice_focal_GBps"], res["ops_dice_ce_GBps"] = round(nbytes / kmed["ops_dice_focal"] / 1e6, 1), round(nbytes / kmed["ops_dice_ce"] / 1e6, 1)
    ratio = med["dice_focal"] / med["dice_ce"]
    res.update({"dice_focal_over_dice_ce": round(ratio, 4), "within_10_percent_of_dice_ce": bool(0.9 <= ratio <= 1.1),
                "two_modules_over_dice_focal": round(med["two_modules"] / med["dice_focal"], 3),
                "torch_ops_over_dice_focal": round(med["torch_ops"] / med["dice_focal"], 3),
                "dice_focal_GBps": round(nbytes / med["dice_focal"] / 1e6, 1), "dice_ce_GBps": round(nbytes / med["dice_ce"] / 1e6, 1),
                "two_modules_minus_dice_focal_value": values["two_modules"] - values["dice_focal"],
                "torch_ops_minus_dice_focal_value": values["torch_ops"] - values["dice_focal"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "focal.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_focal: needs a GPU")
    res = {"bench": "focal", "device": torch.cuda.get_device_name(0), "gamma": GAMMA, "reps": a.reps, "warmup": a.warmup,
           "timed": "forward + backward, HIP events, median; variants alternate inside each repetition", "sizes": {}}
    for name, (N, C, sp) in SIZES.items():
        res["sizes"][name] = one_size(name, N, C, sp, a.reps, a.warmup)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
