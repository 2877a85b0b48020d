"""Timing of the one-pass Dice + top-k cross-entropy loss (cbim_topk_fwd / cbim_topk_bwd) on the GPU next to its yardstick and the
composition it replaces:
    python tools/bench_topk.py [--reps 30] [--warmup 5] [--k 10] [--out profiles/topk.json]
Sizes: logits 1x16x128^3 and 2x4x16x192x192 (the ACDC shape), float32, labels int64 [N,1,...].  Each variant is one forward and one
backward of a scalar loss, timed with HIP events around both; the variants alternate inside every repetition (same process, same
tensors), each timed call right after an untimed call of the same variant (the method of tools/bench_focal.py), and the figure is
the median of --reps repetitions after --warmup:
  dice_topk    DiceTopKLoss(weight, k)                                             one pass forward + the select, one backward
  dice_ce      DiceCELoss(weight) on the same tensors: THE YARDSTICK for a one-pass loss
  torch_ops    cross_entropy(reduction="none") + torch.topk + the DiceLoss module: the baseline this loss replaces
At these sizes a single forward + backward leaves the device waiting for the host between launches, so the kernels of dice_topk and
dice_ce are also timed alone (ops_*): 10 forward + backward pairs through ops between one pair of events, per pair.
The values of the variants are compared at the timed size before timing, and the distance of the kernels and of the float32 torch
composition to the float64 value of the top-k term is recorded (fp32_parity)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402,F401
from cbim_amd import functional as Fn  # noqa: E402
from cbim_amd import ops  # noqa: E402
from cbim_amd.training.losses import DiceCELoss, DiceLoss, DiceTopKLoss  # noqa: E402

SIZES = {"1x16x128x128x128": (1, 16, (128, 128, 128)), "2x4x16x192x192": (2, 4, (16, 192, 192))}
BATCH = 10


def one_size(name, N, C, sp, k, reps, warmup):
    gen = torch.Generator(device="cuda").manual_seed(17)
    z = (2 * torch.randn((N, C) + sp, generator=gen, device="cuda")).requires_grad_(True)
    y1 = torch.randint(0, C, (N, 1) + sp, generator=gen, device="cuda")
    y1[:, :, :2] = 0
    weight = torch.rand(C, generator=gen, device="cuda") + 0.5
    K = Fn.topk_count(y1.numel(), k)
    dtk, dce, dl = DiceTopKLoss(weight, k=k).cuda(), DiceCELoss(weight).cuda(), DiceLoss()

    def torch_ops_loss():
        nll = F.cross_entropy(z, y1.squeeze(1), weight=weight, reduction="none").reshape(-1)
        return torch.topk(nll, K, sorted=False).values.sum() / K + dl(z, y1)

    variants = {"dice_topk": lambda: dtk(z, y1), "dice_ce": lambda: dce(z, y1), "torch_ops": torch_ops_loss}
    values = {n: float(f().detach()) for n, f in variants.items()}
    # fp32 parity of the top-k term: the kernels and the float32 composition against the float64 composition
    with torch.no_grad():
        nll64 = F.cross_entropy(z.double(), y1.squeeze(1), weight=weight.double(), reduction="none").reshape(-1)
        tk64 = float(torch.topk(nll64, K, sorted=False).values.sum() / K)
        nll32 = F.cross_entropy(z, y1.squeeze(1), weight=weight, reduction="none").reshape(-1)
        tk32 = float(torch.topk(nll32, K, sorted=False).values.sum() / K)
        tkk = float(ops.topk_fwd(z.detach(), y1.squeeze(1).contiguous(), weight, K, False)[0][1])
        del nll64, nll32
    ms = {n: [] for n in variants}
    for it in range(reps + warmup):
        for n, f in variants.items():
            z.grad = None
            f().backward()          # untimed: every timed call follows a call of its own variant (same cache state for all)
            z.grad = None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f().backward()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[n].append(e0.elapsed_time(e1))
    med = {n: statistics.median(v) for n, v in ms.items()}
    # the kernels alone: BATCH forward + backward pairs through ops between one pair of events, per pair, alternating the families
    zd, y = z.detach(), y1.squeeze(1).contiguous()
    g2 = torch.tensor([1.0, 1.0], device="cuda")

    def pair_topk():
        out, coef, ws = ops.topk_fwd(zd, y, weight, K, True)
        return ops.topk_bwd(zd, y, weight, coef, g2, ws, True)

    def pair_ce():
        out, coef = ops.dice_ce_fwd(zd, y, weight)
        return ops.dice_ce_bwd(zd, y, weight, coef, g2)

    kms = {"ops_dice_topk": [], "ops_dice_ce": []}
    for it in range(reps + warmup):
        for n, f in (("ops_dice_topk", pair_topk), ("ops_dice_ce", pair_ce)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                f()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                kms[n].append(e0.elapsed_time(e1) / BATCH)
    kmed = {n: statistics.median(v) for n, v in kms.items()}
    voxels = N * sp[0] * sp[1] * sp[2]
    res = {"classes": C, "voxels": voxels, "k_percent": k, "K": K, "values": {n: round(v, 7) for n, v in values.items()},
           "fp32_parity": {"topk_float64": tk64, "kernels_rel": abs(tkk - tk64) / tk64, "torch_float32_rel": abs(tk32 - tk64) / tk64}}
    for n in variants:
        res[f"{n}_ms"] = round(med[n], 4)
        res[f"{n}_min_max_ms"] = [round(min(ms[n]), 4), round(max(ms[n]), 4)]
    for n in kms:
        res[f"{n}_pair_ms"] = round(kmed[n], 4)
        res[f"{n}_pair_min_max_ms"] = [round(min(kms[n]), 4), round(max(kms[n]), 4)]
    res.update({"dice_topk_over_dice_ce": round(med["dice_topk"] / med["dice_ce"], 4),
                "torch_ops_over_dice_topk": round(med["torch_ops"] / med["dice_topk"], 3),
                "one_pass_beats_the_composition": bool(med["dice_topk"] < med["torch_ops"]),
                "ops_dice_topk_over_ops_dice_ce": round(kmed["ops_dice_topk"] / kmed["ops_dice_ce"], 4),
                "torch_ops_minus_dice_topk_value": values["torch_ops"] - values["dice_topk"]})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--k", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "topk.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk: needs a GPU")
    res = {"bench": "topk", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "timed": "forward + backward, HIP events, median; variants alternate inside each repetition", "sizes": {}}
    for name, (N, C, sp) in SIZES.items():
        res["sizes"][name] = one_size(name, N, C, sp, a.k, a.reps, a.warmup)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
