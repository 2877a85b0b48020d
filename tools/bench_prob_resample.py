"""Timing of the fused probability resampling (cbim_resample_argmax) on the GPU next to the composition it replaces:
    python tools/bench_prob_resample.py [--reps 20] [--warmup 5] [--out profiles/prob_resample.json]
Shapes: 16 classes, a 160x320x320 probability volume at the training spacing, a 320x512x512 scan grid (spacings 2.0 / 1.6 / 1.6
against 1.0, same origin).  fused: resample_argmax on the probabilities; fused_counter: the same on sliding-window sums with
their count; composition: resample3d 'linear' over the 16 channels, torch.argmax, the cast to uint8 — in the same process, each
the median of --reps HIP-event timings after --warmup runs.  Bytes are what the algorithm has to move, computed from the shapes
(fused: the source once and one byte per output voxel; composition: also the K float32 volumes written and read again and the
int64 argmax written and read); bytes/s is that over the time, not a counter reading.  The labels of the two are compared at the
timed size (equal wherever the composed top-two margin exceeds 1e-6)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402,F401
from cbim_amd.inference import resample as rs  # noqa: E402

K, SRC, DST = 16, (160, 320, 320), (320, 512, 512)
SRC_SPACING, DST_SPACING = (1.6, 1.6, 2.0), (1.0, 1.0, 1.0)


def timed(fn, reps, warmup):
    ms = []
    for it in range(reps + warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        del out
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "prob_resample.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prob_resample: needs a GPU")
    gen = torch.Generator(device="cuda").manual_seed(11)
    prob = torch.softmax(4 * torch.randn((K,) + SRC, generator=gen, device="cuda"), 0)
    counter = torch.randint(1, 9, SRC, generator=gen, device="cuda").float()
    sums = prob * counter
    zero = (0.0, 0.0, 0.0)
    m = rs.index_map((SRC_SPACING, zero, rs.IDENTITY), (DST_SPACING, zero, rs.IDENTITY))
    n_src, n_dst = SRC[0] * SRC[1] * SRC[2], DST[0] * DST[1] * DST[2]
    fused = lambda: rs.resample_argmax(prob, m, DST)                                               # noqa: E731
    fused_c = lambda: rs.resample_argmax(sums, m, DST, counter=counter)                            # noqa: E731
    composed = lambda: rs.resample3d(prob, m, DST, "linear").argmax(0).to(torch.uint8)             # noqa: E731
    # same labels at the timed size
    comp = rs.resample3d(prob, m, DST, "linear")
    top2 = comp.topk(2, dim=0).values
    clear = (top2[0] - top2[1]) > 1e-6
    want = comp.argmax(0)
    del comp, top2
    got = fused()
    mismatches = int(((got.long() != want) & clear).sum())
    unclear = int((~clear).sum())
    del want, clear, got
    t_f, t_c, t_fc = timed(fused, a.reps, a.warmup), timed(composed, a.reps, a.warmup), timed(fused_c, a.reps, a.warmup)
    b_f = 4 * K * n_src + n_dst
    b_fc = b_f + 4 * n_src
    b_c = 4 * K * n_src + 2 * 4 * K * n_dst + 2 * 8 * n_dst + n_dst
    res = {"bench": "prob_resample", "device": torch.cuda.get_device_name(0), "classes": K, "source": list(SRC), "destination": list(DST),
           "reps": a.reps, "warmup": a.warmup,
           "fused_ms": t_f[0], "fused_min_max_ms": t_f[1:], "fused_counter_ms": t_fc[0], "fused_counter_min_max_ms": t_fc[1:],
           "composition_ms": t_c[0], "composition_min_max_ms": t_c[1:],
           "composition_over_fused": round(t_c[0] / t_f[0], 2), "composition_over_fused_counter": round(t_c[0] / t_fc[0], 2),
           "fused_algorithm_bytes": b_f, "composition_algorithm_bytes": b_c,
           "fused_GBps": round(b_f / t_f[0] / 1e6, 1), "fused_counter_GBps": round(b_fc / t_fc[0] / 1e6, 1),
           "composition_GBps": round(b_c / t_c[0] / 1e6, 1),
           "label_mismatches_on_clear_voxels": mismatches, "voxels_outside_or_under_1e-6_margin": unclear}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
