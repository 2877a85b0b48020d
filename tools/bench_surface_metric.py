"""Timing of the surface-distance metrics (ASD / HD95) on the GPU: the procedural CT-sized pair (160x320x320, 16 classes, spacing
2.0/0.8/0.8) and case C of the tests (128^3, 16 classes).  Prints one JSON line:
    python tools/bench_surface_metric.py [--reps 7] [--inference]
device_ms: HIP-event time of surface_distances (scan, readback of boxes, the four list launches, readback of the lists), warmed,
median of --reps; tail_ms: the numpy float64 tail of calculate_distance on the lists (area lookup, lexsort, sums); points: surface
points over all classes and both directions.  The area table is the fixture's (spacing 2.5/0.8/1.25): it only feeds the timing
of the tail.  --inference adds the sliding-window inference (ResUNet base 32, 128^3 windows, bf16) of the same volumes."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402
from cbim_amd.metric import utils as mu  # noqa: E402
from cbim_amd.metric.surface import surface_distances  # noqa: E402
from tests import surface_checks as sc  # noqa: E402
from tests.util import load_golden  # noqa: E402


def one(case, reps, table, inference):
    pred, gt = sc.ellipsoid_pair(case["shape"], case["classes"], case["seed"])
    p, t = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    sp = torch.tensor(case["spacing"])
    dev_ms, wall_ms, tail_ms = [], [], []
    for it in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        e0.record()
        lists = surface_distances(p, t, sp, case["classes"])
        e1.record()
        torch.cuda.synchronize()
        w1 = time.perf_counter()
        for s in lists:
            for a, b in (("distances_gt_to_pred", "codes_gt"), ("distances_pred_to_gt", "codes_pred")):
                d, ar = mu._sorted_surfels(s[a], s[b], table)
                if len(d):
                    np.sum(d * ar) / np.sum(ar)
                    mu._percentile_distance(d, ar, 95)
        w2 = time.perf_counter()
        if it >= 2:
            dev_ms.append(e0.elapsed_time(e1)); wall_ms.append((w1 - w0) * 1e3); tail_ms.append((w2 - w1) * 1e3)
    out = dict(shape=list(case["shape"]), classes=case["classes"], device_ms=round(statistics.median(dev_ms), 3),
               wall_ms=round(statistics.median(wall_ms), 3), tail_ms=round(statistics.median(tail_ms), 3),
               points=int(sum(len(s["codes_gt"]) + len(s["codes_pred"]) for s in lists)))
    if inference:
        from cbim_amd.inference.inference3d import inference_sliding_window
        from cbim_amd.model.dim3 import UNet
        cbim_amd.set_compute_dtype("bf16")
        net = UNet(1, 32, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=case["classes"], block="BasicBlock",
                   norm="in").cuda()
        args = argparse.Namespace(window_size=[128, 128, 128], classes=case["classes"])
        x = torch.randn((1, 1) + tuple(case["shape"]), device="cuda")
        ms = []
        for it in range(3):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            inference_sliding_window(net, x, args, return_labels=True)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - w0) * 1e3)
        cbim_amd.set_compute_dtype(None)
        out["sliding_window_inference_ms"] = round(min(ms[1:]), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inference", action="store_true")
    a = ap.parse_args()
    table = load_golden("surface_large")["table"]
    res = {"bench": "surface_metric", "device": torch.cuda.get_device_name(0),
           "ct": one(sc.CASE_CT, a.reps, table, a.inference), "case_c": one(sc.CASE_C, a.reps, table, a.inference)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
