"""Timing of the connected-component filter on the GPU, per stage and whole, next to scipy on the same volume:
    python tools/bench_components.py [--reps 9] [--out profiles/components.json]
Volumes: the procedural CT-sized label map (160x320x320, 16 classes: ellipsoids plus 0.2 % salt noise) and the worst case for the
atomics (dense random noise, p = 0.5, 26-connectivity: one giant component through every tile face).  Each figure is the median of
--reps HIP-event timings after two warm-up runs, buffers allocated beforehand.  scipy_ms: ndimage.label per class + bincount + mask
on the host, timed once by this script when scipy is importable, else null."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402,F401
from cbim_amd import _lib  # noqa: E402
from cbim_amd.inference import components as cc  # noqa: E402
from cbim_amd.ops import _p, _stream  # noqa: E402

SHAPE = (160, 320, 320)


def ct_volume(classes=16, seed=3):
    rng = np.random.default_rng(seed)
    D, H, W = SHAPE
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij", sparse=True)
    v = np.zeros(SHAPE, np.uint8)
    for c in range(1, classes):
        cz, cy, cx = rng.uniform(0.15, 0.85, 3) * SHAPE
        rz, ry, rx = rng.uniform(0.06, 0.16, 3) * SHAPE
        v[((z - cz) / rz) ** 2 + ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0] = c
    salt = rng.random(SHAPE) < 0.002
    v[salt] = rng.integers(1, classes, int(salt.sum()), dtype=np.uint8)
    return v


def noise_volume(seed=4):
    return (np.random.default_rng(seed).random(SHAPE) < 0.5).astype(np.uint8)


def scipy_ms(vol, rank, min_size):
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    t0 = time.perf_counter()
    out = vol.copy()
    st = ndi.generate_binary_structure(3, rank)
    for c in np.unique(vol[vol > 0]):
        comp, n = ndi.label(vol == c, st)
        sizes = np.bincount(comp.ravel(), minlength=n + 1)
        sizes[0] = 0
        keep = np.zeros(n + 1, bool)
        keep[np.argmax(sizes)] = sizes.max() >= min_size
        out[(vol == c) & ~keep[comp]] = 0
    return round((time.perf_counter() - t0) * 1e3, 1)


def timed(fn, reps):
    ms = []
    for it in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4)


def one(vol, conn, reps, with_scipy):
    lib = _lib.lib()
    t = torch.from_numpy(vol).cuda()
    D, H, W = SHAPE
    N = t.numel()
    st = _stream(t)
    parent = torch.empty(SHAPE, dtype=torch.int32, device="cuda")
    size = torch.empty(SHAPE, dtype=torch.int32, device="cuda")
    comp = torch.empty(SHAPE, dtype=torch.int32, device="cuda")
    best = torch.empty(256, dtype=torch.int64, device="cuda")
    n = torch.empty(1, dtype=torch.int32, device="cuda")
    scratch = torch.empty(int(lib.cbim_components_workspace_bytes(D, H, W)), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(t)
    keep, mins = cc.filter_tables("all", 50, t.device)
    label = lambda: _lib.check(lib.cbim_components_label(_p(t), D, H, W, conn, _p(parent), st), "label")          # noqa: E731
    sizes = lambda: _lib.check(lib.cbim_components_sizes(_p(t), _p(parent), D, H, W, _p(size), _p(best), st), "sizes")   # noqa: E731
    filt = lambda: _lib.check(lib.cbim_components_filter(_p(t), _p(parent), _p(size), _p(best), _p(keep), _p(mins), _p(out), N, st),   # noqa: E731
                              "filter")
    number = lambda: _lib.check(lib.cbim_components_number(_p(parent), D, H, W, _p(comp), _p(n), _p(scratch), st), "number")   # noqa: E731
    res = {"connectivity": conn, "label_ms": timed(label, reps), "sizes_ms": timed(sizes, reps), "filter_ms": timed(filt, reps),
           "number_ms": timed(number, reps),
           "filter_components_ms": timed(lambda: cc.filter_components(t, keep_largest="all", min_size=50, connectivity=conn, out=out),
                                         reps),
           "components": int(n.item()), "foreground": int((t > 0).sum().item())}
    res["scipy_ms"] = scipy_ms(vol, {6: 1, 18: 2, 26: 3}[conn], 50) if with_scipy else None
    if res["scipy_ms"]:
        res["scipy_over_gpu"] = round(res["scipy_ms"] / res["filter_components_ms"], 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "components.json"))
    a = ap.parse_args()
    res = {"bench": "components", "device": torch.cuda.get_device_name(0), "shape": list(SHAPE),
           "ct_16_classes": one(ct_volume(), 26, a.reps, not a.no_scipy),
           "noise_p50": one(noise_volume(), 26, a.reps, not a.no_scipy)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
