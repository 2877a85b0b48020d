"""Timing of volume prediction on the GPU, stage by stage.  One CT-like case: 160x320x320 at spacing 0.8/0.8/2.5 mm (x, y, z)
resampled to 1 mm isotropic (400x256x256), 16 classes, the headline ResUNet (base 32) with 128^3 windows in bf16, a 2-model
ensemble.  Prints one JSON line:
    python tools/bench_prediction.py [--reps 5] [--scipy]
Per stage the HIP-event time (warmed, median of --reps) and, for the new kernels, the achieved GB/s against their algorithmic
bytes (percentile: 4 passes over the volume; prefilter: 3 axes x 2 sweeps x read + write; resample: one read of the source + one
write; ensemble tail: prob_sum + total read, total written, labels written; label resample: read + write of 1-byte labels).
`non_network_share`: everything but the models' sliding windows, as a share of the whole.  `stock`: the same stage written with
stock torch on the same box in the same process (torch.quantile is limited to 16M elements, so kthvalue stands in for it).
--scipy adds the CPU time of scipy's cubic resample of the same volume, for scale."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402
from cbim_amd import _lib  # noqa: E402
from cbim_amd import prediction as P  # noqa: E402
from cbim_amd.inference import inference3d  # noqa: E402
from cbim_amd.inference import resample as rs  # noqa: E402
from cbim_amd.ops import _p, _stream  # noqa: E402

SHAPE, SPACING, TARGET, CLASSES, WINDOW, MODELS = (160, 320, 320), (0.8, 0.8, 2.5), (1.0, 1.0, 1.0), 16, [128, 128, 128], 2


def timed(fn, reps):
    ms, out = [], None
    for it in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy", action="store_true")
    a = ap.parse_args()
    from cbim_amd.model.dim3 import UNet
    dev = torch.device("cuda")
    rng = np.random.default_rng(11)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32) for n in SHAPE], indexing="ij")
    raw = np.round(700 * np.exp(-2 * (zz ** 2 + yy ** 2 + xx ** 2)) + rng.standard_normal(SHAPE, dtype=np.float32) * 80 - 200).astype(np.float32)
    img = torch.from_numpy(raw).to(dev)
    lib, st = _lib.lib(), _stream(img)
    out_shape = rs.resampled_size(SHAPE, SPACING, TARGET)
    m = rs.index_map((SPACING, (0, 0, 0), rs.IDENTITY), (TARGET, (0, 0, 0), rs.IDENTITY))
    n_in, n_out = img.numel(), int(np.prod(out_shape))
    res, stock = {}, {}

    coef = torch.empty_like(img)
    ms, _ = timed(lambda: _lib.check(lib.cbim_bspline3_prefilter(_p(img), _p(coef), 1, *SHAPE, st)), a.reps)
    res["prefilter"] = dict(ms=ms, gbs=n_in * 4 * 12 / ms / 1e6)
    ms, vol = timed(lambda: _cubic(lib, coef, m, out_shape, st), a.reps)
    res["resample_cubic"] = dict(ms=ms, gbs=(n_in + n_out) * 4 / ms / 1e6)
    ms, max98 = timed(lambda: rs.percentile(vol, 98), a.reps)
    res["percentile"] = dict(ms=ms, gbs=n_out * 4 * 4 / ms / 1e6, value=float(max98))
    k = int(np.floor((n_out - 1) * np.float32(0.98))) + 1
    ms, kv = timed(lambda: torch.kthvalue(vol.view(-1), k).values.item(), a.reps)
    stock["percentile_kthvalue"] = dict(ms=ms)
    norm = torch.clamp(vol, 0.0, float(max98)) / float(max98)
    args = argparse.Namespace(dimension="3d", classes=CLASSES, training_size=WINDOW, window_size=WINDOW, sliding_window=True,
                              target_spacing=TARGET)
    padded, idx = P.pad_to_training_size(norm, args)
    cbim_amd.set_compute_dtype("bf16")
    nets = []
    for seed in range(MODELS):
        torch.manual_seed(seed)
        nets.append(UNet(1, 32, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=CLASSES, block="BasicBlock", norm="in").to(dev))
    x = padded[None, None].contiguous()
    accs, net_ms = [], []
    for net in nets:
        ms, (acc, counter, _) = timed(lambda: inference3d._sliding_window_accumulate(net, x, args), 2)
        net_ms.append(ms)
        accs.append((acc[0], counter[0, 0]))
    res["sliding_window_per_model"] = dict(ms=net_ms)
    S = accs[0][1].numel()
    total = torch.empty_like(accs[0][0])
    labels = torch.empty(accs[0][1].shape, dtype=torch.uint8, device=dev)

    def tail():
        for i, (acc, counter) in enumerate(accs):
            P.ensemble_finalize(acc, counter, total, labels, i == 0, i == MODELS - 1)
    ms, _ = timed(tail, a.reps)
    res["ensemble_tail"] = dict(ms=ms, gbs=(CLASSES * S * 4 * (3 * MODELS - 1) + S * 4 * MODELS + S) / ms / 1e6)

    def tail_stock():
        t = torch.zeros_like(total)
        for acc, counter in accs:
            t += acc / counter
        return torch.max(t, dim=0)[1]
    ms, lab_stock = timed(tail_stock, a.reps)
    stock["ensemble_tail_three_pass"] = dict(ms=ms)
    assert torch.equal(lab_stock.to(torch.uint8), labels)
    un = P.unpad_img(labels, idx, args).contiguous()
    geom, ref = (TARGET, (0, 0, 0), rs.IDENTITY), (SPACING, (0, 0, 0), rs.IDENTITY)
    ms, back = timed(lambda: rs.resample_label_to_ref(un, geom, ref, SHAPE), a.reps)
    res["label_resample"] = dict(ms=ms, gbs=(un.numel() + n_in) / ms / 1e6)
    try:
        ms, back_stock = timed(lambda: F.interpolate(un[None, None], size=SHAPE, mode="nearest")[0, 0], a.reps)
        stock["label_resample_interpolate_nearest"] = dict(ms=ms, dtype="uint8")
    except RuntimeError:                     # no uint8 kernel in this torch build: through float32 and back, as a caller would
        ms, back_stock = timed(lambda: F.interpolate(un[None, None].float(), size=SHAPE, mode="nearest")[0, 0].to(torch.uint8), a.reps)
        stock["label_resample_interpolate_nearest"] = dict(ms=ms, dtype="float32 round trip")
    cbim_amd.set_compute_dtype(None)
    new = sum(res[k]["ms"] for k in ("prefilter", "resample_cubic", "percentile", "ensemble_tail", "label_resample"))
    whole = new + sum(net_ms)
    out = {"bench": "prediction", "device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "resampled": list(out_shape),
           "classes": CLASSES, "models": MODELS, "stages": res, "stock": stock, "whole_ms": whole, "non_network_share": new / whole}
    if a.scipy:
        from scipy import ndimage
        t0 = time.perf_counter()
        ndimage.map_coordinates(raw, rs.map_coordinates_zyx(m, out_shape), order=3, mode="mirror", output=np.float32)
        out["scipy_cubic_resample_cpu_s"] = time.perf_counter() - t0
    print(json.dumps(out))


def _cubic(lib, coef, m, out_shape, st):
    dst = torch.empty(out_shape, dtype=torch.float32, device=coef.device)
    im = _lib.IndexMap()
    im.m[:] = [float(v) for v in m.reshape(12)]
    _lib.check(lib.cbim_resample3d(rs.CUBIC, _p(coef), _p(dst), 4, 1, *coef.shape, *out_shape, im, 0, st))
    return dst


if __name__ == "__main__":
    main()
