"""Timing of volume prediction on the GPU, stage by stage.  One CT-like case: 160x320x320 at spacing 0.8/0.8/2.5 mm (x, y, z)
resampled to 1 mm isotropic (400x256x256), 16 classes, the headline ResUNet (base 32) with 128^3 windows in bf16, a 2-model
ensemble.  Prints one JSON line:
    python tools/bench_prediction.py [--reps 5] [--scipy]
Per stage the HIP-event time (warmed, median of --reps) and, for the new kernels, the achieved GB/s against their algorithmic
bytes (percentile: 4 passes over the volume; prefilter: 3 axes x 2 sweeps x read + write; resample: one read of the source + one
write; ensemble tail: prob_sum + total read, total written, labels written; label resample: read + write of 1-byte labels).
`non_network_share`: everything but the models' sliding windows, as a share of the whole.  `stock`: the same stage written with
stock torch on the same box in the same process (torch.quantile is limited to 16M elements, so kthvalue stands in for it).
--scipy adds the CPU time of scipy's cubic resample of the same volume, for scale.

    python tools/bench_prediction.py --tta [--reps 5] [--out profiles/tta.json] [--no-volume]
times the window tail of ONE 128^3, 16-class window under 8 mirror variants + Gaussian window weights, without the network:
(a) cbim_window_gather_mirror + cbim_softmax_accumulate_tta; (b) the same result composed from what the engine had before them:
slice + .contiguous(), 8 x torch.flip of the input, 8 x torch.flip of the logits, 8 x cbim_softmax_accumulate into a temporary, a
torch multiply-add by the weight volume.  Both in the same process, alternating, each sample a loop of --inner calls between two
device events; the results are compared first.  Algorithmic bytes of (a): V*(2 + K) + 2*K + 2 + 1 floats per window voxel.  Unless
--no-volume, also the sliding-window time of one model over the whole resampled volume with TTA off and on (information only).
The JSON line is also written to --out with the device name and the date."""
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
    ap.add_argument("--tta", action="store_true", help="only the mirror-TTA / Gaussian window tail stage")
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-volume", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tta.json"))
    a = ap.parse_args()
    if a.tta:
        return tta_stage(a)
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


def tta_stage(a):
    import datetime
    dev = torch.device("cuda")
    V, K, win, vol, origin = 8, CLASSES, tuple(WINDOW), (160, 256, 256), (16, 64, 96)
    codes = inference3d.mirror_variants((0, 1, 2))
    weights = inference3d.window_weights(win, "gaussian", 0.125, dev)
    w3 = (weights[0][:, None, None] * weights[1][None, :, None]) * weights[2][None, None, :]
    gen = torch.Generator(device="cuda").manual_seed(3)
    img = torch.randn((1, 1) + vol, device=dev, generator=gen)
    logits = torch.randn((V, K) + win, device=dev, generator=gen) * 3
    d0, h0, w0 = origin
    sl = (slice(None), slice(None), slice(d0, d0 + win[0]), slice(h0, h0 + win[1]), slice(w0, w0 + win[2]))
    dims = [[2 + ax for ax in range(3) if c >> ax & 1] for c in codes]
    tmp = torch.empty((1, K) + win, device=dev)

    def new(acc, wsum):
        x = inference3d._gather_mirror(img, codes, d0, h0, w0, win)
        inference3d._accumulate_tta(logits, codes, weights, acc, wsum, d0, h0, w0)
        return x

    def composed(acc, wsum):
        w = img[sl].contiguous()
        x = torch.cat([torch.flip(w, d) if d else w for d in dims])
        tmp.zero_()
        for v, d in enumerate(dims):
            lv = logits[v:v + 1]
            inference3d._accumulate(torch.flip(lv, d) if d else lv, tmp, None, 0, 0, 0)
        acc[sl] += w3 * tmp
        wsum[sl] += w3 * float(V)
        return x

    outs = []
    for fn in (new, composed):                       # same result first (reordered float32 sums: last bits only)
        acc, wsum = torch.zeros((1, K) + vol, device=dev), torch.zeros((1, 1) + vol, device=dev)
        x = fn(acc, wsum)
        outs.append((x, acc, wsum))
    assert torch.equal(outs[0][0], outs[1][0])
    d_acc = float((outs[0][1] - outs[1][1]).abs().max())
    d_ws = float(((outs[0][2] - outs[1][2]).abs() / outs[1][2].clamp_min(1e-30)).max())
    assert d_acc < 8 * 2.0 ** -20 and d_ws < 1e-6, (d_acc, d_ws)
    acc, wsum = outs[0][1], outs[0][2]
    ms = {"new": [], "composed": []}
    for it in range(a.reps + 1):                      # alternating; the first round is warm-up
        for name, fn in (("new", new), ("composed", composed)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.inner):
                fn(acc, wsum)
            e1.record()
            torch.cuda.synchronize()
            if it:
                ms[name].append(e0.elapsed_time(e1) / a.inner)
    t_new, t_old = statistics.median(ms["new"]), statistics.median(ms["composed"])
    nvox = win[0] * win[1] * win[2]
    floats = V * (2 + K) + 2 * K + 2 + 1
    out = {"bench": "tta_window_tail", "device": torch.cuda.get_device_name(0), "date": datetime.date.today().isoformat(),
           "window": list(win), "classes": K, "variants": V, "window_weight": "gaussian", "reps": a.reps, "inner": a.inner,
           "new_ms": t_new, "composed_ms": t_old, "ratio": t_old / t_new, "new_ms_all": ms["new"], "composed_ms_all": ms["composed"],
           "new_algorithmic_gbs": floats * 4 * nvox / t_new / 1e6, "max_abs_diff_acc": d_acc}
    del outs, acc, wsum, logits, tmp
    if not a.no_volume:
        out["volume"] = tta_volume()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def tta_volume():
    """information only: one model's sliding windows over the resampled 400x256x256 volume, bf16, TTA + Gaussian off and on"""
    from cbim_amd.model.dim3 import UNet
    dev = torch.device("cuda")
    shape = rs.resampled_size(SHAPE, SPACING, TARGET)
    x = torch.rand((1, 1) + tuple(shape), device=dev)
    torch.manual_seed(0)
    net = UNet(1, 32, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=CLASSES, block="BasicBlock", norm="in").to(dev)
    base = dict(dimension="3d", classes=CLASSES, window_size=WINDOW, sliding_window=True)
    on = dict(base, tta_mirror_axes=(0, 1, 2), window_weight="gaussian", tta_batch=1)
    cbim_amd.set_compute_dtype("bf16")
    try:
        res = {"shape": list(shape), "tta_batch": 1}
        for name, kw in (("off_ms", base), ("on_ms", on)):
            res[name], _ = timed(lambda: inference3d.inference_sliding_window(net, x, argparse.Namespace(**kw)), 1)
    finally:
        cbim_amd.set_compute_dtype(None)
    res["on_over_off"] = res["on_ms"] / res["off_ms"]
    return res


def _cubic(lib, coef, m, out_shape, st):
    dst = torch.empty(out_shape, dtype=torch.float32, device=coef.device)
    im = _lib.IndexMap()
    im.m[:] = [float(v) for v in m.reshape(12)]
    _lib.check(lib.cbim_resample3d(rs.CUBIC, _p(coef), _p(dst), 4, 1, *coef.shape, *out_shape, im, 0, st))
    return dst


if __name__ == "__main__":
    main()
