"""Timing of foreground-oversampled patch sampling on the device (cbim_class_index / cbim_pick_voxel / cbim_crop3d_at) on the GPU,
next to the composition it replaces and to the uniform sample:
    python tools/bench_sampling.py [--reps 40] [--warmup 5] [--parent-resident FILE] [--out profiles/sampling.json]
Volume: 160x320x320, float32 image + int8 labels with 16 classes in 16^3 blocks, class 15 being one 20^3 blob; crops of 128^3.
  index_build      class_index of the volume (two launches: the zeroing of the totals and the one read of the volume); HIP events
  pick_crop        pick_class_voxel + crop_around_device_coordinate_3d, BATCH pairs queued back to back between one pair of
                   events, per pair: the kernels without the host
  pick_crop_host   one such pair, host clock from the call to the end of a device synchronise: THE figure to hold against
  composition      what it replaces: torch.nonzero(lab == c), the r-th row copied to the host, crop_around_coordinate_3d(center);
                   host clock to the end of a synchronise (the copy to the host is a synchronisation of its own)
  getitem_*        one whole ResidentVolumeDataset.__getitem__ (training_size 128^3, affine_pad_size 32), host clock to the end of
                   a synchronise, under the same seeds for every variant: forced (oversample_foreground = 1.0), uniform (the key
                   absent) and, with --parent-resident (a copy of training/dataset/resident.py of the parent commit), that
                   commit's uniform sample in the same process.  A sample's cost depends on the branch its seed takes (affine
                   resample or plain crop) and on the intensity ops it draws, so the medians are given per branch.
The variants alternate inside every repetition (the whole samples in rotating order); figures are medians over --reps repetitions after --warmup, with min and max.
The picks are compared with numpy's before timing."""
import argparse
import importlib.util
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
from cbim_amd.training import augmentation as A  # noqa: E402
from cbim_amd.training.dataset.resident import ResidentVolumeDataset  # noqa: E402

DIMS, K, CROP, BLOB, BATCH = (160, 320, 320), 16, [128, 128, 128], 20, 20


def volume():
    g = torch.Generator().manual_seed(11)
    coarse = torch.randint(0, K - 1, tuple(d // 16 for d in DIMS), generator=g)
    lab = coarse.repeat_interleave(16, 0).repeat_interleave(16, 1).repeat_interleave(16, 2).to(torch.int8)
    lab[100:100 + BLOB, 40:40 + BLOB, 250:250 + BLOB] = K - 1
    img = torch.randn((1,) + DIMS, generator=g)
    return img.cuda(), lab.cuda()


def stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def event_ms(fn, n=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def load_parent(path):
    spec = importlib.util.spec_from_file_location("cbim_amd.training.dataset.parent_resident", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ResidentVolumeDataset


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-resident", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "sampling.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling: needs a GPU")
    img, lab = volume()
    img5, lab5 = img.unsqueeze(0), lab.view((1, 1) + DIMS)
    idx = A.class_index(lab, K)
    counts = idx.counts().tolist()
    assert counts[K - 1] == BLOB ** 3 and idx.ignored() == 0
    # the picks against numpy, before any timing
    lab_np = lab.cpu().numpy()
    rng = np.random.default_rng(3)
    where = {}
    for uc, ur in rng.random((64, 2)):
        z, y, x, c = (int(v) for v in A.pick_class_voxel(idx, uc, ur).cpu())
        elig = [k for k in range(1, K) if counts[k] > 0]
        cw = elig[min(int(np.int64(uc * float(len(elig)))), len(elig) - 1)]
        if cw not in where:
            where[cw] = np.flatnonzero(lab_np.reshape(-1) == cw)
        r = min(int(np.int64(ur * float(counts[cw]))), counts[cw] - 1)
        assert (z, y, x, c) == tuple(int(v) for v in np.unravel_index(where[cw][r], DIMS)) + (cw,)
    del where

    blob = [K - 1]
    draws = rng.random((a.reps + a.warmup, 2))

    def pick_crop(uc, ur):
        return A.crop_around_device_coordinate_3d(img5, lab5, CROP, A.pick_class_voxel(idx, uc, ur, blob))

    def composition(uc, ur):
        nz = torch.nonzero(lab == K - 1)
        r = min(int(ur * nz.shape[0]), nz.shape[0] - 1)
        return A.crop_around_coordinate_3d(img5, lab5, CROP, nz[r].tolist(), mode="center")

    a0, b0 = pick_crop(0.3, 0.6)
    a1, b1 = composition(0.3, 0.6)
    assert torch.equal(a0, a1) and torch.equal(b0, b1)
    ms = {n: [] for n in ("index_build", "pick_crop", "pick_crop_host", "composition")}
    for it, (uc, ur) in enumerate(draws):
        got = {"index_build": event_ms(lambda: A.class_index(lab, K)),
               "pick_crop": event_ms(lambda: pick_crop(uc, ur), BATCH),
               "pick_crop_host": host_ms(lambda: pick_crop(uc, ur)),
               "composition": host_ms(lambda: composition(uc, ur))}
        if it >= a.warmup:
            for n, v in got.items():
                ms[n].append(v)

    # whole samples
    def args(**extra):
        return argparse.Namespace(training_size=CROP, affine_pad_size=[32] * 3, scale=[0.3] * 3, rotate=[30] * 3,
                                  translate=[0] * 3, **extra)

    sets = {"forced": ResidentVolumeDataset([img], [lab], args(oversample_foreground=1.0, num_classes=K)),
            "uniform": ResidentVolumeDataset([img], [lab], args())}
    if a.parent_resident:
        sets["uniform_parent"] = load_parent(a.parent_resident)([img], [lab], args())
    gms = {f"getitem_{n}_{b}": [] for n in sets for b in ("affine", "plain")}
    for it in range(a.reps + a.warmup):
        order = list(sets.items())
        for n, ds in order[it % len(order):] + order[:it % len(order)]:      # no variant always runs after the same other one
            np.random.seed(100 + it); torch.manual_seed(100 + it)
            t = host_ms(lambda: ds[0])
            first = np.random.RandomState(100 + it).random_sample(2)
            affine = first[1 if n == "forced" else 0] < 0.5          # the forced dataset draws "forced?" first
            if it >= a.warmup:
                gms[f"getitem_{n}_{'affine' if affine else 'plain'}"].append(t)

    nbytes = lab.numel()
    res = {"bench": "sampling", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "volume": list(DIMS), "classes": K, "blob_voxels": BLOB ** 3, "crop": CROP, "chunk": int(_lib.lib().cbim_class_index_chunk()),
           "index_bytes": idx.table.numel() * 4 + idx.totals.numel() * 8,
           "timed": "medians; variants alternate inside each repetition; *_host and composition and getitem_*: host clock to the "
                    "end of a device synchronise; index_build and pick_crop: HIP events (pick_crop: %d pairs queued back to back, per pair)" % BATCH}
    for n, v in list(ms.items()) + list(gms.items()):
        if v:
            res[n] = stat(v)
    res["index_build_GBps_of_label_bytes"] = round(nbytes / (res["index_build"]["median_ms"] * 1e-3) / 1e9, 1)
    res["composition_over_pick_crop_host"] = round(res["composition"]["median_ms"] / res["pick_crop_host"]["median_ms"], 2)
    res["forced_sample_cheaper_than_the_composition"] = bool(res["pick_crop_host"]["median_ms"] < res["composition"]["median_ms"])
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
