"""Predict one volume: a raw float32 scan as .npy plus its spacing in, a uint8 label map on the scan's own grid as .npy out.
    python examples/predict_volume.py --img scan.npy --spacing 0.8,0.8,2.5 --load a.pth,b.pth --out label.npy \\
        [--target_spacing 1,1,1] [--classes 16] [--base_chan 32] [--training_size 128,128,128] [--ema] [--fp32]
        [--keep-largest all|1,2,6] [--min-size 50]
The checkpoints are the reference trainer's (`model_state_dict` / `ema_model_state_dict`) of a ResUNet; several of them form an
ensemble.  NIfTI reading and writing stay with the caller (origin and direction only matter when they differ between grids)."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cbim_amd  # noqa: E402
from cbim_amd.prediction import init_model, predict_volume  # noqa: E402


def main():
    floats = lambda s: tuple(float(v) for v in s.split(","))      # noqa: E731
    ints = lambda s: [int(v) for v in s.split(",")]               # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", required=True)
    ap.add_argument("--spacing", type=floats, required=True, help="x,y,z in mm")
    ap.add_argument("--target_spacing", type=floats, default=(1.0, 1.0, 1.0), help="the training spacing, x,y,z")
    ap.add_argument("--load", type=lambda s: s.split(","), required=True, help="checkpoint paths, ',' separated")
    ap.add_argument("--out", required=True)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--base_chan", type=int, default=32)
    ap.add_argument("--training_size", type=ints, default=[128, 128, 128])
    ap.add_argument("--ema", action="store_true")
    ap.add_argument("--fp32", action="store_true")
    ap.add_argument("--keep-largest", default=None, help="'all' or class values, ',' separated: keep only their largest component")
    ap.add_argument("--min-size", type=int, default=0, help="drop connected components below this many voxels")
    args = ap.parse_args()
    args.dimension, args.model, args.in_chan, args.norm, args.block = "3d", "resunet", 1, "in", "BasicBlock"
    args.down_scale, args.kernel_size = [[2, 2, 2]] * 4, [[3, 3, 3]] * 5
    args.sliding_window, args.window_size = True, args.training_size           # prediction.py:269-270
    cbim_amd.set_compute_dtype("fp32" if args.fp32 else "bf16")
    models = init_model(args)
    img = torch.from_numpy(np.load(args.img).astype(np.float32))
    components = None
    if args.keep_largest or args.min_size:
        keep = () if not args.keep_largest else ("all" if args.keep_largest == "all" else ints(args.keep_largest))
        components = {"keep_largest": keep, "min_size": args.min_size}
    label = predict_volume(models, img, args.spacing, args, components=components)
    np.save(args.out, label.cpu().numpy())
    print(f"{args.img}: {tuple(img.shape)} at {args.spacing} mm -> {args.out} uint8, classes present {np.unique(label.cpu().numpy()).tolist()}")


if __name__ == "__main__":
    main()
