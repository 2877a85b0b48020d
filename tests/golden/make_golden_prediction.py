"""Golden fixtures for volume prediction.   python tests/golden/make_golden_prediction.py

Part 1 — EXECUTES THE REAL REFERENCE (prediction.py: pad_to_training_size, the percentile lines of preprocess, prediction,
unpad_img) on the CPU.  The reference's text is run unmodified; to import it here SimpleITK and skimage.measure are stub modules
(nothing of them is called), training.dataset.utils is the shim tests/ref_trainer_seam.py uses, and torch.Tensor.cuda is the
identity in this process.  Two seeded ResUNets (base 8, 3 classes; weights reproducible through oracle.unet_ref) form the
ensemble; the raw volume is 20x48x40 with integer intensities (stored as int16), training_size 32^3.
  prediction_ensemble.npz          raw volume, max98, original_idx, padded shape, the reference's label map, weight checksums
  prediction_ensemble_p<k>.npz     the reference's summed probabilities of class k, float32 (one file per class: 255 KB each)

Part 2 — the resampling yardstick.  SimpleITK is not installed where this project is developed, so the two resamplers cannot be
pinned to ITK's output; the geometry rules are ITK's documented ones and the numbers come from scipy.ndimage in float64
(spline_filter / map_coordinates order=3 mode='mirror'; order=1 mode='nearest'; order=0), with ITK's inside rule
-0.5 <= c < n - 0.5 applied on top.  The source coordinates are computed here in ITK's two steps (index -> physical point ->
continuous index), independently of the engine's composed index map.
  prediction_resample.npz          small anisotropic volumes, geometries, float64 results
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402

SEEDS, INPUT_SEED, SHAPE, TRAIN, CLASSES, BASE = (5051, 5052), 7, (20, 48, 40), [32, 32, 32], 3, 8
MARGIN = 2e-5            # 1e-5 per model (tests/infer_checks.py:56)


def raw_volume():
    """A CT-like raw scan: integer intensities, a negative background, a bright tail above the 98th percentile."""
    rng = np.random.default_rng(INPUT_SEED)
    v = rng.standard_normal(SHAPE) * 180.0 + 120.0
    v[rng.random(SHAPE) < 0.03] += 900.0
    return np.round(v).astype(np.int16)


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def import_reference_prediction():
    UNet, _ = mg.import_reference()
    for name in ("SimpleITK", "skimage", "skimage.measure"):
        sys.modules.setdefault(name, _Stub(name))
    ds = types.ModuleType("training.dataset.utils")
    ds.get_dataset = lambda args, mode, **kw: None
    import training  # noqa: F401  (the reference's package)
    dpk = types.ModuleType("training.dataset")
    dpk.__path__ = []
    sys.modules["training.dataset"] = dpk
    sys.modules["training.dataset.utils"] = ds
    import matplotlib
    matplotlib.use("Agg")
    torch.Tensor.cuda = lambda self, *a, **k: self
    return UNet, importlib.import_module("prediction")


def ensemble_fixture():
    from oracle.unet_ref import state_dict_checksum
    UNet, ref = import_reference_prediction()
    torch.set_num_threads(8)
    args = argparse.Namespace(dimension="3d", classes=CLASSES, training_size=TRAIN, window_size=TRAIN, sliding_window=True)
    nets = []
    for seed in SEEDS:
        torch.manual_seed(seed)
        nets.append(UNet(1, BASE, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=CLASSES, block="BasicBlock", norm="in"))
    raw = raw_volume()
    np_img = raw.astype(np.float32)
    max98 = np.percentile(np_img, 98)                                       # prediction.py:169-171, the same three expressions
    np_img = np.clip(np_img, 0, max98)
    np_img = np_img / max98
    assert np_img.dtype == np.float32
    np_img, original_idx = ref.pad_to_training_size(np_img, args)
    tensor_img = torch.from_numpy(np_img)
    label = ref.prediction(nets, tensor_img, args)
    # the summed probabilities are a local of prediction(); re-run its loop body (prediction.py:42-57) with the reference's own inference
    inference = ref.get_inference(args)
    with torch.no_grad():
        total = torch.zeros([CLASSES] + list(tensor_img.shape))
        for net in nets:
            total += inference(net, tensor_img.float().unsqueeze(0).unsqueeze(0), args).squeeze(0)
    assert torch.equal(total.max(0)[1], label)
    top2 = total.topk(2, dim=0).values
    low = float(((top2[0] - top2[1]) <= MARGIN).float().mean())
    assert low < 1e-3, low
    unpadded = ref.unpad_img(label.numpy().astype(np.uint8), original_idx, args)
    assert unpadded.shape == SHAPE
    meta = dict(raw=raw, max98=np.float32(max98), original_idx=np.asarray(original_idx, np.int64),
                padded_shape=np.asarray(np_img.shape, np.int64), label=label.numpy().astype(np.uint8), label_unpadded=unpadded,
                low_margin_share=np.float64(low), seeds=np.asarray(SEEDS, np.int64),
                sd_checksum=np.asarray([state_dict_checksum(n.state_dict()) for n in nets], np.float64))
    _save("prediction_ensemble", meta)
    for k in range(CLASSES):
        _save(f"prediction_ensemble_p{k}", dict(prob_sum=total[k].numpy()))
    print("ensemble: original_idx", original_idx, "padded", np_img.shape, "max98", max98, "share at or under the margin", low)


def _save(name, d):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **d)
    kb = os.path.getsize(path) / 1024
    print(f"  {name}.npz {kb:.0f} KB")
    assert kb < 300, (name, kb)


# ---- part 2 ------------------------------------------------------------------------------------------------------------------

def itk_coords(src_geom, dst_geom, shape_zyx):
    """Continuous source index (z, y, x) of every voxel of the destination grid, ITK's way: TransformIndexToPhysicalPoint of the
    destination, TransformPhysicalPointToContinuousIndex of the source, float64.  Geometries in x, y, z."""
    (ss, so, sd), (ds, do, dd) = [(np.asarray(s, np.float64), np.asarray(o, np.float64), np.asarray(d, np.float64).reshape(3, 3))
                                  for s, o, d in (src_geom, dst_geom)]
    k, j, i = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape_zyx], indexing="ij")
    idx = np.stack([i, j, k]).reshape(3, -1)                                 # x, y, z
    phys = do[:, None] + dd @ (idx * ds[:, None])
    cont = (np.linalg.inv(sd) @ (phys - so[:, None])) / ss[:, None]
    return cont[::-1].reshape((3,) + tuple(shape_zyx))


def yardstick(vol, co, order):
    from scipy import ndimage
    inside = np.ones(co.shape[1:], bool)
    for a in range(3):
        frac = (co[a] + 0.5) - np.floor(co[a] + 0.5)
        assert float(np.minimum(frac, 1 - frac).min()) > 1e-6, f"axis {a}: a source index sits on a rounding tie / the buffer edge"
        inside &= (co[a] >= -0.5) & (co[a] < vol.shape[a] - 0.5)
    if order == 0:
        out = ndimage.map_coordinates(vol, np.floor(co + 0.5), order=0, mode="nearest")
        return np.where(inside, out, np.zeros((), vol.dtype)), inside
    mode = "mirror" if order == 3 else "nearest"
    out = ndimage.map_coordinates(vol.astype(np.float64), co, order=order, mode=mode)
    return np.where(inside, out, 0.0), inside


IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def resample_cases():
    """name -> (volume shape zyx, spacing xyz, target spacing xyz, origin, direction)."""
    c, s = np.cos(0.31), np.sin(0.31)
    t, u = np.cos(0.17), np.sin(0.17)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    rx = np.array([[1.0, 0, 0], [0, t, -u], [0, u, t]])
    return {
        # z: 7 slices of 2.45 mm -> round(17.15) = 17 slices of 1 mm; the last sits at source index 6.53 >= 6.5: outside the buffer
        "up": ((7, 12, 15), (0.8, 0.9, 2.45), (0.71, 0.64, 1.0), (0.0, 0.0, 0.0), IDENT),
        "down": ((16, 14, 18), (0.8, 0.75, 1.0), (1.31, 1.73, 2.31), (-31.5, 12.25, 4.0), IDENT),
        "oblique": ((9, 13, 11), (0.9, 1.1, 2.2), (1.0, 1.0, 1.0), (5.0, -7.5, 11.0), tuple((rz @ rx).reshape(-1))),
    }


def resample_fixture():
    from cbim_amd.inference.resample import resampled_size
    rng = np.random.default_rng(4242)
    out = {}
    for name, (shape, sp, tsp, origin, direction) in resample_cases().items():
        zz, yy, xx = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
        vol = (np.sin(5 * zz + 3 * yy) * np.cos(4 * xx - yy) * 300 + rng.standard_normal(shape) * 40 + 100).astype(np.float32)
        lab_shape = resampled_size(shape, sp, tsp)
        src_geom, dst_geom = (sp, origin, direction), (tsp, origin, direction)
        if name == "oblique":          # a destination grid that is NOT the source's own: other direction and origin
            dst_geom = (tsp, (4.2, -6.9, 10.1), IDENT)
        co = itk_coords(src_geom, dst_geom, lab_shape)
        out[f"{name}_vol"] = vol
        out[f"{name}_geom_src"] = np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in src_geom])
        out[f"{name}_geom_dst"] = np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in dst_geom])
        out[f"{name}_shape_dst"] = np.asarray(lab_shape, np.int64)
        for tag, order in (("cubic", 3), ("linear", 1), ("nearest", 0)):
            res, inside = yardstick(vol, co, order)
            out[f"{name}_{tag}"] = res
        out[f"{name}_outside"] = np.int64((~inside).sum())
        # a label map on the destination grid, brought back onto the source grid (ResampleLabelToRef)
        lab = (rng.integers(0, 4, [(n + 2) // 3 for n in lab_shape]).repeat(3, 0).repeat(3, 1).repeat(3, 2)
               [:lab_shape[0], :lab_shape[1], :lab_shape[2]]).astype(np.uint8)
        back, inside_b = yardstick(lab, itk_coords(dst_geom, src_geom, shape), 0)
        out[f"{name}_label"] = lab
        out[f"{name}_label_back"] = back.astype(np.uint8)
        print(f"  {name}: {shape} -> {lab_shape}, outside {int((~inside).sum())}, back outside {int((~inside_b).sum())}")
    assert int(out["up_outside"]) > 0
    _save("prediction_resample", out)


if __name__ == "__main__":
    if "--resample-only" not in sys.argv:
        ensemble_fixture()
    resample_fixture()
