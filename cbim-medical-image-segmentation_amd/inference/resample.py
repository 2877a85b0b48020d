"""Resampling between voxel grids and exact percentiles on the device (csrc/predict_kernels.hip) — the SimpleITK / numpy steps
of the reference's prediction.py (ResampleXYZAxis / ResampleLabelToRef of dataset_conversion/utils.py:7-33, np.percentile of
prediction.py:169).

AXIS ORDER, stated once: a geometry is SimpleITK's ``(spacing, origin, direction)`` with spacing and origin as (x, y, z) and the
direction as 9 values, row-major, in x, y, z; arrays and tensors are indexed [z, y, x], so array axis a belongs to geometry
axis 2 - a.  Everything that crosses between the two (``index_map``, the size rule of ``resample_xyz_axis``) reverses once, here.

The geometry rules are ITK's documented ones (index -> physical point -> continuous index in float64, inside test
-0.5 <= c < n - 0.5, nearest = floor(c + 0.5), B-spline coefficients with mirror boundaries); SimpleITK itself is not needed.
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..ops import _dev_ok, _p, _stream

NEAREST, LINEAR, CUBIC = 0, 1, 3
_MODES = {"nearest": NEAREST, "linear": LINEAR, "bspline": CUBIC}
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _device(t):
    if _lib.backend() == "emu":
        return torch.device("cpu")
    return t.device if torch.is_tensor(t) and t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _geom(g):
    spacing, origin, direction = g
    return (np.asarray(spacing, np.float64), np.asarray(origin, np.float64), np.asarray(direction, np.float64).reshape(3, 3))


def index_map(src_geom, dst_geom):
    """The float64 [3, 4] map from an index (k, j, i) of the destination grid to the continuous index (z, y, x) of the source
    grid: physical point P = O_dst + Dir_dst (S_dst * idx), source index = (Dir_src^-1 (P - O_src)) / S_src — composed into one
    affine map in x, y, z and then reversed into array order."""
    ss, so, sd = _geom(src_geom)
    ds, do, dd = _geom(dst_geom)
    inv = np.linalg.inv(sd) / ss[:, None]                  # diag(1 / S_src) Dir_src^-1
    a = inv @ (dd * ds[None, :])
    b = inv @ (do - so)
    m = np.empty((3, 4), np.float64)
    m[:, :3] = a[::-1, ::-1]
    m[:, 3] = b[::-1]
    return m


def map_coordinates_zyx(m, shape):
    """The continuous source index of every voxel of a destination grid of `shape`, [3, *shape] float64, in the kernel's own
    order of operations ((m0 k + m1 j) + m2 i) + m3 — what a host-side check of the kernel has to evaluate."""
    k, j, i = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.stack([((m[a, 0] * k + m[a, 1] * j) + m[a, 2] * i) + m[a, 3] for a in range(3)])


def resample3d(src, m, out_shape, mode, default_value=0):
    """src [D, H, W] or [C, D, H, W] -> out_shape (z, y, x) through the index map m; mode 'nearest' (uint8 / int8 / bool / int32 /
    float32, copied), 'linear' or 'bspline' (float32; 'bspline' runs the prefilter first)."""
    mode = _MODES[mode] if isinstance(mode, str) else mode
    src = torch.as_tensor(src)
    squeeze = src.dim() == 3
    if squeeze:
        src = src[None]
    if src.dim() != 4:
        raise NotImplementedError("cbim_amd: resampling is 3-D only ([D, H, W] or [C, D, H, W])")
    if mode != NEAREST:
        src = src.float()
    elif src.element_size() not in (1, 4):
        raise TypeError(f"cbim_amd: nearest resampling copies 1-byte or 4-byte elements, not {src.dtype}")
    src = src.to(_device(src)).contiguous()
    _dev_ok(src)
    Cn, Di, Hi, Wi = map(int, src.shape)
    Do, Ho, Wo = map(int, out_shape)
    lib, st = _lib.lib(), _stream(src)
    if mode == CUBIC:
        coef = torch.empty_like(src)
        _lib.check(lib.cbim_bspline3_prefilter(_p(src), _p(coef), Cn, Di, Hi, Wi, st), "bspline3_prefilter")
        src = coef
    dst = torch.empty((Cn, Do, Ho, Wo), dtype=src.dtype, device=src.device)
    bits = int(np.asarray(default_value).astype(_np_dtype(src.dtype)).reshape(1).view(np.uint8 if src.element_size() == 1 else np.uint32)[0])
    im = _lib.IndexMap()
    im.m[:] = [float(v) for v in np.asarray(m, np.float64).reshape(12)]
    _lib.check(lib.cbim_resample3d(mode, _p(src), _p(dst), src.element_size(), Cn, Di, Hi, Wi, Do, Ho, Wo, im, bits, st),
               "resample3d")
    return dst[0] if squeeze else dst


def _np_dtype(dt):
    return {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8, torch.int8: np.int8, torch.bool: np.bool_}[dt]


def resampled_size(shape_zyx, spacing, target_spacing):
    """ResampleXYZAxis' size rule, int(round(n * sp / target)) per axis (dataset_conversion/utils.py:12), in array order."""
    n = tuple(int(v) for v in shape_zyx)[::-1]
    return tuple(int(round(n[a] * spacing[a] * 1.0 / target_spacing[a])) for a in range(3))[::-1]


def resample_xyz_axis(img, spacing, target_spacing, interp="bspline"):
    """ResampleXYZAxis (dataset_conversion/utils.py:7-21): img [D, H, W] (or [C, D, H, W]) with `spacing` (x, y, z) onto the grid
    of `target_spacing` with the same origin and direction; voxels whose source index falls outside the buffer are 0."""
    img = torch.as_tensor(img)
    out_shape = resampled_size(img.shape[-3:], spacing, target_spacing)
    zero = (0.0, 0.0, 0.0)
    m = index_map((tuple(spacing), zero, IDENTITY), (tuple(target_spacing), zero, IDENTITY))
    return resample3d(img, m, out_shape, interp)


def resample_label_to_ref(label, label_geom, ref_geom, ref_shape):
    """ResampleLabelToRef (dataset_conversion/utils.py:23-33): the label map on the reference image's grid (ref_shape in z, y, x),
    nearest neighbour, 0 outside."""
    return resample3d(label, index_map(label_geom, ref_geom), ref_shape, "nearest")


def _buffer_box(t):
    """(Db, Hb, Wb) of the contiguous [.., Db, Hb, Wb] buffer that t [.., D, H, W] is a leading corner of (t itself when
    contiguous; a view such as ``total[:, :D, :H, :W]``), or None when its strides are not those of such a corner."""
    *lead, D, H, W = (int(v) for v in t.shape)
    if t.is_contiguous():
        return (D, H, W)
    st = [int(v) for v in t.stride()]
    sz, sy, sx = st[-3:]
    if sx != 1 or sy < W or sz < sy * H or sz % sy:
        return None
    box = (D, sz // sy, sy)
    if lead:
        if len(lead) != 1 or (lead[0] > 1 and (st[0] < sz * D or st[0] % sz)):
            return None
        if lead[0] > 1:
            box = (st[0] // sz, sz // sy, sy)
    return box


def resample_argmax(prob, m, out_shape, counter=None, crop=None):
    """The label map of class probabilities on another grid: prob float32 [K, D, H, W] (K <= 256) interpolated trilinearly onto
    out_shape (z, y, x) through the index map m, first maximum over the classes, 0 outside — argmax(resample3d(prob, m,
    out_shape, 'linear'), 0) in one kernel that never writes the K resampled volumes.  counter float32 [D, H, W]: the window
    count the sliding-window sums are still to be divided by (each tap is prob / counter, the labels are those of the
    materialised quotient).  crop (z0, z1, y0, y1, x0, x1): the box of the buffer that is the image — m maps into the box,
    the edge clamps stay inside it: the result of ``prob[:, z0:z1, y0:y1, x0:x1]`` without the copy.  A prob that is itself a
    leading corner of a larger contiguous buffer (``total[:, :D, :H, :W]``) is read in place.  Returns uint8 [*out_shape]."""
    prob = torch.as_tensor(prob)
    if prob.dim() != 4:
        raise NotImplementedError("cbim_amd: resample_argmax takes class probabilities [K, D, H, W]")
    if prob.dtype != torch.float32 or (counter is not None and torch.as_tensor(counter).dtype != torch.float32):
        raise TypeError("cbim_amd: resample_argmax takes float32 probabilities and counts")
    dev = _device(prob)
    prob = prob.to(dev)
    K, D, H, W = map(int, prob.shape)
    if counter is not None:
        counter = torch.as_tensor(counter).to(dev)
        if tuple(counter.shape) != (D, H, W):
            raise ValueError(f"cbim_amd: counter {tuple(counter.shape)} does not match the probabilities {tuple(prob.shape)}")
    box = _buffer_box(prob)
    if box is None or (counter is not None and (_buffer_box(counter) or (0, 0, 0))[1:] != box[1:]):
        prob, box = prob.contiguous(), (D, H, W)
        counter = None if counter is None else counter.contiguous()
    crop = (0, D, 0, H, 0, W) if crop is None else tuple(int(v) for v in crop)
    if len(crop) != 6:
        raise ValueError("cbim_amd: crop is (z0, z1, y0, y1, x0, x1)")
    if box != (D, H, W) and any(hi > n for hi, n in zip(crop[1::2], (D, H, W))):
        raise ValueError(f"cbim_amd: crop {crop} leaves the view {(D, H, W)}")
    Do, Ho, Wo = map(int, out_shape)
    labels = torch.empty((Do, Ho, Wo), dtype=torch.uint8, device=dev)
    _dev_ok(labels)                                           # prob and counter sit on the same device, possibly as corner views
    im = _lib.IndexMap()
    im.m[:] = [float(v) for v in np.asarray(m, np.float64).reshape(12)]
    _lib.check(_lib.lib().cbim_resample_argmax(_p(prob), _p(counter), K, box[0], box[1], box[2], (C.c_int * 6)(*crop), _p(labels),
                                               Do, Ho, Wo, im, _stream(prob)), "resample_argmax")
    return labels


def resample_probabilities_to_ref(prob, geom, ref_geom, ref_shape, counter=None, crop=None):
    """The probability twin of resample_label_to_ref: class probabilities [K, D, H, W] on the grid `geom` (that of the crop box
    when crop is given) -> the uint8 label map on the reference image's grid, by trilinear interpolation of every class and
    the first maximum there (the nnU-Net rule); 0 outside.  Same index map as the label path."""
    return resample_argmax(prob, index_map(geom, ref_geom), ref_shape, counter=counter, crop=crop)


def order_stats(t, ranks):
    """The values at the given 0-based ranks (at most 4) of the ascending order of the float32 tensor t, as a numpy float32
    array: one readback of len(ranks) floats.  t must not hold NaN."""
    t = torch.as_tensor(t)
    if t.dtype != torch.float32:
        raise TypeError(f"cbim_amd: order statistics are taken of float32 data, not {t.dtype}")
    t = t.to(_device(t)).contiguous().view(-1)
    _dev_ok(t)
    n = t.numel()
    ranks = [int(r) % n for r in ranks]
    lib, st = _lib.lib(), _stream(t)
    nb = int(lib.cbim_order_stats_workspace())
    ws = torch.empty(nb, dtype=torch.uint8, device=t.device)
    out = torch.empty(len(ranks), dtype=torch.float32, device=t.device)
    rk = (C.c_int64 * len(ranks))(*ranks)
    _lib.check(lib.cbim_order_stats_f32(_p(t), n, rk, len(ranks), _p(out), _p(ws), nb, st), "order_stats_f32")
    return out.cpu().numpy()


def percentile(t, q):
    """np.percentile(t, q) (method 'linear') of a float32 tensor for a scalar q, bit for bit: the two neighbouring order statistics
    come from the device, the interpolation between them is numpy's own float32 arithmetic replayed on the host."""
    n = int(torch.as_tensor(t).numel())
    qq = np.true_divide(q, np.float32(100))                 # numpy divides by a float32 100 for float32 data
    if not (0 <= qq <= 1):
        raise ValueError("Percentiles must be in the range [0, 100]")
    virtual = np.asanyarray((n - 1) * qq)
    prev = np.floor(virtual)
    if virtual >= n - 1:
        lo = hi = -1
    else:
        lo, hi = int(prev), int(prev) + 1
    gamma = np.asanyarray(virtual - prev, dtype=virtual.dtype)
    a, b = (np.float32(v) for v in order_stats(t, [lo, hi]))
    diff = np.subtract(b, a)
    res = np.add(a, diff * gamma)
    if gamma >= 0.5:
        res = np.subtract(b, diff * (1 - gamma))
    return res
