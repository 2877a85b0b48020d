"""Per-class surface points of two label volumes and their distances to the other surface, on the device
(csrc/surface_kernels.hip) — the raw material of the reference's ASD / HD95 (metric/metrics.py compute_surface_distances).

Two host synchronisations per volume whatever the number of classes: the per-class boxes and surface-point counts
(``cbim_surface_scan``), then the compacted lists (``cbim_surface_lists``).  The kernels know nothing about surfel areas: they
emit ``(distance, neighbour code)`` per surface point and the caller looks the areas up (``metric.utils.calculate_distance``).
"""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ..ops import _dev_ok, _p, _stream

KEYS = ("distances_gt_to_pred", "codes_gt", "distances_pred_to_gt", "codes_pred")


def _labels(t, device):
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.dtype not in (torch.int8, torch.int64):
        t = t.long()
    return t.to(device).contiguous()


def spacing_array(spacing):
    """The spacing as the numpy array the reference's ``spacing.numpy()`` yields: a tensor keeps its dtype, any other sequence is
    taken as the float32 values the reference's datasets deliver."""
    if torch.is_tensor(spacing):
        return spacing.detach().cpu().numpy()
    return np.asarray(spacing, dtype=np.float32)


def _empty():
    return {k: np.zeros(0, np.uint8 if k.startswith("codes") else np.float64) for k in KEYS}


def surface_distances(label_pred, label_true, spacing, C_):
    """label_pred, label_true: [D, H, W] label tensors (int8 or int64, device or host); spacing: 3 values.
    Returns a list of C_ - 1 dicts (classes 1 .. C_-1) with the UNSORTED arrays ``distances_gt_to_pred`` (float64),
    ``codes_gt`` (uint8), ``distances_pred_to_gt``, ``codes_pred``; a class absent from both volumes gives four empty arrays,
    a class absent from one gives ``inf`` distances on the other side."""
    label_pred, label_true = torch.as_tensor(label_pred), torch.as_tensor(label_true)
    if label_pred.dim() != 3 or label_true.dim() != 3 or len(spacing_array(spacing)) != 3:
        raise NotImplementedError("cbim_amd: surface metrics are 3-D only (2-D masks are outside the model/dim3 hot path)")
    if tuple(label_pred.shape) != tuple(label_true.shape):
        raise ValueError(f"label_pred {tuple(label_pred.shape)} and label_true {tuple(label_true.shape)} differ in shape")
    device = torch.device("cpu") if _lib.backend() == "emu" else \
        (label_pred.device if label_pred.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    pred, gt = _labels(label_pred, device), _labels(label_true, device)
    _dev_ok(pred, gt)
    D, H, W = map(int, pred.shape)
    s = [float(v) for v in spacing_array(spacing).astype(np.float64)]
    lib, st = _lib.lib(), _stream(pred)

    box = torch.empty((C_, 8), dtype=torch.int32, device=device)
    _lib.check(lib.cbim_surface_scan(_p(pred), pred.element_size(), _p(gt), gt.element_size(), D, H, W, C_, _p(box), st),
               "surface_scan")
    box = box.cpu().numpy()                                           # synchronisation 1: boxes + counts

    out = [_empty() for _ in range(C_ - 1)]
    present = [c for c in range(1, C_) if box[c, 6] + box[c, 7] > 0]
    if not present:
        return out
    descs = (_lib.SurfaceDesc * len(present))()
    vtot = entries = 0
    for d, c in zip(descs, present):
        lo, hi = box[c, 0:3], box[c, 3:6]
        d.cls, (d.z0, d.y0, d.x0), (d.nz, d.ny, d.nx) = c, map(int, lo), map(int, hi - lo + 1)
        d.off = vtot
        vtot += d.nz * d.ny * d.nx
        for m in range(2):
            d.list_off[m], d.list_cap[m] = entries, int(box[c, 6 + m])
            entries += int(box[c, 6 + m])
    desc_bytes = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
    desc_dev = desc_bytes.to(device)
    codes = torch.empty(2 * vtot, dtype=torch.uint8, device=device)
    dx = torch.empty(2 * vtot, dtype=torch.int16, device=device)
    dyx = torch.empty(2 * vtot, dtype=torch.int32, device=device)
    # one buffer, one readback: [entries] float64 distances | [n][2] int32 list lengths | [entries] uint8 codes
    n = len(present)
    o_cur, o_code = 8 * entries, 8 * entries + 8 * n
    buf = torch.empty(o_code + entries, dtype=torch.uint8, device=device)
    base = buf.data_ptr()
    _lib.check(lib.cbim_surface_lists(_p(pred), pred.element_size(), _p(gt), gt.element_size(), D, H, W,
                                      C.cast(descs, C.c_void_p), _p(desc_dev), n, vtot, s[0], s[1], s[2],
                                      _p(codes), _p(dx), _p(dyx), C.c_void_p(base), C.c_void_p(base + o_code), entries,
                                      C.c_void_p(base + o_cur), st), "surface_lists")
    host = buf.cpu().numpy()                                          # synchronisation 2: the lists
    dist = host[:o_cur].view(np.float64)
    cursor = host[o_cur:o_code].view(np.int32).reshape(n, 2)
    code = host[o_code:]
    for k, (d, c) in enumerate(zip(descs, present)):
        for m, (kd, kc) in enumerate((KEYS[0:2], KEYS[2:4])):
            if int(cursor[k, m]) != d.list_cap[m]:
                raise RuntimeError(f"cbim_amd: surface list of class {c} holds {int(cursor[k, m])} points, the scan counted "
                                   f"{d.list_cap[m]}")
            a, b = d.list_off[m], d.list_off[m] + d.list_cap[m]
            out[c - 1][kd], out[c - 1][kc] = dist[a:b].copy(), code[a:b].copy()
    return out
