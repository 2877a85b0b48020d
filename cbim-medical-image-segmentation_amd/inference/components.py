"""Connected components of a label map on the device (csrc/components_kernels.hip) and the clean-up every organ pipeline applies to
a prediction before it is scored or written: keep the largest component of an organ, drop specks below N voxels.

Two voxels are connected iff they are neighbours under ``connectivity`` (6, 18 or 26) and carry the same non-zero value, so one
pass labels every class at once and touching organs of different class never merge.  For a binary input ``connected_components``
is ``scipy.ndimage.label(x, generate_binary_structure(3, k))`` element for element (k = 1, 2, 3), numbering included.  Every
result is a function of the input alone: the union-find behind it always links towards the smaller linear index, so the root of a
component is its first voxel in raster order whatever order the atomics land in.

    comp, n = connected_components(labels)                                   # int32 ids 1..n, one host sync (n)
    clean = filter_components(labels, keep_largest="all", min_size=50)       # uint8, no host sync, graph-capturable
"""
import functools

import numpy as np
import torch

from .. import _lib
from ..ops import _p, _stream

CONNECTIVITIES = (6, 18, 26)


def _engine_device_type():
    return "cpu" if _lib.backend() == "emu" else "cuda"


def _as_labels(labels):
    """The uint8 [D, H, W] contiguous tensor the kernels take.  uint8 and bool pass without a copy or a sync; int64 is range-checked
    (one host sync) and narrowed."""
    if not torch.is_tensor(labels):
        raise ValueError("components: labels must be a torch tensor on the engine's device")
    if labels.dim() != 3:
        raise ValueError(f"components: labels must be [D, H, W], not {tuple(labels.shape)}")
    if labels.device.type != _engine_device_type():
        raise ValueError(f"components: labels on '{labels.device.type}', the loaded kernel library ({_lib.backend()}) executes on "
                         f"'{_engine_device_type()}'")
    if labels.numel() == 0:
        raise ValueError("components: empty volume")
    if labels.dtype == torch.uint8:
        return labels.contiguous()
    if labels.dtype == torch.bool:
        return labels.contiguous().view(torch.uint8)
    if labels.dtype == torch.int64:
        lo, hi = (int(v) for v in torch.stack((labels.min(), labels.max())).tolist())
        if lo < 0 or hi > 255:
            raise ValueError(f"components: int64 labels must lie in 0..255, found {lo}..{hi}")
        return labels.to(torch.uint8).contiguous()
    raise ValueError(f"components: labels must be uint8, bool or int64, not {labels.dtype}")


def _check_connectivity(connectivity):
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"components: connectivity must be 6, 18 or 26, not {connectivity!r}")
    return int(connectivity)


def _label(lab, connectivity):
    """Stages 1-3: parent int32 [D, H, W], the linear index of each voxel's root (-1 for background)."""
    D, H, W = map(int, lab.shape)
    parent = torch.empty((D, H, W), dtype=torch.int32, device=lab.device)
    _lib.check(_lib.lib().cbim_components_label(_p(lab), D, H, W, connectivity, _p(parent), _stream(lab)), "components_label")
    return parent


def _sizes(lab, parent):
    """Stages 4-5: size int32 [D, H, W] (voxel count at every root, 0 elsewhere), best int64 [256] (the packed per-class winner)."""
    D, H, W = map(int, lab.shape)
    size = torch.empty((D, H, W), dtype=torch.int32, device=lab.device)
    best = torch.empty(256, dtype=torch.int64, device=lab.device)
    _lib.check(_lib.lib().cbim_components_sizes(_p(lab), _p(parent), D, H, W, _p(size), _p(best), _stream(lab)), "components_sizes")
    return size, best


def _number(parent):
    D, H, W = map(int, parent.shape)
    nbytes = int(_lib.lib().cbim_components_workspace_bytes(D, H, W))
    if nbytes < 0:
        _lib.check(nbytes, "components_workspace_bytes")
    comp = torch.empty((D, H, W), dtype=torch.int32, device=parent.device)
    n = torch.empty(1, dtype=torch.int32, device=parent.device)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=parent.device)
    _lib.check(_lib.lib().cbim_components_number(_p(parent), D, H, W, _p(comp), _p(n), _p(scratch), _stream(parent)),
               "components_number")
    return comp, n


def connected_components(labels, connectivity=26):
    """labels: uint8, bool or int64 (values 0..255) [D, H, W] on the engine's device.  Returns (comp int32 [D, H, W], n): ids 1..n
    in raster order of each component's first voxel, 0 for background.  One host synchronisation (n)."""
    connectivity = _check_connectivity(connectivity)
    lab = _as_labels(labels)
    comp, n = _number(_label(lab, connectivity))
    return comp, int(n.item())


def component_sizes(labels, connectivity=26):
    """int64 [n + 1] on the device: entry 0 is the background count, entry k the voxels of component k of
    ``connected_components``."""
    connectivity = _check_connectivity(connectivity)
    lab = _as_labels(labels)
    parent = _label(lab, connectivity)
    size, _ = _sizes(lab, parent)
    index = torch.arange(parent.numel(), dtype=torch.int32, device=parent.device)
    fg = size.reshape(-1)[parent.reshape(-1) == index].to(torch.int64)          # the roots, in raster order
    return torch.cat(((parent.numel() - fg.sum()).reshape(1), fg))


def _table_key(keep_largest, min_size):
    if isinstance(keep_largest, str):
        if keep_largest != "all":
            raise ValueError(f"components: keep_largest must be an iterable of class values or 'all', not {keep_largest!r}")
        kl = tuple(range(1, 256))
    else:
        kl = tuple(sorted({int(c) for c in keep_largest}))
    if isinstance(min_size, dict):
        ms = tuple(sorted((int(c), int(v)) for c, v in min_size.items()))
    else:
        ms = int(min_size)
    for c in kl + (tuple(c for c, _ in ms) if isinstance(ms, tuple) else ()):
        if not 1 <= c <= 255:
            raise ValueError(f"components: class value {c} outside 1..255")
    return kl, ms


@functools.lru_cache(maxsize=64)
def _tables(kl, ms, device):
    keep = np.zeros(256, np.uint8)
    keep[list(kl)] = 1
    if isinstance(ms, tuple):
        mins = np.zeros(256, np.int32)
        for c, v in ms:
            mins[c] = v
    else:
        mins = np.full(256, ms, np.int32)
    mins = np.clip(mins, 0, None)
    return torch.from_numpy(keep).to(device), torch.from_numpy(mins).to(device)


def filter_tables(keep_largest=(), min_size=0, device=None):
    """The two 256-entry device tables of the filter kernel: (keep_largest uint8, min_size int32).  They are cached per
    (arguments, device), so only the first call with given arguments uploads anything."""
    kl, ms = _table_key(keep_largest, min_size)
    device = torch.device(_engine_device_type() if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return _tables(kl, ms, device)


def filter_components(labels, keep_largest=(), min_size=0, connectivity=26, out=None):
    """The label map with the unwanted components set to 0 (uint8 [D, H, W]).

    keep_largest: iterable of class values, or "all" for 1..255: of such a class only the largest component survives (of two equally
                  large ones, the one whose first voxel comes first in raster order).
    min_size:     int for every foreground class, or {class: int}: components below it vanish; one of exactly min_size voxels stays.
                  A class under both rules whose largest component is below min_size vanishes entirely.
    out:          uint8 tensor of the same shape to write into; may be ``labels`` itself.

    Classes under neither rule pass through untouched.  No host synchronisation (for uint8 / bool input) and no allocation sized by
    the number of components: the whole path can be captured in a graph, once the tables of these arguments have been uploaded
    by a first eager call or by ``filter_tables``."""
    connectivity = _check_connectivity(connectivity)
    lab = _as_labels(labels)
    keep, mins = filter_tables(keep_largest, min_size, lab.device)
    if out is None:
        out = torch.empty_like(lab)
    elif not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.shape == lab.shape and out.device == lab.device
              and out.is_contiguous()):
        raise ValueError("components: out must be a contiguous uint8 tensor of the labels' shape on their device")
    parent = _label(lab, connectivity)
    size, best = _sizes(lab, parent)
    _lib.check(_lib.lib().cbim_components_filter(_p(lab), _p(parent), _p(size), _p(best), _p(keep), _p(mins), _p(out),
                                                 lab.numel(), _stream(lab)), "components_filter")
    return out
