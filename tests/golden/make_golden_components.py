"""Writes tests/golden/components.npz: what scipy.ndimage.label gives on the volumes of tests/components_checks.py (the inputs are
formulas there and are not stored).
    python tests/golden/make_golden_components.py

  rand_<shape>_<density>_<conn>_n / _sha / _map   binary volumes: component count, SHA-256 of scipy's int32 map, and for the small
                                                  shape the map itself (uint16)
  multi_<conn>_n / _map                           the 0..5 map: scipy run per class, components renumbered over all classes by
                                                  their first voxel in raster order
  filter_<conn>_<case>                            expected filtered maps from label + bincount + argmax per class
"""
import os
import sys

import numpy as np
from scipy import ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests import components_checks as ck  # noqa: E402


def label(vol, rank):
    comp, n = ndi.label(vol, ndi.generate_binary_structure(3, rank))
    return comp.astype(np.int32), int(n)


def label_multi(vol, rank):
    """every class on its own, then ids in the order of the components' first voxels over all classes"""
    firsts, maps = [], []
    for c in np.unique(vol[vol > 0]):
        comp, n = label(vol == c, rank)
        first = ndi.minimum(np.arange(vol.size).reshape(vol.shape), comp, index=np.arange(1, n + 1)).astype(np.int64)
        firsts += [(int(f), len(maps), k + 1) for k, f in enumerate(np.atleast_1d(first))]
        maps.append(comp)
    out = np.zeros(vol.shape, np.int32)
    for new, (_, m, k) in enumerate(sorted(firsts)):
        out[maps[m] == k] = new + 1
    return out, len(firsts)


def filtered(vol, rank, keep_largest, min_size):
    kl = range(1, 256) if isinstance(keep_largest, str) else keep_largest
    out = vol.copy()
    for c in np.unique(vol[vol > 0]):
        comp, n = label(vol == c, rank)
        sizes = np.bincount(comp.ravel(), minlength=n + 1)
        sizes[0] = 0
        keep = np.ones(n + 1, bool)
        keep[0] = False
        if c in kl:
            keep[:] = False
            keep[np.argmax(sizes)] = True                      # the first of equal maxima: the smaller id, first in raster order
        ms = min_size.get(int(c), 0) if isinstance(min_size, dict) else min_size
        keep &= sizes >= ms
        out[(vol == c) & ~keep[comp]] = 0
    return out


def build():
    g = {}
    for si in range(len(ck.SHAPES)):
        for pi in range(len(ck.DENSITIES)):
            vol = ck.binary_volume(si, pi)
            for conn, rank in ck.CONN:
                comp, n = label(vol, rank)
                key = f"rand_{si}_{pi}_{conn}"
                g[key + "_n"], g[key + "_sha"] = np.int64(n), ck.sha(comp)
                if si < ck.STORED_MAPS:
                    assert n < 65536
                    g[key + "_map"] = comp.astype(np.uint16)
    vol = ck.multi_volume()
    for conn, rank in ck.CONN:
        comp, n = label_multi(vol, rank)
        assert n < 65536
        g[f"multi_{conn}_n"], g[f"multi_{conn}_map"] = np.int64(n), comp.astype(np.uint16)
    vol = ck.filter_volume()
    for conn, rank in ((6, 1), (26, 3)):
        for name, (kl, ms) in ck.FILTER_CASES.items():
            g[f"filter_{conn}_{name}"] = filtered(vol, rank, kl, ms)
    return g


if __name__ == "__main__":
    path = os.path.join(HERE, "components.npz")
    np.savez_compressed(path, **build())
    print(path, os.path.getsize(path), "bytes")
