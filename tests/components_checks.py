"""Connected components and their filter (cbim_amd.inference.components, csrc/components_kernels.hip) — shared by the CPU (host-side
executor) and -m gpu suites.  Every comparison is exact integer equality.

The oracle is scipy.ndimage.label: tests/golden/make_golden_components.py wrote what it gives into tests/golden/components.npz
(scipy is not imported here).  Inputs come from the formulas below, so the fixture holds only results: for the random binary
volumes the component count and, for the small shape, scipy's whole map; for the larger shape the SHA-256 of scipy's int32 map,
which pins the map just as exactly in 32 bytes."""
import hashlib

import numpy as np
import torch

from cbim_amd import _lib
from cbim_amd import prediction as P
from cbim_amd.inference import components as cc
from tests.util import load_golden

CONN = ((6, 1), (18, 2), (26, 3))                     # connectivity, rank of scipy's generate_binary_structure(3, rank)
# no multiple of a tile edge (8, 8, 32), every axis crosses a tile border; then the degenerate ones
SHAPES = ((9, 21, 70), (33, 65, 130), (1, 5, 300), (37, 1, 3), (1, 1, 1))
STORED_MAPS = 1                                        # the first STORED_MAPS shapes have scipy's map in the fixture
DENSITIES = (0.1, 0.31, 0.5)                           # straddling the percolation points of the three connectivities
MULTI_SHAPE, FILTER_SHAPE = (9, 21, 70), (10, 24, 68)
FILTER_CASES = {                                       # name -> (keep_largest, min_size)
    "largest_1_3": ((1, 3), 0),
    "largest_all": ("all", 0),
    "min_4": ((), 4),
    "min_class2_7": ((), {2: 7}),
    "both_1": ((1, 4), {1: 3, 2: 5}),
    "vanish_3": ((3,), {3: 100000}),
}


def uniform(shape, seed):
    """float64 in [0, 1) from a splitmix64 hash of (seed, linear index): the same numbers whatever the numpy version."""
    with np.errstate(over="ignore"):
        h = np.arange(int(np.prod(shape)), dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        h = (h ^ (h >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        h = (h ^ (h >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        h = h ^ (h >> np.uint64(31))
    return ((h >> np.uint64(11)).astype(np.float64) / float(1 << 53)).reshape(shape)


def binary_volume(si, pi):
    return (uniform(SHAPES[si], 100 + 10 * si + pi) < DENSITIES[pi]).astype(np.uint8)


def multi_volume():
    """values 0..5, each with probability 1/6"""
    return np.minimum((uniform(MULTI_SHAPE, 7) * 6).astype(np.uint8), 5)


def filter_volume():
    """Five classes: sparse noise (many small components per class) over background, three boxes, and by hand the boundary and
    tie cases of the filter: class 5 has exactly two components of 6 voxels (the largest, a tie) and one of 5."""
    u = uniform(FILTER_SHAPE, 11)
    v = np.zeros(FILTER_SHAPE, np.uint8)
    for c in (1, 2, 3, 4):
        v[(u >= 0.1 * c) & (u < 0.1 * c + 0.085)] = c
    v[1:5, 2:9, 3:20] = 1
    v[5:9, 10:20, 30:50] = 2
    v[0:3, 15:22, 50:66] = 3
    v[6:10, 0:6, 0:12] = 0
    v[7, 1, 1:7] = 5          # 6 voxels, first in raster order
    v[7, 3, 1:6] = 5          # 5 voxels
    v[9, 5, 5:11] = 5         # 6 voxels: ties with the first one
    return v


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).digest(), dtype=np.uint8)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cc(vol, dev, conn):
    comp, n = cc.connected_components(_t(vol, dev), conn)
    assert comp.dtype == torch.int32 and tuple(comp.shape) == vol.shape and isinstance(n, int)
    return comp.cpu().numpy(), n


def golden():
    return load_golden("components")


# ---- 1. against scipy, three connectivities ----------------------------------------------------------------------------------------

def check_random(dev, oracle=None):
    """oracle: None, or f(volume, rank) -> (map, n) (the CPU suite passes scipy itself on top of the fixture)."""
    g = golden()
    for si in range(len(SHAPES)):
        for pi in range(len(DENSITIES)):
            vol = binary_volume(si, pi)
            for conn, rank in CONN:
                key = f"rand_{si}_{pi}_{conn}"
                comp, n = _cc(vol, dev, conn)
                assert n == int(g[key + "_n"]), (key, n, int(g[key + "_n"]))
                assert np.array_equal(sha(comp), g[key + "_sha"]), key
                if si < STORED_MAPS:
                    assert np.array_equal(comp, g[key + "_map"].astype(np.int32)), key
                if oracle is not None:
                    ref, rn = oracle(vol, rank)
                    assert n == rn and np.array_equal(comp, ref), key
                sizes = cc.component_sizes(_t(vol, dev), conn)
                assert sizes.dtype == torch.int64
                assert np.array_equal(sizes.cpu().numpy(), np.bincount(comp.ravel(), minlength=n + 1)), key


# ---- 2. connectivity really differs --------------------------------------------------------------------------------------------------

def check_connectivity(dev):
    z, y, x = np.meshgrid(np.arange(8), np.arange(9), np.arange(10), indexing="ij")
    board = ((x + y + z) % 2 == 0).astype(np.uint8)
    comp, n = _cc(board, dev, 6)
    assert n == int(board.sum()) == 360                   # one component per voxel, numbered in raster order
    assert np.array_equal(comp[board > 0], np.arange(1, n + 1))
    for conn in (18, 26):
        comp, n = _cc(board, dev, conn)
        assert n == 1 and np.array_equal(comp, board.astype(np.int32))
    corner = np.zeros((3, 4, 5), np.uint8)
    corner[0, 1, 2] = corner[1, 2, 3] = 1
    assert [_cc(corner, dev, c)[1] for c in (6, 18, 26)] == [2, 2, 1]
    edge = np.zeros((3, 4, 5), np.uint8)
    edge[1, 1, 2] = edge[1, 2, 3] = 1
    assert [_cc(edge, dev, c)[1] for c in (6, 18, 26)] == [2, 1, 1]
    for a, b in (((7, 7, 31), (8, 8, 32)), ((7, 8, 32), (8, 7, 31)), ((8, 7, 32), (7, 8, 31))):   # the same across a tile corner
        far = np.zeros((10, 10, 34), np.uint8)
        far[a] = far[b] = 1
        assert [_cc(far, dev, c)[1] for c in (6, 18, 26)] == [2, 2, 1], (a, b)


# ---- 3. long chains across many tiles ------------------------------------------------------------------------------------------------

def serpentines(shape=(17, 40, 130)):
    """Class 1: a one-voxel-thick path through the even z planes (rows at even y over the full width, turning at x = 0 / W - 1,
    planes joined by single voxels in the odd planes); class 2: the same one voxel beside it (odd planes, odd rows, x = 1 .. W - 2).
    Returns (volume, length of path 1, length of path 2)."""
    D, H, W = shape
    v = np.zeros(shape, np.uint8)

    def put(c, z, y, x):
        assert not np.any(v[z, y, x]), (c, z, y, x)
        v[z, y, x] = c

    length = {}
    for c, z0, y0, xa, xb in ((1, 0, 0, 0, W - 1), (2, 1, 1, 1, W - 2)):
        rows = list(range(y0, H, 2))
        planes = list(range(z0, D, 2))
        for k, z in enumerate(planes):
            for r, y in enumerate(rows):
                put(c, z, y, slice(xa, xb + 1))
                if r + 1 < len(rows):
                    put(c, z, y + 1, xb if r % 2 == 0 else xa)
            if k + 1 < len(planes):                        # the path ends where the last row ends; the next plane runs it backwards
                end = (rows[-1], xb if len(rows) % 2 == 1 else xa)
                put(c, z + 1, *(end if k % 2 == 0 else (y0, xa)))
        length[c] = len(planes) * (len(rows) * (xb - xa + 1) + len(rows) - 1) + len(planes) - 1
    return v, length[1], length[2]


def check_serpentine(dev):
    one, n1, _ = serpentines()
    one = np.where(one == 1, 1, 0).astype(np.uint8)
    assert int(one.sum()) == n1
    for conn in (6, 18, 26):
        comp, n = _cc(one, dev, conn)
        assert n == 1 and np.array_equal(comp, one.astype(np.int32)), conn
        assert cc.component_sizes(_t(one, dev), conn).tolist() == [one.size - n1, n1]
    both, n1, n2 = serpentines()
    assert int((both == 1).sum()) == n1 and int((both == 2).sum()) == n2
    for conn in (6, 18, 26):
        comp, n = _cc(both, dev, conn)
        assert n == 2 and np.array_equal(comp, both.astype(np.int32)), conn     # path 1 starts at voxel 0: ids equal classes
        assert cc.component_sizes(_t(both, dev), conn).tolist() == [both.size - n1 - n2, n1, n2]


# ---- 4. multi-class ----------------------------------------------------------------------------------------------------------------------

def check_multi_class(dev):
    g, vol = golden(), multi_volume()
    for conn, _ in CONN:
        comp, n = _cc(vol, dev, conn)
        assert n == int(g[f"multi_{conn}_n"])
        assert np.array_equal(comp, g[f"multi_{conn}_map"].astype(np.int32)), conn
    as64, _ = cc.connected_components(_t(vol.astype(np.int64), dev), 26)       # the other input forms
    assert np.array_equal(as64.cpu().numpy(), g["multi_26_map"].astype(np.int32))
    b = binary_volume(0, 1)
    asbool, n = cc.connected_components(_t(b.astype(bool), dev), 18)
    assert n == int(g["rand_0_1_18_n"]) and np.array_equal(asbool.cpu().numpy(), g["rand_0_1_18_map"].astype(np.int32))


# ---- 5. all background, all one class --------------------------------------------------------------------------------------------

def check_trivial(dev):
    shape = (9, 10, 40)
    zero = np.zeros(shape, np.uint8)
    comp, n = _cc(zero, dev, 26)
    assert n == 0 and not comp.any()
    assert cc.component_sizes(_t(zero, dev)).tolist() == [zero.size]
    assert not cc.filter_components(_t(zero, dev), keep_largest="all", min_size=3).any()
    full = np.full(shape, 7, np.uint8)
    for conn in (6, 18, 26):
        comp, n = _cc(full, dev, conn)
        assert n == 1 and (comp == 1).all()
        assert cc.component_sizes(_t(full, dev), conn).tolist() == [0, full.size]
    assert torch.equal(cc.filter_components(_t(full, dev), keep_largest="all", min_size=full.size), _t(full, dev))
    assert not cc.filter_components(_t(full, dev), min_size=full.size + 1).any()


# ---- 6. filter semantics -----------------------------------------------------------------------------------------------------------------

def check_filter(dev):
    g, vol = golden(), filter_volume()
    t = _t(vol, dev)
    for conn in (6, 26):
        for name, (kl, ms) in FILTER_CASES.items():
            want = g[f"filter_{conn}_{name}"]
            got = cc.filter_components(t, keep_largest=kl, min_size=ms, connectivity=conn)
            assert got.dtype == torch.uint8 and got.data_ptr() != t.data_ptr()
            assert np.array_equal(got.cpu().numpy(), want), (conn, name)
            assert np.array_equal(t.cpu().numpy(), vol)                               # the input is left alone
            alias = t.clone()
            res = cc.filter_components(alias, keep_largest=kl, min_size=ms, connectivity=conn, out=alias)
            assert res is alias and np.array_equal(alias.cpu().numpy(), want), (conn, name, "aliased")
    # what the fixture's cases mean, spelled out (scipy decided the maps; these are the rules of the issue)
    got = cc.filter_components(t, keep_largest=(1, 3)).cpu().numpy()
    for c in (2, 4, 5):
        assert np.array_equal(got == c, vol == c)                                     # classes not listed: bit-identical
    five = vol == 5
    assert int(five.sum()) == 17
    k6 = cc.filter_components(t, min_size={5: 6}).cpu().numpy() == 5                  # exactly min_size stays, min_size - 1 goes
    assert int(k6.sum()) == 12 and not k6[7, 3].any() and k6[7, 1, 1:7].all() and k6[9, 5, 5:11].all()
    assert int((cc.filter_components(t, min_size={5: 7}).cpu().numpy() == 5).sum()) == 0
    tie = cc.filter_components(t, keep_largest=(5,)).cpu().numpy() == 5               # the tie goes to the first in raster order
    assert int(tie.sum()) == 6 and tie[7, 1, 1:7].all()
    both = cc.filter_components(t, keep_largest=(5,), min_size={5: 7}).cpu().numpy()  # largest below min_size: the class vanishes
    assert not (both == 5).any() and np.array_equal(both[vol != 5], vol[vol != 5])
    untouched = cc.filter_components(t, min_size=1)
    assert torch.equal(untouched, t)


# ---- 7. reproducibility ---------------------------------------------------------------------------------------------------------------

def check_reproducible(dev):
    t = _t(binary_volume(1, 2), dev)                                                  # (33, 65, 130), p = 0.5
    runs = []
    for _ in range(2):
        parent = cc._label(t, 26)
        size, best = cc._sizes(t, parent)
        runs.append((parent, size, best, cc.filter_components(t, keep_largest="all", min_size=2)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    parent = runs[0][0].cpu().numpy().ravel()
    fg = parent >= 0
    assert np.array_equal(parent[parent[fg]], parent[fg])                             # flat: every parent is a root
    assert (parent[fg] <= np.flatnonzero(fg)).all()                                   # and the root is the component's first voxel


# ---- 8. by construction, and through a captured graph ----------------------------------------------------------------------------

BOX_SHAPE = (48, 96, 160)
# (class, z0, y0, x0, dz, dy, dx): disjoint, at least one background voxel between any two, across tile borders
BOXES = ((1, 1, 2, 3, 10, 20, 40), (2, 1, 2, 50, 7, 9, 33), (1, 3, 30, 5, 20, 3, 70), (3, 2, 40, 90, 30, 40, 60),
         (4, 14, 2, 50, 5, 5, 5), (2, 25, 60, 2, 20, 30, 80), (3, 40, 2, 2, 7, 50, 31), (4, 36, 62, 100, 11, 31, 59),
         (1, 30, 40, 2, 3, 3, 3), (4, 22, 10, 60, 5, 5, 5))
SINGLES = ((1, 0, 0, 0), (2, 0, 0, 159), (3, 47, 95, 159), (4, 12, 1, 47), (1, 24, 34, 88), (2, 47, 0, 0), (3, 0, 95, 80))


def box_volume():
    v = np.zeros(BOX_SHAPE, np.uint8)
    items = []                                                                        # (first linear index, class, voxels)
    for c, z, y, x, dz, dy, dx in BOXES:
        assert not v[max(z - 1, 0):z + dz + 1, max(y - 1, 0):y + dy + 1, max(x - 1, 0):x + dx + 1].any()
        v[z:z + dz, y:y + dy, x:x + dx] = c
        items.append(((z * BOX_SHAPE[1] + y) * BOX_SHAPE[2] + x, c, dz * dy * dx))
    for c, z, y, x in SINGLES:
        assert not v[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].any()
        v[z, y, x] = c
        items.append(((z * BOX_SHAPE[1] + y) * BOX_SHAPE[2] + x, c, 1))
    return v, sorted(items)


def check_boxes(dev):
    vol, items = box_volume()
    t = _t(vol, dev)
    sizes = [s for _, _, s in items]
    for conn in (6, 26):
        comp, n = cc.connected_components(t, conn)
        assert n == len(items)
        flat = comp.cpu().numpy().ravel()
        assert [int(flat[i]) for i, _, _ in items] == list(range(1, n + 1))           # numbered by first raster voxel
        assert cc.component_sizes(t, conn).tolist() == [vol.size - sum(sizes)] + sizes
    want = np.zeros_like(vol)                                                         # the largest box of each class
    for c in (1, 2, 3, 4):
        _, z, y, x, dz, dy, dx = max((b for b in BOXES if b[0] == c), key=lambda b: (b[4] * b[5] * b[6], -b[1]))
        want[z:z + dz, y:y + dy, x:x + dx] = c
    assert len({b[4] * b[5] * b[6] for b in BOXES if b[0] == 4}) == 2                 # class 4 has a tie of two 125-voxel boxes ...
    assert (want == 4).sum() == 11 * 31 * 59                                          # ... below its largest
    eager = cc.filter_components(t, keep_largest="all", min_size=2)
    assert np.array_equal(eager.cpu().numpy(), want)
    small = cc.filter_components(t, min_size={1: 28, 4: 126}).cpu().numpy()           # 27- and 125-voxel boxes and singles go
    keep = vol.copy()
    for c, z, y, x, dz, dy, dx in BOXES:
        if (c == 1 and dz * dy * dx < 28) or (c == 4 and dz * dy * dx < 126):
            keep[z:z + dz, y:y + dy, x:x + dx] = 0
    for c, z, y, x in SINGLES:
        if c in (1, 4):
            keep[z, y, x] = 0
    assert np.array_equal(small, keep)
    if dev == "cuda":                                                                 # the filter path inside a captured graph
        out = torch.empty_like(t)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            cc.filter_components(t, keep_largest="all", min_size=2, out=out)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- 9. through the public surface ------------------------------------------------------------------------------------------------

SPECS = ({"keep_largest": "all", "min_size": 0, "connectivity": 26}, {"keep_largest": (1,), "min_size": {2: 4}, "connectivity": 6},
         {"min_size": 3})


def check_public_surface(dev, nets, args, shape, spacing, full_specs=1, none_call=True):
    """predict_volume(..., components=spec) == filter_components(predict_volume(...), **spec) for the first full_specs of SPECS
    and, with none_call, components=None == the call without the argument (every one of these is a whole prediction: the CPU
    suite runs the fewest); all SPECS and None also go through postprocess, where the option lives, on the predicted map."""
    rng = np.random.default_rng(5)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    raw = np.round(600 * np.exp(-3 * (zz ** 2 + yy ** 2 + xx ** 2)) + rng.standard_normal(shape) * 60 - 50).astype(np.float32)
    img = torch.from_numpy(raw).to(dev)
    plain = P.predict_volume(nets, img, spacing, args)
    if none_call:
        assert torch.equal(P.predict_volume(nets, img, spacing, args, components=None), plain)
    for spec in SPECS[:full_specs]:
        got = P.predict_volume(nets, img, spacing, args, components=spec)
        assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(shape)
        assert torch.equal(got, cc.filter_components(plain.contiguous(), **spec)), spec
    geom = (tuple(spacing), (0.0, 0.0, 0.0), P.IDENTITY)
    idx = [0, shape[0], 0, shape[1], 0, shape[2]]
    assert torch.equal(P.postprocess(plain, idx, geom, geom, shape, args), plain)
    assert torch.equal(P.postprocess(plain, idx, geom, geom, shape, args, components=None), plain)
    for spec in SPECS:
        got = P.postprocess(plain, idx, geom, geom, shape, args, components=spec)
        assert torch.equal(got, cc.filter_components(plain.contiguous(), **spec)), spec
    # on the scan's grid: the filter comes after the resampling back (a coarser label grid, nearest neighbour up to the scan's)
    coarse = plain[::2, ::2, ::2].contiguous()
    cgeom = (tuple(2 * v for v in spacing), tuple(0.5 * v for v in spacing), P.IDENTITY)
    cidx = [0, coarse.shape[0], 0, coarse.shape[1], 0, coarse.shape[2]]
    up = P.postprocess(coarse, cidx, cgeom, geom, shape, args)
    assert tuple(up.shape) == tuple(shape)
    assert torch.equal(P.postprocess(coarse, cidx, cgeom, geom, shape, args, components=SPECS[0]),
                       cc.filter_components(up.contiguous(), **SPECS[0]))
    try:
        P.postprocess(plain, idx, geom, geom, shape, args, components={"largest": 1})
    except ValueError:
        pass
    else:
        raise AssertionError("an unknown key must raise ValueError")
    return plain


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------------

def _raises(fn):
    try:
        fn()
    except ValueError:
        return True
    return False


def check_refusals(dev):
    ok = torch.zeros((3, 4, 5), dtype=torch.uint8, device=dev)
    assert _raises(lambda: cc.connected_components(ok, 8))
    assert _raises(lambda: cc.filter_components(ok, connectivity=8))
    assert _raises(lambda: cc.component_sizes(ok, connectivity=4))
    assert _raises(lambda: cc.connected_components(torch.zeros((1, 3, 4, 5), dtype=torch.uint8, device=dev)))
    assert _raises(lambda: cc.connected_components(torch.zeros((3, 4, 5), dtype=torch.float32, device=dev)))
    assert _raises(lambda: cc.connected_components(torch.full((3, 4, 5), 256, dtype=torch.int64, device=dev)))
    assert _raises(lambda: cc.connected_components(torch.full((3, 4, 5), -1, dtype=torch.int64, device=dev)))
    assert _raises(lambda: cc.filter_components(ok, keep_largest=(256,)))
    assert _raises(lambda: cc.filter_components(ok, keep_largest="largest"))
    assert _raises(lambda: cc.filter_components(ok, out=torch.zeros((3, 4, 5), dtype=torch.int32, device=dev)))
    assert _raises(lambda: cc.connected_components(np.zeros((3, 4, 5), np.uint8)))
    # the ABI: 2^31 voxels or more are refused from the dimensions alone; nothing is allocated or launched
    lib = _lib.lib()
    assert lib.cbim_components_workspace_bytes(2048, 1024, 1024) == -1               # CBIM_EINVAL
    assert lib.cbim_components_workspace_bytes(1 << 20, 1 << 20, 1 << 20) == -1
    assert lib.cbim_components_workspace_bytes(0, 4, 4) == -1
    assert lib.cbim_components_workspace_bytes(2047, 1024, 1024) == (2047 * 1024 * 1024 // 2048) * 4
    assert lib.cbim_components_workspace_bytes(1, 1, 1) == 16
    assert lib.cbim_components_label(None, 2048, 1024, 1024, 26, None, None) == -1
    assert "2^31" in lib.cbim_last_error_string().decode()
    assert lib.cbim_components_sizes(None, None, 2048, 1024, 1024, None, None, None) == -1
    assert lib.cbim_components_number(None, 2048, 1024, 1024, None, None, None, None) == -1
    assert lib.cbim_components_filter(None, None, None, None, None, None, None, 1 << 31, None) == -1
    assert lib.cbim_components_label(None, 3, 4, 5, 26, None, None) == -1             # null pointers
    parent = torch.empty(61, dtype=torch.int32, device=dev)
    assert lib.cbim_components_label(ok.data_ptr(), 3, 4, 5, 8, parent.data_ptr(), None) == -1
    assert "connectivity" in lib.cbim_last_error_string().decode()
    raw = torch.empty(256, dtype=torch.uint8, device=dev)
    assert lib.cbim_components_label(ok.data_ptr(), 3, 4, 5, 26, raw.data_ptr() + 1, None) == -1   # misaligned int32
