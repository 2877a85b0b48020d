"""Class probabilities resampled to the scan grid, fused with the argmax (cbim_resample_argmax of csrc/predict_kernels.hip,
cbim_amd.inference.resample.resample_argmax / resample_probabilities_to_ref, the `probabilities=` keyword of
prediction.postprocess and `resample=` of prediction.predict_volume) — shared by the CPU (host-side executor,
tests/test_prob_resample_emu.py) and -m gpu (tests/test_gpu_prob_resample.py) suites.

Two references: the composition the engine already had (resample3d 'linear' over the K channels, then argmax) and scipy's
float64 map_coordinates stored in tests/golden/prob_resample.npz (tests/golden/make_golden_prob_resample.py; scipy is not
imported here).  Labels are compared where the reference's top-two margin is above a bar (1e-6 on the float32 composition: a few
ulp of probabilities <= 2 under different — here identical — summation; 1e-5 on float64: the float32 evaluation of an 8-tap
convex combination of values <= 2 is within 8 * 2^-23 * 2 = 2e-6 of it on either class); the share of in-buffer voxels under the
bar is itself bounded by 0.1 %."""
import ctypes as C
import json
import os

import numpy as np
import torch

import cbim_amd
from cbim_amd import _lib
from cbim_amd import prediction as P
from cbim_amd.inference import resample as rs
from cbim_amd.inference.components import filter_components
from cbim_amd.ops import _p
from tests.util import load_golden

CASES = ("a", "b", "c")
MARGIN32, MARGIN64, CAP = 1e-6, 1e-5, 1e-3
IDENT_MAP = np.asarray([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
EINVAL = -1


def record(key, values):
    """observed figures -> $CBIM_PARITY_DIR/prob_resample_parity.json when that directory is named; without it they are only
    printed.  Never a reason to fail."""
    d = os.environ.get("CBIM_PARITY_DIR")
    if not d:
        return
    try:
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "prob_resample_parity.json")
        data = json.load(open(path)) if os.path.isfile(path) else {}
        data[key] = values
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except Exception as e:                                                   # noqa: BLE001
        print(f"record({key}): not written ({type(e).__name__}: {e})")


_FIXTURE = {}


def case(name, dev):
    """(prob on dev, map, destination shape, fixture) — loaded once per device and shared, never modified."""
    if (name, dev) not in _FIXTURE:
        g = load_golden("prob_resample")
        _FIXTURE[(name, dev)] = (torch.from_numpy(g[f"{name}_prob"]).to(dev), g[f"{name}_map"], tuple(int(v) for v in g[f"{name}_shape"]),
                                 {k: g[f"{name}_{k}"] for k in ("label64", "margin64", "inside")})
    return _FIXTURE[(name, dev)]


def inside_mask(m, shape, src):
    co = rs.map_coordinates_zyx(np.asarray(m, np.float64).reshape(3, 4), shape)
    ok = np.ones(co.shape[1:], bool)
    for a in range(3):
        ok &= (co[a] >= -0.5) & (co[a] < src[a] - 0.5)
    return torch.from_numpy(ok)


def compare_to_composition(tag, got, prob, m, shape, counter=None):
    """got == argmax(resample3d(prob / counter, m, shape, 'linear')) wherever the composed top-two margin exceeds MARGIN32; at
    most CAP of the in-buffer voxels are under it; outside voxels are 0.  Returns the number of excluded in-buffer voxels."""
    src = prob if counter is None else prob / counter
    comp = rs.resample3d(src.contiguous(), m, shape, "linear").cpu()
    got = got.cpu()
    inside = inside_mask(m, shape, prob.shape[1:])
    if comp.shape[0] > 1:
        top2 = comp.topk(2, dim=0).values
        clear = ((top2[0] - top2[1]) > MARGIN32) & inside
    else:
        clear = inside
    excluded = int((inside & ~clear).sum())
    wrong = int(((got.long() != comp.argmax(0)) & clear).sum())
    print(f"{tag}: in-buffer {int(inside.sum())}, composed margin <= {MARGIN32} on {excluded}, mismatches on clear voxels {wrong}")
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(shape)
    assert excluded <= CAP * int(inside.sum()), (tag, excluded)
    assert wrong == 0, (tag, wrong)
    assert int(got[~inside].count_nonzero()) == 0, "a voxel outside the buffer must be 0"
    return excluded


def _raises(exc, fn, needle=None):
    try:
        fn()
    except exc as e:
        assert needle is None or needle in str(e), e
        return
    raise AssertionError(f"{exc.__name__} expected")


# ---- 1. / 2. the two references --------------------------------------------------------------------------------------------------

def check_against_composition(dev, tag):
    for name in CASES:
        prob, m, shape, _ = case(name, dev)
        got = rs.resample_argmax(prob, m, shape)
        excluded = compare_to_composition(f"case {name}", got, prob, m, shape)
        record(f"{tag}:{name}:composition", dict(excluded=excluded))


def check_against_float64(dev, tag):
    for name in CASES:
        prob, m, shape, fx = case(name, dev)
        got = rs.resample_argmax(prob, m, shape).cpu().numpy()
        inside = fx["inside"]
        assert np.array_equal(inside, inside_mask(m, shape, prob.shape[1:]).numpy())
        clear = inside & (fx["margin64"] > MARGIN64)
        excluded = int((inside & ~clear).sum())
        wrong = int(((got != fx["label64"]) & clear).sum())
        print(f"case {name}: float64 margin <= {MARGIN64} on {excluded} of {int(inside.sum())}, mismatches on clear voxels {wrong}")
        record(f"{tag}:{name}:float64", dict(excluded=excluded, wrong=wrong))
        assert excluded <= CAP * int(inside.sum()) and wrong == 0, (name, excluded, wrong)
        assert int((got[~inside] != 0).sum()) == 0 and int((~inside).sum()) > 0


# ---- 3. crop ------------------------------------------------------------------------------------------------------------------------

CROP = (2, 7, 2, 8, 3, 10)                  # case a (5 x 6 x 7) inside a 9 x 10 x 12 buffer


def check_crop(dev):
    """The padding holds probability 1 for class 2 (count 1): a tap clamped into it, or an inside test on the buffer's extents,
    shows as class 2 on the rim.  With crop= the labels are those of the sliced-out contiguous copy, bit for bit."""
    prob, m, shape, _ = case("a", dev)
    z0, z1, y0, y1, x0, x1 = CROP
    buf = torch.zeros((3, 9, 10, 12), device=dev)
    buf[2] = 1.0
    buf[:, z0:z1, y0:y1, x0:x1] = prob
    plain = rs.resample_argmax(prob, m, shape)
    got = rs.resample_argmax(buf, m, shape, crop=CROP)
    assert torch.equal(got, rs.resample_argmax(buf[:, z0:z1, y0:y1, x0:x1].contiguous(), m, shape)) and torch.equal(got, plain)
    assert not torch.equal(rs.resample_argmax(buf, m, shape), plain), "the buffer without the crop is another image"
    gen = torch.Generator().manual_seed(7)
    cnt = torch.ones((9, 10, 12))
    cnt[z0:z1, y0:y1, x0:x1] = torch.randint(1, 5, (5, 6, 7), generator=gen).float()
    cnt = cnt.to(dev)
    sums = buf * cnt
    got_c = rs.resample_argmax(sums, m, shape, counter=cnt, crop=CROP)
    want_c = rs.resample_argmax(sums[:, z0:z1, y0:y1, x0:x1].contiguous(), m, shape, counter=cnt[z0:z1, y0:y1, x0:x1].contiguous())
    assert torch.equal(got_c, want_c)
    compare_to_composition("crop + counter", got_c, sums[:, z0:z1, y0:y1, x0:x1], m, shape, counter=cnt[z0:z1, y0:y1, x0:x1])
    # a leading corner of a larger buffer (what prediction(return_total=True) returns for a volume under one window) is read in place
    corner = torch.zeros((3, 7, 9, 8), device=dev)
    corner[:, :, :, :] = 5.0
    corner[:, :5, :6, :7] = prob
    assert torch.equal(rs.resample_argmax(corner[:, :5, :6, :7], m, shape), plain)
    assert rs._buffer_box(corner[:, :5, :6, :7]) == (7, 9, 8) and rs._buffer_box(prob.transpose(2, 3)) is None
    turned = corner[:, :6, :5, :7].transpose(1, 2)                           # any other view is copied first
    assert torch.equal(rs.resample_argmax(turned, m, shape), rs.resample_argmax(turned.contiguous(), m, shape))
    _raises(ValueError, lambda: rs.resample_argmax(corner[:, :5, :6, :7], m, shape, crop=(0, 6, 0, 6, 0, 7)))


# ---- 4. counter -------------------------------------------------------------------------------------------------------------------

def check_counter(dev):
    """prob_sum = total * counter with counts 1..8: the labels through counter= are those of the tensor prob_sum / counter that
    torch forms in float32, bit for bit (the per-tap division is the materialised division)."""
    gen = torch.Generator().manual_seed(8)
    for name in ("a", "b"):
        total, m, shape, _ = case(name, dev)
        cnt = torch.randint(1, 9, tuple(total.shape[1:]), generator=gen).float().to(dev)
        sums = total * cnt
        got = rs.resample_argmax(sums, m, shape, counter=cnt)
        assert torch.equal(got, rs.resample_argmax(sums / cnt, m, shape)), name
        compare_to_composition(f"counter, case {name}", got, sums, m, shape, counter=cnt)


# ---- 5. ties and edges ------------------------------------------------------------------------------------------------------------

def check_ties_and_edges(dev):
    prob, m, shape, _ = case("a", dev)
    src = tuple(prob.shape[1:])
    inside = inside_mask(m, shape, src)
    assert int(rs.resample_argmax(torch.full((4,) + src, 0.25, device=dev), m, shape).count_nonzero()) == 0       # all classes equal
    gen = torch.Generator().manual_seed(9)
    tie = torch.rand((5,) + src, generator=gen)
    tie[3] = tie[1] = tie.max(0).values + 0.5                                                                     # two identical maxima
    got = rs.resample_argmax(tie.to(dev), m, shape).cpu()
    assert bool((got[inside] == 1).all()) and int(got[~inside].count_nonzero()) == 0
    # integer coordinates: the labels of prediction's ensemble kernel, with and without the count
    both = torch.rand((6,) + src, generator=gen)
    both[:, 2] = both[0, 2]                                                                                       # a plane of exact ties
    cnt = torch.randint(1, 9, src, generator=gen).float().to(dev)
    both = both.to(dev)
    for c in (None, cnt):
        want = torch.empty(src, dtype=torch.uint8, device=dev)
        P.ensemble_finalize(both, c, None, want, True, True)
        assert torch.equal(rs.resample_argmax(both, IDENT_MAP, src, counter=c), want)
    away = IDENT_MAP.copy()
    away[:, 3] = (100.0, -40.0, 0.0)
    assert int(rs.resample_argmax(prob, away, shape).count_nonzero()) == 0                                        # wholly outside
    assert int(rs.resample_argmax(prob[:1].contiguous(), m, shape).count_nonzero()) == 0                          # K = 1
    wide = torch.rand((256, 3, 4, 5), generator=gen)                                                              # K = 256
    wide[200, 1:] += 2.0
    wm = np.asarray([[0.45, 0, 0, -0.2], [0, 0.8, 0, 0.1], [0, 0, 0.6, -0.3]])
    got = rs.resample_argmax(wide.to(dev), wm, (7, 5, 9))
    compare_to_composition("K = 256", got, wide.to(dev), wm, (7, 5, 9))
    assert int((got == 200).sum()) > 0, "labels above 127 come back as uint8"
    _raises(RuntimeError, lambda: rs.resample_argmax(torch.rand(257, 2, 2, 2).to(dev), IDENT_MAP, (2, 2, 2)), "code -1")
    for crop in ((0, 6, 0, 6, 0, 7), (2, 2, 0, 6, 0, 7), (-1, 3, 0, 6, 0, 7), (0, 5, 0, 6, 3, 8)):
        _raises(RuntimeError, lambda: rs.resample_argmax(prob, m, shape, crop=crop), "code -1")
    _raises(TypeError, lambda: rs.resample_argmax(prob.double(), m, shape))
    _raises(TypeError, lambda: rs.resample_argmax(prob, m, shape, counter=torch.ones(src, dtype=torch.float64)))
    nan = IDENT_MAP.copy()
    nan[1, 1] = float("nan")
    _raises(RuntimeError, lambda: rs.resample_argmax(prob, nan, shape), "code -1")
    # the C entry point itself: null pointers, K = 0, and nothing written
    L = _lib.lib()
    out = torch.full(shape, 77, dtype=torch.uint8, device=dev)
    im = _lib.IndexMap()
    im.m[:] = [float(v) for v in np.asarray(m).reshape(12)]
    crop = (C.c_int * 6)(0, 5, 0, 6, 0, 7)
    st = None if dev == "cpu" else rs._stream(prob)
    assert L.cbim_resample_argmax(None, None, 3, 5, 6, 7, crop, _p(out), *shape, im, st) == EINVAL
    assert L.cbim_resample_argmax(_p(prob), None, 3, 5, 6, 7, None, _p(out), *shape, im, st) == EINVAL
    assert L.cbim_resample_argmax(_p(prob), None, 3, 5, 6, 7, crop, None, *shape, im, st) == EINVAL
    assert L.cbim_resample_argmax(_p(prob), None, 0, 5, 6, 7, crop, _p(out), *shape, im, st) == EINVAL
    assert b"resample_argmax" in L.cbim_last_error_string()
    assert bool((out == 77).all())
    assert L.cbim_resample_argmax(_p(prob), None, 3, 5, 6, 7, crop, _p(out), *shape, im, st) == 0
    assert torch.equal(out, rs.resample_argmax(prob, m, shape))


# ---- 6. reproducible, capturable; 7. no K x native temporary ------------------------------------------------------------------------

def check_reproducible(dev):
    prob, m, shape, _ = case("b", dev)
    gen = torch.Generator().manual_seed(10)
    cnt = torch.randint(1, 9, tuple(prob.shape[1:]), generator=gen).float().to(dev)
    for c in (None, cnt):
        eager = rs.resample_argmax(prob, m, shape, counter=c)
        assert torch.equal(eager, rs.resample_argmax(prob, m, shape, counter=c))
        if dev == "cuda":
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                out = rs.resample_argmax(prob, m, shape, counter=c)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)


def check_no_channel_temporary(dev):
    """GPU only: across resample_argmax the allocator's high-water mark rises by less than 8 bytes per output voxel (the label map
    is 1); the composition's resampled channels alone are 4 K = 64."""
    prob, m, shape, _ = case("b", dev)
    n = shape[0] * shape[1] * shape[2]
    assert prob.shape[0] == 16 and prob.is_contiguous()

    def rise(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        keep = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del keep
        return peak

    rs.resample_argmax(prob, m, shape)                                       # code object and runtime warm
    fused = rise(lambda: rs.resample_argmax(prob, m, shape))
    composed = rise(lambda: rs.resample3d(prob, m, shape, "linear").argmax(0).to(torch.uint8))
    print(f"allocator rise per output voxel: fused {fused / n:.2f} B, composition {composed / n:.2f} B")
    assert fused < 8 * n, (fused, n)
    assert composed >= 64 * n, (composed, n)


# ---- 8. through the public surface ---------------------------------------------------------------------------------------------

def scan(shape, dev):
    """The anisotropic synthetic scan of prediction_checks.check_round_trip."""
    rng = np.random.default_rng(5)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    raw = np.round(600 * np.exp(-3 * (zz ** 2 + yy ** 2 + xx ** 2)) + rng.standard_normal(shape) * 60 - 50).astype(np.float32)
    return torch.from_numpy(raw).to(dev)


def fp32(fn):
    def run(*a, **kw):
        cbim_amd.set_compute_dtype("fp32")
        try:
            return fn(*a, **kw)
        finally:
            cbim_amd.set_compute_dtype(None)
    run.__doc__, run.__name__ = fn.__doc__, fn.__name__
    return run


@fp32
def check_public_surface(dev, nets, args, shape, spacing):
    """predict_volume(resample='probabilities') for one model (sums and counts straight into the kernel) and for two (through
    return_total) against the step-by-step composition preprocess, prediction(return_total=True), un-pad, linear resample,
    argmax; against 'nearest'; the default; components=; equal spacings; an unknown mode."""
    img = scan(shape, dev)
    geom = (tuple(args.target_spacing), (0.0, 0.0, 0.0), rs.IDENTITY)
    ref_geom = (tuple(spacing), (0.0, 0.0, 0.0), rs.IDENTITY)
    m = rs.index_map(geom, ref_geom)
    padded, idx = P.preprocess(img, spacing, args.target_spacing, args)
    assert any(a != 0 for a in idx[0::2]), "the case is meant to need padding"
    z0, z1, y0, y1, x0, x1 = idx
    nearest = P.predict_volume(nets, img, spacing, args)
    assert torch.equal(nearest, P.predict_volume(nets, img, spacing, args, resample="nearest"))
    for models in (nets[:1], nets):
        calls = []
        real = P.ensemble_finalize
        P.ensemble_finalize = lambda *a, **k: calls.append(1) or real(*a, **k)
        try:
            out = P.predict_volume(models, img, spacing, args, resample="probabilities")
        finally:
            P.ensemble_finalize = real
        assert (len(calls) == 0) == (len(models) == 1), "one model: no total is formed, the sums and counts go to the kernel"
        assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(shape) and int(out.max()) < args.classes
        total = P.prediction(models, padded, args, return_total=True)[1]
        compare_to_composition(f"predict_volume, {len(models)} model(s)", out, total[:, z0:z1, y0:y1, x0:x1].contiguous(), m, shape)
        low = P.predict_volume(models, img, spacing, args) if len(models) == 1 else nearest
        differ = int((out != low).sum())
        print(f"{len(models)} model(s): 'probabilities' differs from 'nearest' on {differ} of {out.numel()} voxels")
        assert differ > 0
    spec = {"keep_largest": "all"}               # every class keeps its largest component (filter_components takes no bare True)
    filtered = P.predict_volume(nets, img, spacing, args, resample="probabilities", components=spec)
    assert torch.equal(filtered, filter_components(out.contiguous(), **spec))
    # postprocess, where the keyword lives: probabilities with the label path's arguments
    labels, total = P.prediction(nets, padded, args, return_total=True)
    assert torch.equal(P.postprocess(labels, idx, None, ref_geom, shape, args, probabilities=total), out)
    assert torch.equal(P.postprocess(labels, idx, None, ref_geom, shape, args), nearest)
    # equal spacings: the plain prediction labels
    same = P.predict_volume(nets, img, tuple(args.target_spacing), args, resample="probabilities")
    p2, i2 = P.preprocess(img, tuple(args.target_spacing), args.target_spacing, args)
    lab2, tot2 = P.prediction(nets, p2, args, return_total=True)
    assert torch.equal(same, P.unpad_img(lab2, i2, args))
    assert torch.equal(P.postprocess(lab2, i2, None, (tuple(args.target_spacing),) + ref_geom[1:], shape, args, probabilities=tot2), same)


def check_unknown_mode(dev):
    """ValueError before any launch: the network must never run."""
    class Never(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the network ran")
    from tests import prediction_checks as pc
    for mode in ("linear", "Probabilities", None):
        _raises(ValueError, lambda: P.predict_volume([Never()], torch.zeros(4, 8, 8, device=dev), (1.0, 1.0, 2.0), pc.pred_args(), resample=mode))
