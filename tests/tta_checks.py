"""Mirror test-time augmentation and Gaussian window weights (cbim_window_gather_mirror, cbim_softmax_accumulate_tta of
csrc/inference_kernels.hip, the args keys of cbim_amd.inference.inference3d) — shared by the CPU (host-side executor,
tests/test_tta_emu.py) and -m gpu (tests/test_gpu_tta.py) suites.

Op level: random logits, no network; volume (9, 20, 100), window (5, 12, 70) — three different extents, one odd (its centre maps
onto itself), W longer than a wavefront and no multiple of 64 — at a non-zero origin and flush with the far corner.
Through the network: fp32 compute mode; on the GPU the ResUNet and volume of tests/infer_checks.py, on the host-side executor
(where one 32^3 forward of that net takes half a minute) a stock-torch stand-in net on small windows."""
import argparse
import ctypes as C
import itertools

import numpy as np
import torch

import cbim_amd
from cbim_amd import _lib
from cbim_amd.inference import inference3d as I
from cbim_amd.inference.utils import split_idx
from cbim_amd.ops import _p
from tests.util import load_golden, rel_err

VOLUME, WINDOW = (9, 20, 100), (5, 12, 70)
ORIGINS = ((2, 3, 7), (4, 8, 30))          # inside; flush with the far corner.  The two windows overlap.
CODE_SETS = {1: [0], 2: [0, 4], 8: list(range(8))}
EINVAL = -1


def _dims(code):
    """tensor dims of an [N, C, D, H, W] array that a flip code reverses"""
    return [2 + a for a in range(3) if code >> a & 1]


def _flip(t, code):
    d = _dims(code)
    return torch.flip(t, d) if d else t


def _weights(dev, sigma_scale=0.2):
    return I.window_weights(WINDOW, "gaussian", sigma_scale, dev)


# ---- 1. gather -----------------------------------------------------------------------------------------------------------------

def check_gather(dev):
    gen = torch.Generator().manual_seed(31)
    for B in (1, 2):
        img = torch.randn((B, 2) + VOLUME, generator=gen).to(dev)
        for (d0, h0, w0) in ORIGINS:
            sl = img[:, :, d0:d0 + WINDOW[0], h0:h0 + WINDOW[1], w0:w0 + WINDOW[2]]
            for codes in (list(range(8)), [5], [0, 4], [7, 2, 1]):
                got = I._gather_mirror(img, codes, d0, h0, w0, WINDOW)
                want = torch.cat([_flip(sl, c) for c in codes])
                assert got.shape == want.shape and torch.equal(got, want), (B, codes, (d0, h0, w0))


# ---- 2. bit identity with cbim_softmax_accumulate ------------------------------------------------------------------------------

def check_bit_identity(dev):
    gen = torch.Generator().manual_seed(32)
    for B, K in itertools.product((1, 2), (3, 16, 19)):              # 19: the any-K form of the kernel
        for (d0, h0, w0) in ORIGINS:
            logits = (torch.randn((B, K) + WINDOW, generator=gen) * 3).to(dev)
            acc0 = torch.rand((B, K) + VOLUME, generator=gen).to(dev) + 0.5      # non-zero: `+=` is what is tested
            cnt0 = torch.randint(1, 5, (B, 1) + VOLUME, generator=gen).float().to(dev)
            a, c = acc0.clone(), cnt0.clone()
            I._accumulate(logits, a, c, d0, h0, w0)
            a2, c2 = acc0.clone(), cnt0.clone()
            I._accumulate_tta(logits, [0], None, a2, c2, d0, h0, w0)
            assert torch.equal(a.view(torch.int32), a2.view(torch.int32)), (B, K)
            assert torch.equal(c.view(torch.int32), c2.view(torch.int32)), (B, K)
            assert not torch.equal(a, acc0)
            a3 = acc0.clone()                                          # no weight sum wanted
            I._accumulate_tta(logits, [0], None, a3, None, d0, h0, w0)
            assert torch.equal(a.view(torch.int32), a3.view(torch.int32))


# ---- 3. / 4. against a float64 composition; reproducibility -----------------------------------------------------------------------

def _tta_case(B, K, V, weighted, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn((V * B, K) + WINDOW, generator=gen) * 3) for _ in ORIGINS]


def _run_engine(dev, logits, B, K, V, weights):
    """Two overlapping windows accumulated, then cbim_prob_finalize: (probabilities, labels, covered mask)."""
    acc = torch.zeros((B, K) + VOLUME, device=dev)
    wsum = torch.zeros((B, 1) + VOLUME, device=dev)
    for lg, (d0, h0, w0) in zip(logits, ORIGINS):
        I._accumulate_tta(lg.to(dev), CODE_SETS[V], weights, acc, wsum, d0, h0, w0)
    covered = (wsum > 0).cpu()
    assert bool((acc.cpu()[~covered.expand_as(acc)] == 0).all()), "a voxel outside both windows was written"
    labels = I._finalize(acc, wsum, True)
    return acc.cpu(), labels.cpu(), covered


def _run_float64(logits, B, K, V, weights):
    """flip back, softmax(dim=1), weight, sum, divide — in float64"""
    num = torch.zeros((B, K) + VOLUME, dtype=torch.float64)
    den = torch.zeros((B, 1) + VOLUME, dtype=torch.float64)
    terms = torch.zeros((B, 1) + VOLUME, dtype=torch.int64)
    if weights is None:
        w3 = torch.ones(WINDOW, dtype=torch.float64)
    else:
        wz, wy, wx = (w.cpu().double() for w in weights)
        w3 = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
    for lg, (d0, h0, w0) in zip(logits, ORIGINS):
        win = (slice(None), slice(None), slice(d0, d0 + WINDOW[0]), slice(h0, h0 + WINDOW[1]), slice(w0, w0 + WINDOW[2]))
        for v, code in enumerate(CODE_SETS[V]):
            p = torch.softmax(_flip(lg[v * B:(v + 1) * B].double(), code), dim=1)
            num[win] += w3 * p
            den[win] += w3
            terms[win] += 1
    return num / den, int(terms.max())


def check_against_float64(dev):
    """|p - p64| <= (N + K + 8) * 2^-22 with N the largest number of (window, variant) terms at a voxel: one rounding per
    accumulated term, the K-term softmax sum, a few ulp for expf and the division, all on values in [0, 1].  Labels equal the
    float64 argmax wherever the float64 top-2 gap exceeds that bound.  Then the same run again: bitwise equal."""
    seed = 400
    for B, K, V, weighted in itertools.product((1, 2), (3, 16), (1, 2, 8), (False, True)):
        seed += 1
        logits = _tta_case(B, K, V, weighted, seed)
        weights = _weights(dev) if weighted else None
        prob, labels, covered = _run_engine(dev, logits, B, K, V, weights)
        want, N = _run_float64(logits, B, K, V, weights)
        assert N == 2 * V
        bound = (N + K + 8) * 2.0 ** -22
        m = covered.expand_as(prob)
        err = float((prob.double() - want)[m].abs().max())
        print(f"B {B} K {K} V {V} weighted {weighted}: max |p - p64| {err:.3e}  bound {bound:.3e}")
        assert err <= bound, (B, K, V, weighted, err, bound)
        top2 = want.topk(2, dim=1).values
        clear = ((top2[:, 0] - top2[:, 1]) > bound) & covered[:, 0]
        assert int(((labels != want.argmax(1)) & clear).sum()) == 0
        assert float(clear.float().mean()) > 0.3
        prob2, labels2, _ = _run_engine(dev, logits, B, K, V, weights)
        assert torch.equal(prob.view(torch.int32), prob2.view(torch.int32)) and torch.equal(labels[covered[:, 0]], labels2[covered[:, 0]])


def check_reproducible(dev):
    """Check 4 on its own, at the largest case: two runs, bitwise equal (no atomics, fixed summation order)."""
    logits = _tta_case(2, 16, 8, True, 77)
    a = _run_engine(dev, logits, 2, 16, 8, _weights(dev))
    b = _run_engine(dev, logits, 2, 16, 8, _weights(dev))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    assert torch.equal(a[1][a[2][:, 0]], b[1][b[2][:, 0]])


# ---- 5. argument errors ------------------------------------------------------------------------------------------------------

def check_argument_errors(dev):
    """CBIM_EINVAL and nothing launched: the buffers keep their contents."""
    L = _lib.lib()
    B, K = 1, 3
    D, H, W = VOLUME
    wd, wh, ww = WINDOW
    logits = torch.randn((8 * B, K) + WINDOW).to(dev)
    acc = torch.full((B, K) + VOLUME, 0.25, device=dev)
    wsum = torch.full((B, 1) + VOLUME, 2.0, device=dev)
    wz, wy, wx = _weights(dev)
    img = torch.randn((B, 2) + VOLUME).to(dev)
    out = torch.full((8 * B, 2) + WINDOW, 7.0, device=dev)

    def codes(c):
        return (C.c_int * len(c))(*c)

    def acc_call(cs, V, ws=(None, None, None), origin=(0, 0, 0), size=WINDOW):
        return L.cbim_softmax_accumulate_tta(_p(logits), codes(cs), V, _p(ws[0]), _p(ws[1]), _p(ws[2]), _p(acc), _p(wsum), B, K,
                                             *size, D, H, W, *origin, None if dev == "cpu" else I._stream(logits))

    def gather_call(cs, V, origin=(0, 0, 0)):
        return L.cbim_window_gather_mirror(_p(img), _p(out), codes(cs), V, B, 2, wd, wh, ww, D, H, W, *origin,
                                           None if dev == "cpu" else I._stream(img))

    nine = list(range(8)) + [0]
    assert acc_call(nine, 9) == EINVAL and gather_call(nine, 9) == EINVAL
    assert acc_call([0], 0) == EINVAL and gather_call([0], 0) == EINVAL
    assert acc_call([0, 8], 2) == EINVAL and gather_call([0, 8], 2) == EINVAL
    assert acc_call([-1], 1) == EINVAL and gather_call([-1], 1) == EINVAL
    for origin in ((5, 0, 0), (0, 9, 0), (0, 0, 31), (-1, 0, 0)):
        assert acc_call([0], 1, origin=origin) == EINVAL and gather_call([0], 1, origin=origin) == EINVAL
    for ws in ((wz, None, None), (None, wy, None), (None, None, wx), (wz, wy, None)):
        assert acc_call([0], 1, ws=ws) == EINVAL
    assert b"weight" in L.cbim_last_error_string()
    assert bool((acc == 0.25).all()) and bool((wsum == 2.0).all()) and bool((out == 7.0).all())
    assert acc_call([0, 4], 2, ws=(wz, wy, wx), origin=ORIGINS[1]) == 0           # and the same call shape is accepted when valid
    assert gather_call([0, 4], 2, origin=ORIGINS[1]) == 0
    try:                                                                             # the python wrapper: vectors of the wrong length
        I._accumulate_tta(logits[:B], [0], (wz, wy, wx[:-1].contiguous()), acc, wsum, 0, 0, 0)
    except ValueError:
        pass
    else:
        raise AssertionError("weight vectors of the wrong length must be refused")


# ---- through the network -----------------------------------------------------------------------------------------------------

def stand_in_nets(dev, n=1):
    """For the host-side executor, where one forward of even a narrow ResUNet takes seconds: small stock-torch convolution stacks
    with random (so not mirror-symmetric) kernels.  What is under test there is the window tail around the network."""
    from tests.infer_checks import CLASSES
    nets = []
    for seed in range(61, 61 + n):
        torch.manual_seed(seed)
        nets.append(torch.nn.Sequential(torch.nn.Conv3d(1, 6, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv3d(6, CLASSES, 3, padding=1)).to(dev))
    return nets


def setup(dev):
    """(net, volume [1, 1, D, H, W] on dev, window, mirror axes of the sliding-window check): the fixture net, its whole volume,
    32^3 windows and all three axes on the GPU; on the host-side executor a stand-in net, a crop of one and a half windows per
    axis and the W axis."""
    from tests.infer_checks import WINDOW as W32, _net
    x = torch.from_numpy(load_golden("infer_resunet_b8")["x"])
    if dev == "cpu":
        return stand_in_nets(dev)[0], x[:, :, :6, :24, :24].contiguous(), [4, 16, 16], (2,)
    return _net(dev)[0], x.to(dev), list(W32), (0, 1, 2)


def infer_args(window, **kw):
    from tests.infer_checks import CLASSES
    a = argparse.Namespace(window_size=list(window), classes=CLASSES, dimension="3d", sliding_window=True)
    a.__dict__.update(kw)
    return a


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
def check_mirror_equivariance(dev):
    """Check 6: T(flip_W(x)) == flip_W(T(x)) to the fp32 bar (1e-4) for the whole-image path under TTA over all three axes —
    both sides are the same eight forwards summed in another order — and NOT without TTA (> 1e-3: the net is not symmetric)."""
    net, x, window, _ = setup(dev)
    x = x[:, :, :window[0], :window[1], :window[2]].contiguous()
    xf = torch.flip(x, [4]).contiguous()
    plain = I.inference_whole_image(net, x)
    e_plain = rel_err(I.inference_whole_image(net, xf).cpu(), torch.flip(plain, [4]).cpu())
    args = infer_args(window, tta_mirror_axes=(0, 1, 2), window_weight="gaussian")       # the weight is ignored here
    t = I.inference_whole_image(net, x, args)
    e_tta = rel_err(I.inference_whole_image(net, xf, args).cpu(), torch.flip(t, [4]).cpu())
    print(f"mirror equivariance along W: without TTA {e_plain:.3e}, with TTA {e_tta:.3e}")
    assert e_plain > 1e-3
    assert e_tta < 1e-4
    assert rel_err(t.sum(1).cpu(), torch.ones_like(t[:, 0]).cpu()) < 1e-5                    # the mean of probabilities
    assert torch.equal(I.inference_whole_image(net, x, infer_args(window)), plain)         # no key: the old path, same bits
    few = I.inference_whole_image(net, x, infer_args(window, tta_mirror_axes=(0, 1, 2), tta_batch=3))
    assert rel_err(few.cpu(), t.cpu()) < 1e-4


def _expected_sliding(net, x, window, axes, mode, sigma_scale):
    """float64, from the public whole-image path per split_idx window (duplicate last window included) and variant."""
    _, _, D, H, W = x.shape
    half = [w // 2 for w in window]
    codes = I.mirror_variants(axes)
    ws = I.window_weights(window, mode, sigma_scale, "cpu")
    if ws is None:
        w3 = torch.ones(tuple(window), dtype=torch.float64)
    else:
        wz, wy, wx = (w.double() for w in ws)
        w3 = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
    num = den = None
    for i, j, k in itertools.product(range(D // half[0]), range(H // half[1]), range(W // half[2])):
        (d0, d1), (h0, h1), (w0, w1) = split_idx(half[0], D, i), split_idx(half[1], H, j), split_idx(half[2], W, k)
        win = x[:, :, d0:d1, h0:h1, w0:w1]
        for code in codes:
            p = _flip(I.inference_whole_image(net, _flip(win, code).contiguous()), code).cpu().double()
            if num is None:
                num = torch.zeros((x.shape[0], p.shape[1], D, H, W), dtype=torch.float64)
                den = torch.zeros((x.shape[0], 1, D, H, W), dtype=torch.float64)
            num[:, :, d0:d1, h0:h1, w0:w1] += w3 * p
            den[:, :, d0:d1, h0:h1, w0:w1] += w3
    return num / den


@fp32
def check_sliding_window_tta(dev):
    """Check 7: Gaussian-weighted sliding window under mirror TTA against the float64 composition of the public whole-image path
    (rel_err < 1e-4); labels are the argmax of the returned probabilities; tta_batch = 1 agrees with the default to the same bar."""
    net, x, window, axes = setup(dev)
    args = infer_args(window, tta_mirror_axes=axes, window_weight="gaussian", window_sigma_scale=0.25)
    prob, labels = I.inference_sliding_window(net, x, args, return_labels=True)
    want = _expected_sliding(net, x, window, axes, "gaussian", 0.25)
    err = rel_err(prob.cpu(), want)
    print(f"sliding window, axes {axes}, gaussian: rel_err to the float64 composition {err:.3e}")
    assert err < 1e-4
    assert torch.equal(labels.cpu(), prob.cpu().argmax(1))
    one = I.inference_sliding_window(net, x, infer_args(window, tta_mirror_axes=axes, window_weight="gaussian",
                                                        window_sigma_scale=0.25, tta_batch=1))
    assert rel_err(one.cpu(), prob.cpu()) < 1e-4
    plain = I.inference_sliding_window(net, x, infer_args(window))
    assert rel_err(plain.cpu(), want) > 1e-3, "the keys were ignored"
    # mirror TTA with the constant weight: the counter is windows x variants
    if dev == "cpu":
        acc, counter, _ = I._sliding_window_accumulate(net, x, infer_args(window, tta_mirror_axes=axes))
        _, c0, _ = I._sliding_window_accumulate(net, x, infer_args(window))
        assert torch.equal(counter, c0 * len(I.mirror_variants(axes)))


@fp32
def check_defaults_are_the_old_path(dev):
    """Check 8: no new key and the keys at their defaults: bitwise the same output, through cbim_softmax_accumulate alone (the new
    entry points are not called); on the GPU also within 1e-4 of the reference's golden, the bar of infer_checks."""
    net, x, window, _ = setup(dev)
    calls = []
    real_gather, real_acc = I._gather_mirror, I._accumulate_tta
    I._gather_mirror = lambda *a, **k: calls.append("gather") or real_gather(*a, **k)
    I._accumulate_tta = lambda *a, **k: calls.append("tta") or real_acc(*a, **k)
    try:
        p0, l0 = I.inference_sliding_window(net, x, infer_args(window), return_labels=True)
        p1, l1 = I.inference_sliding_window(net, x, infer_args(window, tta_mirror_axes=(), window_weight="constant",
                                                               window_sigma_scale=0.125, tta_batch=None), return_labels=True)
        assert calls == []
        I.inference_sliding_window(net, x[:, :, :window[0], :window[1], :window[2]].contiguous(), infer_args(window, tta_mirror_axes=(1,)))
        assert calls == ["gather", "tta"] * 8                                         # the duplicate last windows included
    finally:
        I._gather_mirror, I._accumulate_tta = real_gather, real_acc
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32)) and torch.equal(l0, l1)
    if dev != "cpu":
        g = load_golden("infer_resunet_b8")
        assert rel_err(p0.cpu(), g["prob"]) < 1e-4


@fp32
def check_consumers(dev):
    """Check 9: prediction() with a two-model ensemble under TTA + Gaussian equals the sum of the two models'
    inference_sliding_window results (1e-4 on return_total); the whole-image branch hands the variant mean on with no counter;
    validation() on a one-volume loader with the keys set returns the Dice of that prediction."""
    from cbim_amd import prediction as P
    from cbim_amd.metric.utils import calculate_dice_split
    from cbim_amd.training.validation import validation
    from tests import prediction_checks as pc
    from tests import surface_checks as sc
    keys = dict(tta_mirror_axes=(2,) if dev == "cpu" else (0, 1, 2), window_weight="gaussian", window_sigma_scale=0.25)
    if dev == "cpu":
        nets, window = stand_in_nets(dev, 2), [4, 16, 16]
        img = torch.from_numpy(load_golden("infer_resunet_b8")["x"])[0, 0, :6, :24, :16].contiguous()
    else:
        nets, g = pc.ensemble_nets(dev)
        window = pc.TRAIN
        img, _ = P.preprocess(torch.from_numpy(g["raw"].astype(np.float32)).to(dev), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0), pc.pred_args())
    args = pc.pred_args(training_size=window, window_size=window, **keys)
    labels, total = P.prediction(nets, img, args, return_total=True)
    want = sum(I.inference_sliding_window(n, img[None, None], args)[0] for n in nets)
    err = rel_err(total.cpu(), want.cpu())
    print(f"prediction() under TTA + gaussian: rel_err to the sum of the models' sliding windows {err:.3e}")
    assert err < 1e-4
    assert torch.equal(labels.cpu().long(), total.cpu().max(0)[1])
    plain = P.prediction(nets, img, pc.pred_args(training_size=window, window_size=window), return_total=True)[1]
    assert rel_err(plain.cpu(), want.cpu()) > 1e-3, "the keys were ignored"
    # whole image: the variant mean, no counter
    crop = img[:window[0], :window[1], :window[2]].contiguous()
    wargs = pc.pred_args(training_size=window, window_size=window, sliding_window=False, **keys)
    wl, wt = P.prediction(nets, crop, wargs, return_total=True)
    wwant = sum(I.inference_whole_image(n, crop[None, None], wargs)[0] for n in nets)
    assert rel_err(wt.cpu(), wwant.cpu()) < 1e-4 and torch.equal(wl.cpu().long(), wt.cpu().max(0)[1])
    # validation(): the Dice of the sliding-window prediction under the same keys
    table = load_golden("surface_small")["A_table"]
    shape = (6, 24, 16) if dev == "cpu" else sc.VAL_SHAPE
    items = sc.val_loader(1, shape)
    vargs = sc.val_args(window_size=window, area_table=lambda spacing: table, **keys)
    dice, asd, hd = validation(nets[0], items, vargs)
    _, lp = I.inference_sliding_window(nets[0], items[0][0].float().to(dev), vargs, return_labels=True)
    d = calculate_dice_split(lp.reshape(-1, 1), items[0][1].to(dev).reshape(-1, 1), vargs.classes)[0].cpu().numpy()[1:]
    present = [c for c in range(vargs.classes - 1) if bool((items[0][1] == c + 1).any())]
    assert present and np.array_equal(dice[present], d[present]), (dice, d)


# ---- 10. host logic -----------------------------------------------------------------------------------------------------------

def check_host_logic():
    assert I.mirror_variants(()) == [0]
    assert I.mirror_variants((2,)) == [0, 4] and I.mirror_variants((0,)) == [0, 1] and I.mirror_variants([1]) == [0, 2]
    assert I.mirror_variants((0, 2)) == [0, 1, 4, 5] and I.mirror_variants((2, 0)) == [0, 1, 4, 5]
    assert I.mirror_variants((1, 2)) == [0, 2, 4, 6]
    assert I.mirror_variants((0, 1, 2)) == list(range(8))
    assert I.window_weights((4, 5, 6), "constant", 0.125, "cpu") is None
    for scale in (0.125, 0.3, 1e-3):
        ws = I.window_weights((5, 12, 70), "gaussian", scale, "cpu")
        assert len(ws) == 3
        for w, n in zip(ws, (5, 12, 70)):
            i = np.arange(n, dtype=np.float64)
            want = np.maximum(np.exp(-0.5 * ((i - (n - 1) / 2) / (scale * n)) ** 2), 1e-3).astype(np.float32)
            assert w.dtype == torch.float32 and w.shape == (n,) and np.array_equal(w.numpy(), want)
            assert np.array_equal(w.numpy(), w.numpy()[::-1]), "symmetric about the window centre"
    wz, wy, wx = I.window_weights((5, 12, 70), "gaussian", 1e-6, "cpu")           # the floor: the product stays above 1e-9
    assert float(wz.min()) == float(np.float32(1e-3)) and float(wx[0]) == float(np.float32(1e-3)) and float(wz[2]) == 1.0
    assert float(wz.min() * wy.min() * wx.min()) > 0.99e-9
    bad = (dict(tta_mirror_axes=(3,)), dict(tta_mirror_axes=(1, 1)), dict(window_weight="hann"),
           dict(window_weight="gaussian", window_sigma_scale=0.0), dict(tta_batch=0))
    for kw in bad:
        for call in (lambda a: I._Tta(a, (8, 8, 8), "cpu"), lambda a: I._Tta(a, (8, 8, 8), "cpu", weighted=False)):
            try:
                call(infer_args([8, 8, 8], **kw))
            except ValueError:
                continue
            raise AssertionError(f"{kw} must raise ValueError")


def check_key_errors_before_any_launch(dev):
    """The five ValueError cases through the public entry points, with a net that must never be called."""
    class Never(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the network ran")
    x = torch.zeros(1, 1, 8, 8, 8, device=dev)
    bad = (dict(tta_mirror_axes=(3,)), dict(tta_mirror_axes=(1, 1)), dict(window_weight="hann"),
           dict(window_weight="gaussian", window_sigma_scale=-1.0), dict(tta_batch=0))
    for kw in bad:
        for fn in (I.inference_sliding_window, I.inference_whole_image):
            try:
                fn(Never(), x, infer_args([8, 8, 8], **kw))
            except ValueError:
                continue
            raise AssertionError(f"{kw} must raise ValueError in {fn.__name__}")
