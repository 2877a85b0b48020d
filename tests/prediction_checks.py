"""Volume prediction (cbim_amd.prediction, cbim_amd.inference.resample, csrc/predict_kernels.hip) against the fixtures of
tests/golden/make_golden_prediction.py — shared by the CPU (host-side executor) and -m gpu suites.

What is pinned to what: percentiles to numpy (bit for bit); pad / unpad / ensemble to the REAL reference; the ensemble kernel to the
three torch operations it replaces (bit for bit).  The two resamplers CANNOT be pinned to ITK: SimpleITK is not installed where
this project is developed.  Their geometry rules are ITK's documented ones and their numbers are held against scipy.ndimage in
float64 (stored in the fixture; scipy is not imported here)."""
import argparse
import json
import os

import numpy as np
import torch

import cbim_amd
from cbim_amd import prediction as P
from cbim_amd.inference import resample as rs
from tests.util import load_golden, rel_err

SEEDS, TRAIN, CLASSES, BASE = (5051, 5052), [32, 32, 32], 3, 8
FP32_FACTOR = 4.0        # the project's fp32 bar (README, round 5): at most 4x as far from float64 as a plain float32 evaluation
CASES = ("up", "down", "oblique")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pred_args(**kw):
    a = argparse.Namespace(dimension="3d", classes=CLASSES, training_size=TRAIN, window_size=TRAIN, sliding_window=True,
                           target_spacing=(1.0, 1.0, 1.0))
    a.__dict__.update(kw)
    return a


# ---- 1. order statistics and percentile ------------------------------------------------------------------------------------------

def percentile_arrays(big):
    rng = np.random.default_rng(77)
    a = np.round(rng.standard_normal(4099) * 40).astype(np.float32) / 8          # duplicates, negatives
    a[::5] = 0.0
    a[1::9] = -0.0
    out = {"mixed_4099": a, "ragged_1001": rng.standard_normal(1003).astype(np.float32)[2:],       # 8-byte, not 16-byte aligned
           "constant": np.full(77, -3.25, np.float32), "single": np.asarray([1.5], np.float32),
           "pair": np.asarray([2.0, -1.0], np.float32),
           "ct_like": np.round(rng.standard_normal(38400) * 180 + 120).astype(np.float32)}
    if big:                                                                         # >= 2^24 elements, ragged
        b = rng.standard_normal((1 << 24) + 13).astype(np.float32)
        b[::3] = np.round(b[::3] * 4) / 4
        out["big_2p24"] = b
    return out


def _same_float(got, want):
    """bit for bit; between a +0 and a -0 that tie inside the data numpy's own partition order is unspecified, there the value
    decides"""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype:
        return False
    return got.tobytes() == want.tobytes() or (float(got) == 0.0 and float(want) == 0.0)


def check_percentile(dev, big=False):
    for name, a in percentile_arrays(big).items():
        t = torch.from_numpy(a).to(dev)
        for q in (0, 50, 98, 100):
            got, want = rs.percentile(t, q), np.percentile(a, q)
            assert _same_float(got, want), (name, q, got, want)
        n = a.size
        ranks = sorted({0, n // 3, n - 1, (n * 98) // 100})[:4]
        assert np.array_equal(rs.order_stats(t, ranks), np.sort(a)[ranks]), name


# ---- 2. pad / unpad / ensemble against the reference ------------------------------------------------------------------------

def ensemble_nets(dev):
    from cbim_amd.model.dim3 import UNet
    from oracle.unet_ref import make_unet_state_dict, state_dict_checksum
    g = load_golden("prediction_ensemble")
    nets = []
    for seed, chk in zip(SEEDS, g["sd_checksum"]):
        sd = make_unet_state_dict(1, BASE, CLASSES, [[3, 3, 3]] * 5, "BasicBlock", seed=seed)
        assert abs(state_dict_checksum(sd) - float(chk)) < 1e-6
        net = UNet(1, BASE, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=CLASSES, block="BasicBlock", norm="in")
        net.load_state_dict(sd)
        nets.append(net.to(dev))
    return nets, g


def check_pad_unpad(dev):
    g = load_golden("prediction_ensemble")
    args = pred_args()
    raw = g["raw"].astype(np.float32)
    for img in (raw, torch.from_numpy(raw).to(dev)):
        padded, idx = P.pad_to_training_size(img, args)
        assert list(idx) == [int(v) for v in g["original_idx"]] and tuple(padded.shape) == tuple(int(v) for v in g["padded_shape"])
        back = P.unpad_img(padded, idx, args)
        assert tuple(back.shape) == raw.shape and np.array_equal(np.asarray(back.cpu() if torch.is_tensor(back) else back), raw)
    # odd differences: the reference's `+2` pads (34 - 21) // 2 = 6 on both sides of a 21-voxel axis, 33 in all
    padded, idx = P.pad_to_training_size(np.zeros((21, 32, 5), np.float32), args)
    assert padded.shape == (33, 32, 33) and idx == [6, 27, 0, 32, 14, 19]
    for bad in ("2d",):
        try:
            P.pad_to_training_size(raw, pred_args(dimension=bad))
        except NotImplementedError:
            continue
        raise AssertionError("2-D must raise NotImplementedError")


def check_ensemble_reference(dev):
    """The engine in fp32 mode against the reference's two-model ensemble: same original_idx and shapes, summed probabilities
    within rel_err 1e-4 (tests/infer_checks.py:53), labels equal wherever the reference's top-2 margin exceeds 2e-5 (1e-5 per
    model, infer_checks.py:56), labels equal to the argmax of the engine's own sum everywhere."""
    nets, g = ensemble_nets(dev)
    args = pred_args()
    ref_sum = torch.from_numpy(np.stack([load_golden(f"prediction_ensemble_p{k}")["prob_sum"] for k in range(CLASSES)]))
    top2 = ref_sum.topk(2, dim=0).values
    clear = (top2[0] - top2[1]) > 2e-5
    share = float((~clear).float().mean())                                     # the generator's own expression
    print(f"share of voxels at or under the 2e-5 margin: {share:.5%}")
    assert share < 1e-3 and share == float(g["low_margin_share"])
    raw = torch.from_numpy(g["raw"].astype(np.float32)).to(dev)
    cbim_amd.set_compute_dtype("fp32")
    try:
        img, idx = P.preprocess(raw, (1.0, 1.0, 1.0), args.target_spacing, args)          # percentile normalisation, pad
        assert list(idx) == [int(v) for v in g["original_idx"]] and tuple(img.shape) == tuple(int(v) for v in g["padded_shape"])
        labels, total = P.prediction(nets, img, args, return_total=True)
        only_labels = P.prediction(nets, img, args) if dev != "cpu" else labels      # (a second ten minutes on the host-side executor)
    finally:
        cbim_amd.set_compute_dtype(None)
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == tuple(img.shape)
    err = rel_err(total.cpu(), ref_sum)
    wrong = int(((labels.cpu() != torch.from_numpy(g["label"])) & clear).sum())
    print(f"summed probabilities rel_err {err:.3e}; label mismatches on clear voxels {wrong}")
    assert err < 1e-4
    assert wrong == 0
    assert torch.equal(labels.cpu().long(), total.cpu().max(0)[1])
    assert torch.equal(labels, only_labels)
    un = P.unpad_img(labels, idx, args)
    assert tuple(un.shape) == tuple(g["label_unpadded"].shape)


# ---- 3. the ensemble kernel alone ---------------------------------------------------------------------------------------------

def check_ensemble_kernel(dev):
    gen = torch.Generator().manual_seed(99)
    for K in (2, 16):
        for M in (1, 2, 3):
            S = (5, 9, 13)
            want = torch.zeros((K,) + S)
            total = torch.full((K,) + S, float("nan"), device=dev) if M > 1 else None
            labels = torch.full(S, 255, dtype=torch.uint8, device=dev)
            for m in range(M):
                ps = torch.rand((K,) + S, generator=gen) * 4
                ps[:, m % 5] = ps[0, m % 5]                                   # exact ties between the classes: first maximum wins
                cnt = torch.randint(1, 9, S, generator=gen).float()
                ps_dev = ps.to(dev)
                P.ensemble_finalize(ps_dev, cnt.to(dev), total, labels, m == 0, m == M - 1)
                assert torch.equal(ps_dev.cpu(), ps), "prob_sum was modified"
                if m < M - 1:
                    assert bool((labels == 255).all()), "labels are written on the last model only"
                pred = ps / cnt                                               # inference3d.py:88
                want += pred                                                  # prediction.py:57
            _, lab = torch.max(want, dim=0)                                   # prediction.py:59
            assert torch.equal(labels.cpu().long(), lab), (K, M)
            if total is not None:
                assert torch.equal(total.cpu(), want), (K, M)
    ps = torch.rand((3, 4, 4, 4), generator=gen).to(dev)                      # whole-image inference: no counter
    labels = torch.empty((4, 4, 4), dtype=torch.uint8, device=dev)
    P.ensemble_finalize(ps, None, None, labels, True, True)
    assert torch.equal(labels.cpu().long(), ps.cpu().max(0)[1])


# ---- 4. resampling ---------------------------------------------------------------------------------------------------------------

def _geom(v):
    return tuple(v[0:3]), tuple(v[3:6]), tuple(v[6:15])


BS_HZ, BS_Z = 24, np.float32(-0.26794919243112270647)


def np32_prefilter(vol):
    """The kernel's recursion as a plain sequential float32 numpy evaluation, axis after axis."""
    c = vol.astype(np.float32).copy()
    z, one = BS_Z, np.float32(1)
    for axis in range(3):
        s = np.moveaxis(c, axis, 0)                                           # a view: written through
        n = s.shape[0]
        s *= np.float32(6)
        if n > BS_HZ:
            zi, c0 = z, s[0].copy()
            for i in range(1, BS_HZ):
                c0 += zi * s[i]
                zi = zi * z
        else:
            zn1 = one
            for _ in range(n - 1):
                zn1 = zn1 * z
            zi, c0 = z, s[0] + zn1 * s[n - 1]
            for i in range(1, n - 1):
                c0 += zi * (s[i] + zn1 * s[n - 1 - i])
                zi = zi * z
            c0 = c0 / (one - zn1 * zn1)
        s[0] = c0
        for i in range(1, n):
            s[i] = s[i] + z * s[i - 1]
        s[n - 1] = (z / (z * z - one)) * (s[n - 1] + z * s[n - 2])
        for i in range(n - 2, -1, -1):
            s[i] = z * (s[i + 1] - s[i])
    return c


def np32_interpolate(src, co, cubic):
    """The kernel's tap sum (x innermost, then y, then z; sequential float32 accumulation) in numpy, with the inside rule."""
    shape = src.shape
    f = np.floor(co)
    t = (co - f).astype(np.float32)
    b = f.astype(np.int64)
    one, half, sixth = np.float32(1), np.float32(0.5), np.float32(1) / np.float32(6)
    w, ix = [], []
    for a in range(3):
        n = shape[a]
        if cubic:
            x = t[a]
            w3 = sixth * x * x * x
            w0 = sixth + half * x * (x - one) - w3
            w2 = x + w0 - np.float32(2) * w3
            w1 = one - w0 - w2 - w3
            w.append([w0, w1, w2, w3])
            p = 2 * n - 2
            mi = [np.mod(b[a] - 1 + k, p) for k in range(4)]
            ix.append([np.where(m >= n, p - m, m) for m in mi])
        else:
            w.append([one - t[a], t[a]])
            ix.append([np.clip(b[a] + k, 0, n - 1) for k in range(2)])
    nt = 4 if cubic else 2
    acc = np.zeros(co.shape[1:], np.float32)
    for a in range(nt):
        plane = np.zeros_like(acc)
        for bb in range(nt):
            row = np.zeros_like(acc)
            for c in range(nt):
                row = row + w[2][c] * src[ix[0][a], ix[1][bb], ix[2][c]]
            plane = plane + w[1][bb] * row
        acc = acc + w[0][a] * plane
    inside = np.ones(acc.shape, bool)
    for a in range(3):
        inside &= (co[a] >= -0.5) & (co[a] < shape[a] - 0.5)
    assert acc.dtype == np.float32
    return np.where(inside, acc, np.float32(0))


def record(key, values):
    """measured ratios -> $CBIM_PARITY_DIR/prediction_parity.json when that directory is named (profiles/prediction_parity.json
    is a copy of one MI355X run); without it the figures are only printed.  Never a reason to fail."""
    d = os.environ.get("CBIM_PARITY_DIR")
    if not d:
        return
    try:
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "prediction_parity.json")
        data = json.load(open(path)) if os.path.isfile(path) else {}
        data[key] = values
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except Exception as e:                                                   # noqa: BLE001
        print(f"record({key}): not written ({type(e).__name__}: {e})")


def check_resample(dev, tag):
    """Nearest: exactly the fixture.  Linear and cubic: the engine's largest distance to scipy's float64 result is at most
    FP32_FACTOR x that of the plain float32 numpy evaluation of the same recursion and tap sum above."""
    g = load_golden("prediction_resample")
    for name in CASES:
        vol = g[f"{name}_vol"]
        src_geom, dst_geom = _geom(g[f"{name}_geom_src"]), _geom(g[f"{name}_geom_dst"])
        shape_dst = tuple(int(v) for v in g[f"{name}_shape_dst"])
        m = rs.index_map(src_geom, dst_geom)
        co = rs.map_coordinates_zyx(m, shape_dst)
        t = torch.from_numpy(vol).to(dev)
        if name != "oblique":                  # same origin and direction: the public ResampleXYZAxis form must give the same grid
            assert rs.resampled_size(vol.shape, src_geom[0], dst_geom[0]) == shape_dst
            out = rs.resample_xyz_axis(t, src_geom[0], dst_geom[0], interp="nearest")
            assert tuple(out.shape) == shape_dst and np.array_equal(out.cpu().numpy(), g[f"{name}_nearest"])
        out = rs.resample3d(t, m, shape_dst, "nearest")
        assert np.array_equal(out.cpu().numpy(), g[f"{name}_nearest"]), name
        assert int((out.cpu().numpy() == 0).sum()) >= int(g[f"{name}_outside"])
        coef32 = np32_prefilter(vol)
        for mode, key, src32 in (("linear", "linear", vol), ("bspline", "cubic", coef32)):
            want = g[f"{name}_{key}"]
            got = rs.resample3d(t, m, shape_dst, mode).cpu().numpy().astype(np.float64)
            plain = np32_interpolate(src32, co, key == "cubic").astype(np.float64)
            d_eng, d_np = float(np.abs(got - want).max()), float(np.abs(plain - want).max())
            ratio = d_eng / d_np
            print(f"{name} {key}: engine {d_eng:.3e}, float32 numpy {d_np:.3e} from float64 (max |value| {np.abs(want).max():.1f}); ratio {ratio:.2f}")
            record(f"{tag}:{name}:{key}", dict(engine=d_eng, numpy_fp32=d_np, ratio=ratio))
            assert d_np > 0 and ratio <= FP32_FACTOR, (name, key, d_eng, d_np)
        # ResampleLabelToRef: a label map on the destination grid back onto the source grid
        lab = torch.from_numpy(g[f"{name}_label"]).to(dev)
        back = rs.resample_label_to_ref(lab, dst_geom, src_geom, vol.shape)
        assert back.dtype == torch.uint8 and np.array_equal(back.cpu().numpy(), g[f"{name}_label_back"]), name
    # channels, int32 bit copies, a non-zero default, and the refusals
    vol = torch.from_numpy(g["up_vol"]).to(dev)
    m = rs.index_map(_geom(g["up_geom_src"]), _geom(g["up_geom_dst"]))
    shape_dst = tuple(int(v) for v in g["up_shape_dst"])
    two = rs.resample3d(torch.stack([vol, -vol]), m, shape_dst, "bspline")
    one = rs.resample3d(vol, m, shape_dst, "bspline")
    assert torch.equal(two[0], one) and torch.equal(two[1], -one)
    bits = vol.view(torch.int32)
    assert torch.equal(rs.resample3d(bits, m, shape_dst, "nearest", default_value=-7)[-1], torch.full(shape_dst[1:], -7, dtype=torch.int32, device=dev))
    try:
        rs.resample3d(vol[:, :1].contiguous(), m, shape_dst, "bspline")
    except RuntimeError as e:
        assert "code -2" in str(e), e                                          # CBIM_EUNSUPPORTED: an axis shorter than 2
    else:
        raise AssertionError("a one-sample axis must be refused by the prefilter")


# ---- 5. round trip -----------------------------------------------------------------------------------------------------------------

def check_round_trip(dev, nets, args, shape, spacing):
    """predict_volume on an anisotropic synthetic scan: a uint8 map of exactly the input's shape, equal to the step-by-step
    composition."""
    rng = np.random.default_rng(5)
    zz, yy, xx = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    raw = np.round(600 * np.exp(-3 * (zz ** 2 + yy ** 2 + xx ** 2)) + rng.standard_normal(shape) * 60 - 50).astype(np.float32)
    img = torch.from_numpy(raw).to(dev)
    out = P.predict_volume(nets, img, spacing, args)
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(shape)
    res = rs.resample_xyz_axis(img, spacing, args.target_spacing, interp="bspline")
    max98 = rs.percentile(res, 98)
    assert _same_float(max98, np.percentile(res.cpu().numpy(), 98))
    norm = torch.clamp(res, 0.0, float(max98)) / float(max98)
    padded, idx = P.pad_to_training_size(norm, args)
    assert any(a != 0 for a in idx[0::2]), "the case is meant to need padding"
    label = P.prediction(nets, padded, args)
    label = P.unpad_img(label, idx, args)
    geom = (tuple(args.target_spacing), (0.0, 0.0, 0.0), rs.IDENTITY)
    back = rs.resample_label_to_ref(label, geom, (tuple(spacing), (0.0, 0.0, 0.0), rs.IDENTITY), shape)
    assert torch.equal(out, back)
    assert int(out.max()) < args.classes
    return out
