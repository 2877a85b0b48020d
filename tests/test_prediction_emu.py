"""CPU suite: volume prediction on the host-side executor — the kernels of csrc/predict_kernels.hip, cbim_amd.inference.resample
and cbim_amd.prediction against numpy, the fixtures the real reference wrote, and scipy's float64 resampling (fixtures of
tests/golden/make_golden_prediction.py).  SimpleITK is not installed where this project is developed: the resamplers are NOT
pinned to ITK's output, only to ITK's documented geometry rules and to scipy.ndimage's numbers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import prediction_checks as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("CBIM_REFERENCE", "/root/reference")


@pytest.fixture(autouse=True)
def _emu_only(dev):
    if dev != "cpu":
        pytest.skip("CPU suite (the -m gpu twin is tests/test_gpu_prediction.py)")


def test_percentile_equals_numpy(dev):
    pc.check_percentile(dev)


def test_pad_unpad_match_reference(dev):
    pc.check_pad_unpad(dev)


def test_ensemble_matches_reference(dev):
    """Two base-8 nets over eight 32^3 windows each: about ten minutes on the host-side executor."""
    pc.check_ensemble_reference(dev)


def test_ensemble_kernel_bit_identical(dev):
    pc.check_ensemble_kernel(dev)


def test_resampling_against_scipy_fixture(dev):
    pc.check_resample(dev, "emu")


def _tiny_nets(dev):
    from cbim_amd.model.dim3 import UNet
    nets = []
    for seed in (41, 42):
        torch.manual_seed(seed)
        nets.append(UNet(1, 4, scale=[[1, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=pc.CLASSES, block="BasicBlock", norm="in").to(dev))
    return nets


def test_round_trip(dev):
    import cbim_amd
    args = pc.pred_args(training_size=[12, 16, 16], window_size=[12, 16, 16])
    cbim_amd.set_compute_dtype("fp32")
    try:
        pc.check_round_trip(dev, _tiny_nets(dev), args, (5, 14, 12), (1.25, 1.25, 2.0))
    finally:
        cbim_amd.set_compute_dtype(None)


def test_two_d_is_refused(dev):
    args = pc.pred_args(dimension="2d")
    for call in (lambda: pc.P.prediction([], torch.zeros(2, 4, 4), args), lambda: pc.P.unpad_img(np.zeros((2, 2, 2)), [0] * 6, args),
                 lambda: pc.P.preprocess(torch.zeros(2, 4, 4), (1, 1, 1), (1, 1, 1), args)):
        with pytest.raises(NotImplementedError):
            call()


def test_reference_prediction_through_the_seam(tmp_path):
    if not os.path.isfile(os.path.join(REFERENCE, "prediction.py")):
        pytest.skip("no reference checkout on this machine")
    env = dict(os.environ)
    assert env.get("CBIM_HIP_LIBRARY"), "CPU suite: the host-side executor library is set by tests/conftest.py"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ref_prediction_seam.py"), REFERENCE, str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=1800)
    assert "PREDICTION-SEAM-OK" in r.stdout, r.stdout + r.stderr


# ---- optional: a randomised property test against live scipy (pinned to the fixture first) --------------------------------------

def _scipy_resample(vol, co, order):
    from scipy import ndimage
    inside = np.ones(co.shape[1:], bool)
    for a in range(3):
        inside &= (co[a] >= -0.5) & (co[a] < vol.shape[a] - 0.5)
    if order == 0:
        return np.where(inside, ndimage.map_coordinates(vol, np.floor(co + 0.5), order=0, mode="nearest"), 0)
    out = ndimage.map_coordinates(vol.astype(np.float64), co, order=order, mode="mirror" if order == 3 else "nearest")
    return np.where(inside, out, 0.0)


def test_random_geometries_against_scipy_restatement(dev):
    pytest.importorskip("scipy")
    from cbim_amd.inference import resample as rs
    from tests.util import load_golden
    g = load_golden("prediction_resample")
    # pin the restatement (and the engine's composed index map) to the fixture first
    m = rs.index_map(pc._geom(g["oblique_geom_src"]), pc._geom(g["oblique_geom_dst"]))
    co = rs.map_coordinates_zyx(m, tuple(int(v) for v in g["oblique_shape_dst"]))
    for key, order in (("cubic", 3), ("linear", 1), ("nearest", 0)):
        assert np.abs(_scipy_resample(g["oblique_vol"], co, order) - g[f"oblique_{key}"]).max() <= 1e-9 * np.abs(g["oblique_vol"]).max()
    rng = np.random.default_rng(2718)
    for trial in range(8):
        shape = tuple(int(v) for v in rng.integers(2, 40, 3))
        vol = (rng.standard_normal(shape) * 100).astype(np.float32)
        sp, tsp = tuple(rng.uniform(0.5, 3.0, 3)), tuple(rng.uniform(0.5, 3.0, 3))
        ang = rng.uniform(-0.4, 0.4)
        d = (np.cos(ang), -np.sin(ang), 0.0, np.sin(ang), np.cos(ang), 0.0, 0.0, 0.0, 1.0) if trial % 2 else rs.IDENTITY
        src, dst = (sp, tuple(rng.uniform(-5, 5, 3)), d), (tsp, tuple(rng.uniform(-5, 5, 3)), rs.IDENTITY)
        out_shape = tuple(int(v) for v in rng.integers(1, 30, 3))
        m = rs.index_map(src, dst)
        co = rs.map_coordinates_zyx(m, out_shape)
        t = torch.from_numpy(vol)
        frac = (co + 0.5) - np.floor(co + 0.5)
        clear = (np.minimum(frac, 1 - frac) > 1e-6).all(0)       # random geometries: compare away from rounding ties only
        assert clear.mean() > 0.99
        assert np.array_equal(rs.resample3d(t, m, out_shape, "nearest").numpy()[clear], _scipy_resample(vol, co, 0)[clear]), trial
        scale = float(np.abs(vol).max())
        for mode, order in (("linear", 1), ("bspline", 3)):
            got = rs.resample3d(t, m, out_shape, mode).numpy()
            assert float(np.abs(got - _scipy_resample(vol, co, order))[clear].max()) <= 2e-5 * scale, (trial, mode)
