"""CPU suite: connected components and their filter (csrc/components_kernels.hip) on the host-side executor, against the fixture
scipy wrote (tests/golden/make_golden_components.py) and against scipy itself."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import components_checks as ck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _emu_only(dev):
    if dev != "cpu":
        pytest.skip("CPU suite (the -m gpu twin is tests/test_gpu_components.py)")


def _scipy_label(vol, rank):
    from scipy import ndimage as ndi
    comp, n = ndi.label(vol, ndi.generate_binary_structure(3, rank))
    return comp.astype(np.int32), int(n)


def test_random_volumes_equal_scipy(dev):
    pytest.importorskip("scipy")
    ck.check_random(dev, oracle=_scipy_label)


def test_fixture_is_what_scipy_gives():
    """The stored results are this scipy's results on the formulas' volumes: the generator run in memory equals the file."""
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_golden_components as mg
    finally:
        sys.path.pop(0)
    fresh, stored = mg.build(), ck.golden()
    assert sorted(fresh) == sorted(stored.files)
    for k, v in fresh.items():
        assert np.array_equal(np.asarray(v), stored[k]) and np.asarray(v).dtype == stored[k].dtype, k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "components.npz")) <= 300 * 1024


def test_connectivity_differs(dev):
    ck.check_connectivity(dev)


def test_serpentines(dev):
    ck.check_serpentine(dev)


def test_multi_class(dev):
    ck.check_multi_class(dev)


def test_all_background_and_all_one_class(dev):
    ck.check_trivial(dev)


def test_filter_semantics(dev):
    ck.check_filter(dev)


def test_reproducible(dev):
    ck.check_reproducible(dev)


def test_boxes_by_construction(dev):
    ck.check_boxes(dev)


def test_public_surface(dev):
    """One tiny net of tests/test_prediction_emu.py and its shapes, two whole predictions: a forward on the host-side executor
    takes minutes.  The two-model ensemble and components=None through predict_volume run in the -m gpu twin."""
    import cbim_amd
    from cbim_amd.model.dim3 import UNet
    from tests import prediction_checks as pc
    torch.manual_seed(41)
    net = UNet(1, 4, scale=[[1, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=pc.CLASSES, block="BasicBlock", norm="in").to(dev)
    args = pc.pred_args(training_size=[12, 16, 16], window_size=[12, 16, 16])
    cbim_amd.set_compute_dtype("fp32")
    try:
        ck.check_public_surface(dev, [net], args, (5, 14, 12), (1.25, 1.25, 2.0), full_specs=1, none_call=False)
    finally:
        cbim_amd.set_compute_dtype(None)


def test_refusals(dev):
    ck.check_refusals(dev)
