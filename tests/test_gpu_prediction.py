"""-m gpu: volume prediction on the MI355X — percentiles against numpy, pad / unpad / ensemble against fixtures the real reference
wrote, the resamplers against scipy's float64 results stored in the fixture.  Neither scipy nor the reference is imported here.
SimpleITK is not installed where this project is developed: the resamplers are NOT pinned to ITK's output, only to ITK's
documented geometry rules and to scipy.ndimage's numbers."""
import pytest

from tests import prediction_checks as pc

pytestmark = pytest.mark.gpu


def test_percentile_equals_numpy(dev):
    pc.check_percentile(dev, big=True)


def test_pad_unpad_match_reference(dev):
    pc.check_pad_unpad(dev)


def test_ensemble_matches_reference(dev):
    pc.check_ensemble_reference(dev)


def test_ensemble_kernel_bit_identical(dev):
    pc.check_ensemble_kernel(dev)


def test_resampling_against_scipy_fixture(dev):
    pc.check_resample(dev, "gpu")


def test_round_trip(dev):
    import cbim_amd
    nets, _ = pc.ensemble_nets(dev)
    for mode in ("fp32", "bf16"):
        cbim_amd.set_compute_dtype(mode)
        try:
            pc.check_round_trip(dev, nets, pc.pred_args(), (10, 36, 30), (1.25, 1.25, 2.5))
        finally:
            cbim_amd.set_compute_dtype(None)
