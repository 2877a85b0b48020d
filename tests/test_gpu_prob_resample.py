"""-m gpu: class probabilities resampled to the scan grid, fused with the argmax, on the MI355X — cbim_resample_argmax against the
composition resample3d('linear') + argmax and against scipy's float64 result stored in the fixture; crop, counter, ties, graph
capture, allocator high-water mark; predict_volume(resample='probabilities') through the ResUNets of tests/prediction_checks.py,
the first of which is the net of tests/infer_checks.py (checks in tests/prob_resample_checks.py)."""
import pytest

from tests import prob_resample_checks as rc

pytestmark = pytest.mark.gpu


def test_labels_equal_the_composition(dev):
    rc.check_against_composition(dev, "gpu")


def test_labels_equal_float64_fixture(dev):
    rc.check_against_float64(dev, "gpu")


def test_crop_is_the_sliced_out_copy(dev):
    rc.check_crop(dev)


def test_counter_is_the_materialised_division(dev):
    rc.check_counter(dev)


def test_ties_edges_and_refusals(dev):
    rc.check_ties_and_edges(dev)


def test_reproducible_and_capturable(dev):
    rc.check_reproducible(dev)


def test_no_channel_temporary(dev):
    rc.check_no_channel_temporary(dev)


def test_through_predict_volume(dev):
    from tests import prediction_checks as pc
    nets, _ = pc.ensemble_nets(dev)
    rc.check_public_surface(dev, nets, pc.pred_args(), (10, 36, 30), (1.25, 1.25, 2.5))


def test_unknown_mode_raises_before_any_launch(dev):
    rc.check_unknown_mode(dev)
