"""-m gpu: the focal loss kernels (csrc/focal_kernels.hip) on the MI355X, against the float64 results of the reference's FocalLoss /
DiceLoss stored in tests/golden/focal.npz; one benchmark-like size and graph capture on top (checks in tests/focal_checks.py)."""
import pytest

from tests import focal_checks as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", fc.CASES)
def test_fixture_cases_through_focal_loss(dev, name):
    fc.check_fixture_case(dev, name)


@pytest.mark.parametrize("name", fc.CASES)
def test_dice_focal_is_focal_plus_dice(dev, name):
    fc.check_dice_focal(dev, name)


def test_one_pass_equals_the_two_modules(dev):
    fc.check_two_modules_agree(dev)


def test_dice_term_is_bit_equal_to_the_ce_dice_kernels(dev):
    fc.check_dice_bits(dev)


def test_saturated_logits_stay_finite(dev):
    fc.check_saturation(dev)


def test_misaligned_base_pointer(dev):
    fc.check_misaligned(dev)


def test_out_of_range_labels_are_counted_not_indexed(dev):
    fc.check_bad_labels(dev)


def test_out_of_range_labels_through_the_modules(dev):
    fc.check_bad_labels_through_modules(dev)


def test_reproducible(dev):
    fc.check_reproducible(dev)


def test_bad_arguments(dev):
    fc.check_bad_arguments(dev)


def test_target_shapes_and_spatial_ranks(dev):
    fc.check_target_shapes_and_ranks(dev)


def test_size_1x16x32x32x32(dev):
    fc.check_size(dev)


def test_graph_capture_replays_bit_equal(dev):
    fc.check_graph_capture(dev)
