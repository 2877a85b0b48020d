"""-m gpu: the top-k cross-entropy kernels (csrc/topk_kernels.hip) on the MI355X, against the float64 results stored in
tests/golden/topk.npz; one benchmark-like size against the float32 torch composition and graph capture on top (checks in
tests/topk_checks.py)."""
import pytest

from tests import topk_checks as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", tc.CASES)
def test_fixture_cases_through_topk_loss(dev, name):
    tc.check_fixture_case(dev, name)


@pytest.mark.parametrize("name", tc.CASES)
def test_dice_topk_is_topk_plus_dice(dev, name):
    tc.check_dice_topk(dev, name)


def test_k100_is_the_mean_cross_entropy(dev):
    tc.check_k100_is_mean_ce(dev)


def test_dice_term_is_bit_equal_to_the_ce_dice_kernels(dev):
    tc.check_dice_bits(dev)


def test_one_pass_equals_the_two_modules(dev):
    tc.check_two_modules_agree(dev)


def test_ties_at_the_threshold_share_evenly(dev):
    tc.check_ties(dev)


def test_saturated_logits_stay_finite(dev):
    tc.check_saturation(dev)


def test_out_of_range_labels_are_counted_not_indexed(dev):
    tc.check_bad_labels(dev)


def test_out_of_range_labels_through_the_modules(dev):
    tc.check_bad_labels_through_modules(dev)


def test_misaligned_base_pointer(dev):
    tc.check_misaligned(dev)


def test_reproducible(dev):
    tc.check_reproducible(dev)


def test_bad_arguments(dev):
    tc.check_bad_arguments(dev)


def test_target_shapes_and_spatial_ranks(dev):
    tc.check_target_shapes_and_ranks(dev)


def test_size_1x16x32x32x32(dev):
    tc.check_size(dev)


def test_graph_capture_replays_bit_equal(dev):
    tc.check_graph_capture(dev)
