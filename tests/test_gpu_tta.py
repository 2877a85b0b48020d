"""-m gpu: mirror test-time augmentation and Gaussian window weights on the MI355X — cbim_window_gather_mirror /
cbim_softmax_accumulate_tta against torch.flip, cbim_softmax_accumulate (bit for bit) and a float64 composition; the args keys of
cbim_amd.inference.inference3d through the ResUNet of tests/infer_checks.py, prediction() and validation() (checks in
tests/tta_checks.py)."""
import pytest

from tests import tta_checks as tc

pytestmark = pytest.mark.gpu


def test_gather_equals_flipped_slice(dev):
    tc.check_gather(dev)


def test_single_variant_is_bit_identical_to_softmax_accumulate(dev):
    tc.check_bit_identity(dev)


def test_accumulate_against_float64_composition(dev):
    tc.check_against_float64(dev)


def test_accumulate_is_reproducible(dev):
    tc.check_reproducible(dev)


def test_argument_errors(dev):
    tc.check_argument_errors(dev)


def test_mirror_equivariance_whole_image(dev):
    tc.check_mirror_equivariance(dev)


def test_sliding_window_against_whole_image_composition(dev):
    tc.check_sliding_window_tta(dev)


def test_defaults_are_the_old_path(dev):
    tc.check_defaults_are_the_old_path(dev)


def test_prediction_and_validation_pick_the_keys_up(dev):
    tc.check_consumers(dev)


def test_key_errors_before_any_launch(dev):
    tc.check_key_errors_before_any_launch(dev)
