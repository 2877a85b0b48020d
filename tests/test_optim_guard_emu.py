"""CPU suite: the guarded FusedAdamW step (global-norm clipping, the GradScaler protocol, skipped non-finite steps) with the kernels
of csrc/optim_kernels.hip on the host-side executor, against torch's clip_grad_norm_ + AdamW (checks in tests/optim_guard_checks.py)."""
import pytest

from tests import optim_guard_checks as gc


@pytest.fixture(autouse=True)
def _emu_only(dev):
    if dev != "cpu":
        pytest.skip("CPU suite (the -m gpu twin is tests/test_gpu_optim_guard.py)")


def test_parity_with_clip_grad_norm_and_adamw(dev):
    gc.check_parity(dev)


def test_huge_limit_is_no_limit_bit_for_bit(dev):
    gc.check_huge_limit_is_no_limit(dev)


def test_nonfinite_gradient_skips_the_step(dev):
    gc.check_nonfinite_skips(dev)


def test_parity_through_grad_scale_65536(dev):
    gc.check_parity(dev, scale=65536.0)


def test_amp_protocol_attributes(dev):
    gc.check_amp_protocol(dev)


def test_misaligned_base_pointers(dev):
    gc.check_misaligned(dev)


def test_reproducible(dev):
    gc.check_reproducible(dev)


def test_parameter_without_gradient(dev):
    gc.check_inactive_parameter(dev)


def test_bad_arguments(dev):
    gc.check_bad_arguments(dev)


def test_grad_norm_and_get_optimizer_surface(dev):
    gc.check_surface(dev)
