"""The channel-slice view contract of the kernel entry points on the host-side executor (tests/view_checks.py)."""
import pytest

from . import view_checks as vc


def _id(v):
    return str(v).replace("torch.", "")


def test_contract_table_is_complete():
    vc.check_contract_complete()
    vc.check_strided_cases_cover_contract()
    vc.check_autograd_cases_complete()


@pytest.mark.parametrize("case,dtype", vc.STRIDED_IDS, ids=_id)
def test_strided_slot_view_equals_dense(dev, case, dtype):
    vc.check_strided_slot(dev, case, dtype)


@pytest.mark.parametrize("family", list(vc.CONV_FAMILIES), ids=_id)
def test_conv_family_view_equals_dense(dev, family):
    for what, k_dense, k_view in vc.check_conv_family(dev, family):
        assert k_dense == k_view or print(f"{what}: dense on {k_dense}, view on {k_view}") is None


@pytest.mark.parametrize("fn,slot", vc.DENSE_IDS, ids=_id)
def test_dense_only_slot_rejects_view(dev, fn, slot, monkeypatch):
    vc.check_dense_slot(dev, fn, slot, monkeypatch)


def test_misaligned_views_rejected(dev, monkeypatch):
    vc.check_misaligned(dev, monkeypatch)


@pytest.mark.parametrize("name,dtype", vc.AUTOGRAD_IDS, ids=_id)
def test_autograd_view_equals_contiguous(dev, name, dtype):
    vc.check_autograd(dev, name, dtype)
