"""-m gpu: the surface-distance kernels, ``calculate_distance`` and the validation loop on the MI355X against fixtures the real
reference wrote.  Neither scipy nor the reference is imported here."""
import pytest

from tests import surface_checks as sc

pytestmark = pytest.mark.gpu


def test_lists_match_reference(dev):
    sc.check_lists(dev)


def test_asd_hd_match_reference(dev):
    sc.check_metrics(dev)


def test_large_case_matches_reference(dev):
    sc.check_large(dev)


def test_area_table_seam(dev):
    sc.check_table_seam(dev)


def test_input_forms(dev):
    sc.check_input_forms(dev)


def test_validation_loop_sliding_window(dev):
    sc.check_validation(dev)


def test_validation_loop_whole_image(dev):
    sc.check_validation(dev, whole_image=True)
