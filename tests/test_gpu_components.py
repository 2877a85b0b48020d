"""-m gpu: connected components and their filter on the MI355X against the fixture scipy wrote, analytic cases, two runs of the
same input, and a captured graph of the filter path.  Neither scipy nor the reference is imported here."""
import pytest

from tests import components_checks as ck

pytestmark = pytest.mark.gpu


def test_random_volumes_equal_scipy(dev):
    ck.check_random(dev)


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


def test_boxes_by_construction_and_graph_replay(dev):
    ck.check_boxes(dev)


def test_public_surface(dev):
    import cbim_amd
    from tests import prediction_checks as pc
    nets, _ = pc.ensemble_nets(dev)
    cbim_amd.set_compute_dtype("fp32")
    try:
        ck.check_public_surface(dev, nets, pc.pred_args(), (10, 36, 30), (1.25, 1.25, 2.5), full_specs=3)
    finally:
        cbim_amd.set_compute_dtype(None)


def test_refusals(dev):
    ck.check_refusals(dev)
