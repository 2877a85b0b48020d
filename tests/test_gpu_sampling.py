"""-m gpu: the foreground-oversampling kernels (csrc/sample_kernels.hip) on the MI355X, against numpy; one volume with
W = 320, the no-synchronisation guarantee and graph capture on top (checks in tests/sampling_checks.py)."""
import pytest

from tests import sampling_checks as sc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", sorted(sc.DTYPES))
@pytest.mark.parametrize("name", ("small", "two", "three"))
def test_index_counts_chunks_and_ignored_labels(dev, name, dtype):
    sc.check_index(dev, name, dtype)


@pytest.mark.parametrize("dtype", sorted(sc.DTYPES))
def test_select_every_class_and_rank_of_the_small_volume(dev, dtype):
    sc.check_select_exhaustive(dev, dtype)


@pytest.mark.parametrize("dtype", sorted(sc.DTYPES))
@pytest.mark.parametrize("name", ("two", "three"))
def test_select_edges_and_seeded_draws(dev, name, dtype):
    sc.check_select_edges(dev, name, dtype)


def test_class_choice(dev):
    sc.check_class_choice(dev)


def test_background_only_volume_falls_back(dev):
    sc.check_background_only(dev)


@pytest.mark.parametrize("dtype", sorted(sc.DTYPES))
def test_crop_equals_the_host_coordinate_crop(dev, dtype):
    sc.check_crop_center(dev, dtype)


def test_crop_offsets_keep_the_voxel_inside(dev):
    sc.check_crop_jitter(dev)


def test_crop_of_the_whole_volume_and_too_large(dev):
    sc.check_crop_whole_and_too_large(dev)


def test_misaligned_base_pointer(dev):
    sc.check_misaligned(dev)


def test_non_contiguous_label(dev):
    sc.check_non_contiguous(dev)


def test_bad_arguments(dev):
    sc.check_bad_arguments(dev)


def test_dataset_is_unchanged_without_the_key(dev):
    sc.check_dataset_unchanged_without_the_key(dev)


def test_dataset_forced_samples(dev):
    sc.check_dataset_forced(dev)


def test_dataset_needs_num_classes(dev):
    sc.check_dataset_needs_num_classes(dev)


def test_chunk_borders_inside_rows_40x64x320(dev):
    sc.check_wide_rows(dev)


def test_pick_and_crop_do_not_synchronise(dev):
    sc.check_no_sync(dev)


def test_graph_capture_replays_bit_equal(dev):
    sc.check_graph_capture(dev)
