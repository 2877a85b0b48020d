"""Evaluation Dice with the reference's call surface (/root/reference/metric/utils.py:33-82).

The reference sums 0/1 masks in float32; those sums are integers, counted exactly on the GPU
(``cbim_dice_counts``) — the float32 arithmetic around them (the +1e-5 terms, including the reference's
double application in ``calculate_dice_split``) is replayed on the tiny per-class vectors, so results are
bit-identical to the reference's.

``calculate_distance`` (ASD / HD95, metric/utils.py:8-29) gets its surface points and distances from the device
(``metric.surface``) and replays the reference's float64 tail — area lookup, sort, sums, cumulative sums — in numpy on the
compacted lists, in the reference's sequential order.  The neighbour-code -> surfel-area table is an input: it is a literal of
the reference's ``metric/lookup_tables.py`` and is not part of this package (see ``area_table=``).
"""
import numpy as np
import torch

from .. import _lib
from ..ops import _dev_ok, _p, _stream


def _counts(pred, target, C, block):
    pred, target = pred.contiguous().view(-1), target.contiguous().view(-1)
    if pred.dtype not in (torch.int8, torch.int64):
        pred = pred.long()
    if target.dtype not in (torch.int8, torch.int64):
        target = target.long()
    _dev_ok(pred, target)
    N = pred.numel()
    nblk = (N + block - 1) // block
    counts = torch.empty((nblk, C, 3), dtype=torch.int32, device=pred.device)
    _lib.check(_lib.lib().cbim_dice_counts(_p(pred), pred.element_size(), _p(target), target.element_size(), N, block, C,
                                           _p(counts), _stream(pred)), "dice_counts")
    return counts


def calculate_dice(pred, target, C):
    """pred, target: [N, 1] label tensors -> (dice[C], intersection[C], summ[C]) — metric/utils.py:62-82
    (note: the returned summ already includes the +1e-5, as in the reference)."""
    assert pred.shape[0] == target.shape[0]
    c = _counts(pred, target, C, max(int(pred.shape[0]), 1))[0]
    intersection = c[:, 0].to(torch.float32)
    summ = (c[:, 1] + c[:, 2]).to(torch.float32)
    summ += 1e-5
    return 2 * intersection / summ, intersection, summ


def calculate_dice_split(pred, target, C, block_size=64 * 64 * 64):
    """metric/utils.py:33-53: block-wise accumulation (each block's summ carries its own +1e-5)."""
    assert pred.shape[0] == target.shape[0]
    N = int(pred.shape[0])
    counts = _counts(pred, target, C, block_size)
    total_sum = torch.zeros(C, device=pred.device)
    total_intersection = torch.zeros(C, device=pred.device)
    for b in range(counts.shape[0]):
        total_intersection += counts[b, :, 0].to(torch.float32)
        summ = (counts[b, :, 1] + counts[b, :, 2]).to(torch.float32)
        summ += 1e-5
        total_sum += summ
    dice = 2 * total_intersection / (total_sum + 1e-5)
    return dice, total_intersection, total_sum


def _area_table(area_table, spacing_np):
    if area_table is None:
        try:
            from metric import lookup_tables          # the host project the engine is plugged into
        except ImportError as e:
            raise ImportError("cbim_amd: calculate_distance needs the neighbour-code -> surfel-area table; `metric.lookup_tables` "
                              "of the host project is not importable, so pass it with the `area_table=` argument (256 float64 "
                              "values for this spacing, or a callable spacing -> table)") from e
        area_table = lookup_tables.create_table_neighbour_code_to_surface_area
    if callable(area_table):
        area_table = area_table(spacing_np)
    table = np.asarray(area_table, dtype=np.float64)
    if table.shape != (256,):
        raise ValueError(f"area_table must hold 256 values, got shape {table.shape}")
    return table


def _sorted_surfels(distances, codes, table):
    """_sort_distances_surfels (metric/metrics.py:237-259): sorted by the pair (distance, area)."""
    areas = table[codes]
    order = np.lexsort((areas, distances))
    return distances[order], areas[order]


def _percentile_distance(distances, areas, percent):
    """One direction of compute_robust_hausdorff (metric/metrics.py:683-713)."""
    if len(distances) == 0:
        return np.inf
    cum = np.cumsum(areas) / np.sum(areas)
    idx = np.searchsorted(cum, percent / 100.0)
    return distances[min(idx, len(distances) - 1)]


def calculate_distance(label_pred, label_true, spacing, C, percentage=95, *, area_table=None):
    """metric/utils.py:8-29: (ASD_list, HD_list), numpy float64 [C-1], for classes 1 .. C-1 of two [D, H, W] label volumes
    (device or host, int8 or int64); ``nan`` (ASD) / ``inf`` (HD) where a side is empty, as in the reference.
    spacing: tensor or sequence of 3 (a plain sequence is taken as float32, the dtype the reference's datasets deliver).
    area_table: 256 float64 surfel areas indexed by neighbour code for this spacing, or a callable spacing -> table; None
    imports ``metric.lookup_tables`` from the host project and raises ImportError when it is absent."""
    from .surface import spacing_array, surface_distances
    lists = surface_distances(label_pred, label_true, spacing, C)
    table = _area_table(area_table, spacing_array(spacing))
    ASD_list = np.zeros(C - 1)
    HD_list = np.zeros(C - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, s in enumerate(lists):
            d_gp, a_g = _sorted_surfels(s["distances_gt_to_pred"], s["codes_gt"], table)
            d_pg, a_p = _sorted_surfels(s["distances_pred_to_gt"], s["codes_pred"], table)
            # compute_average_surface_distance (metric/metrics.py:625-635)
            ASD_list[i] = (np.sum(d_gp * a_g) / np.sum(a_g) + np.sum(d_pg * a_p) / np.sum(a_p)) / 2
            HD_list[i] = max(_percentile_distance(d_gp, a_g, percentage), _percentile_distance(d_pg, a_p, percentage))
    return ASD_list, HD_list
