"""Golden fixtures for the surface-distance metrics (ASD / HD95), produced by EXECUTING THE REAL REFERENCE
(metric/utils.py calculate_distance, metric/metrics.py compute_surface_distances) on CPU.
    python tests/golden/make_golden_surface.py [reference checkout, default: $CBIM_REFERENCE or /root/reference]

The label volumes come from tests/surface_checks.py (procedural, integer arithmetic, seeded); stored are a CRC of them and
RESULTS ONLY: per case the spacing, the reference's 256-entry neighbour-code -> area table for it, per class the four sorted
lists, ASD_list and HD_list at percentage 95 / 50 / 100.  The large case (128^3, 16 classes) stores list lengths, sums and a
strided sample instead of the lists.

The reference's empty-mask branches use np.Inf / np.NaN, which numpy 2 dropped: both aliases are set on the numpy module before
the import; the reference itself is not edited.  If a seed ever lands a percentile within rounding of a cumulative-area step
(an ulp-level reordering would then move the index), pick another seed in tests/surface_checks.py — never loosen the bar.
The seeds in use were checked with `margin` below: the smallest |cumulative area - percentage| over all lists is printed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CBIM_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
np.Inf, np.NaN = np.inf, np.nan

from tests import surface_checks as sc  # noqa: E402

STRIDE = 97


def run(pred, gt, spacing, classes):
    import warnings
    from metric import lookup_tables, metrics
    from metric.utils import calculate_distance
    sp = torch.tensor(spacing, dtype=torch.float32)
    out = {"spacing": sp.numpy(), "table": lookup_tables.create_table_neighbour_code_to_surface_area(sp.numpy()),
           "crc": np.int64(sc.labels_crc(pred, gt))}
    margin = 1.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for pct in sc.PERCENTAGES:
            asd, hd = calculate_distance(torch.from_numpy(pred), torch.from_numpy(gt), sp, classes, pct)
            out["ASD"], out[f"HD{pct}"] = asd, hd
        lists = {}
        for c in range(1, classes):
            s = metrics.compute_surface_distances(gt == c, pred == c, sp.numpy())
            lists[c] = {"d_gt": s["distances_gt_to_pred"], "a_gt": s["surfel_areas_gt"],
                        "d_pred": s["distances_pred_to_gt"], "a_pred": s["surfel_areas_pred"]}
            for a in (s["surfel_areas_gt"], s["surfel_areas_pred"]):
                if len(a):
                    cum = np.cumsum(a) / np.sum(a)
                    margin = min([margin] + [float(np.abs(cum - p / 100.0).min()) for p in sc.PERCENTAGES if p < 100])
    return out, lists, margin


def main():
    small = {}
    for key, (pred, gt, spacing, classes) in sc.all_small_cases().items():
        out, lists, margin = run(pred, gt, spacing, classes)
        print(f"{key}: ASD {out['ASD']}  HD95 {out['HD95']}  HD50 {out['HD50']}  HD100 {out['HD100']}  "
              f"points {[len(v['d_gt']) for v in lists.values()]} / {[len(v['d_pred']) for v in lists.values()]}  "
              f"percentile margin {margin:.2e}")
        # the hand-made cases are symmetric (equal areas, cumulative fractions like 4/8 exactly): a step hit there is by
        # construction and the same on both sides; the seeded cases must stay clear of one
        assert margin > 1e-9 or key not in ("A", "B_iso"), "percentile within rounding of a cumulative-area step: pick another seed"
        small.update({f"{key}_{k}": v for k, v in out.items()})
        for c, l in lists.items():
            small.update({f"{key}_c{c}_{k}": np.asarray(v, np.float64) for k, v in l.items()})
    np.savez_compressed(os.path.join(HERE, "surface_small.npz"), **small)

    pred, gt = sc.ellipsoid_pair(sc.CASE_C["shape"], sc.CASE_C["classes"], sc.CASE_C["seed"])
    out, lists, margin = run(pred, gt, sc.CASE_C["spacing"], sc.CASE_C["classes"])
    print(f"C: ASD {out['ASD']}\n   HD95 {out['HD95']}\n   percentile margin {margin:.2e}")
    assert margin > 1e-9
    n = sc.CASE_C["classes"] - 1
    large = {k: out[k] for k in ("spacing", "table", "crc", "ASD", "HD95")}
    large["stride"] = np.int64(STRIDE)
    large["lengths"] = np.zeros((n, 2), np.int64)
    large["sums"] = np.zeros((n, 2, 2))
    for c, l in lists.items():
        for k, side in enumerate(("gt", "pred")):
            d, a = np.asarray(l["d_" + side], np.float64), np.asarray(l["a_" + side], np.float64)
            large["lengths"][c - 1, k] = len(d)
            large["sums"][c - 1, k] = [d[np.isfinite(d)].sum(), np.sort(a).sum()]
            large[f"c{c}_d_{side}"], large[f"c{c}_a_{side}"] = d[::STRIDE], np.sort(a)[::STRIDE]
    np.savez_compressed(os.path.join(HERE, "surface_large.npz"), **large)
    for f in ("surface_small.npz", "surface_large.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
