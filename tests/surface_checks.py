"""Surface-distance metrics (ASD / HD95) and the validation loop against fixtures the REAL reference wrote
(tests/golden/make_golden_surface.py) — shared by the CPU (host-side executor) and -m gpu suites, and by the fixture generator,
which takes its label volumes from here.  Nothing in this file imports scipy or the reference.

Label volumes are procedural (integer arithmetic only, from a seed); the fixtures hold a CRC of them, not the volumes."""
import argparse
import zlib

import numpy as np
import torch

from tests.util import load_golden

RTOL = 1e-12          # both sides float64, a distance is 3 products + 2 adds + a square root: a few ulp (2.2e-16) at most
PERCENTAGES = (95, 50, 100)
SPACING_ANISO = (2.5, 0.8, 1.25)
CASE_A = dict(shape=(48, 64, 56), classes=5, seed=2101, spacing=SPACING_ANISO)
CASE_C = dict(shape=(128, 128, 128), classes=16, seed=2103, spacing=SPACING_ANISO)
CASE_CT = dict(shape=(160, 320, 320), classes=16, seed=2104, spacing=(2.0, 0.8, 0.8))       # tools/bench_surface_metric.py


# ---- procedural label volumes -----------------------------------------------------------------------------------

def _lcg(seed):
    state = [seed & 0x7FFFFFFF]

    def draw(n):
        state[0] = (state[0] * 1103515245 + 12345) & 0x7FFFFFFF
        return (state[0] >> 8) % max(int(n), 1)
    return draw


def ellipsoid_pair(shape, classes, seed, grow2=3):
    """(label_pred, label_true) int8 [D, H, W]: one ellipsoid per foreground class (later classes overwrite earlier ones, centres
    anywhere in the volume so that some are cut by its faces); the prediction is the ground truth with every radius grown by
    grow2 / 2 voxels and the centre moved by up to one voxel.  All in int64 arithmetic on half-voxel radii."""
    draw = _lcg(seed)
    grid = np.ogrid[:shape[0], :shape[1], :shape[2]]
    gt, pred = np.zeros(shape, np.int8), np.zeros(shape, np.int8)
    for c in range(1, classes):
        r2 = [2 * max(2, n // 8 + draw(n // 6 + 1)) for n in shape]
        ctr = [draw(n) for n in shape]
        shift = [draw(3) - 1 for _ in shape]
        for vol, rr, cc in ((gt, r2, ctr), (pred, [r + grow2 for r in r2], [a + b for a, b in zip(ctr, shift)])):
            rz, ry, rx = (np.int64(r) for r in rr)
            dz, dy, dx = (2 * (g.astype(np.int64) - np.int64(o)) for g, o in zip(grid, cc))
            inside = dz * dz * (ry * rx) ** 2 + dy * dy * (rz * rx) ** 2 + dx * dx * (rz * ry) ** 2 <= (rz * ry * rx) ** 2
            vol[inside] = c
    return pred, gt


def labels_crc(pred, gt):
    return zlib.crc32(np.ascontiguousarray(gt, np.int8).tobytes(), zlib.crc32(np.ascontiguousarray(pred, np.int8).tobytes()))


def edge_cases():
    """name -> (label_pred, label_true, spacing, classes): the small cases (<= 16^3)."""
    out = {}
    z = lambda: np.zeros((12, 14, 16), np.int8)                                                      # noqa: E731
    # class 1 only in gt, class 2 only in pred, class 3 in neither, class 4 in both
    gt, pred = z(), z()
    gt[2:6, 3:8, 2:7] = 1
    pred[6:10, 2:6, 8:13] = 2
    gt[7:11, 8:12, 3:9] = 4
    pred[6:11, 7:12, 4:9] = 4
    out["absent"] = (pred, gt, SPACING_ANISO, 5)
    gt = z()
    gt[3:9, 4:11, 5:12] = 1
    gt[5, 6, 7] = 0                                                                                  # a cavity
    out["identical"] = (gt.copy(), gt, SPACING_ANISO, 2)
    gt, pred = z(), z()
    gt[5, 5, 5] = 1
    pred[7, 6, 5] = 1
    out["single_voxel"] = (pred, gt, SPACING_ANISO, 2)
    gt, pred = z(), z()
    gt[0:4, 0:5, 0:3] = 1                                                                            # low faces
    pred[0:5, 0:4, 0:4] = 1
    gt[8:12, 9:14, 11:16] = 2                                                                        # high faces
    pred[9:12, 10:14, 10:16] = 2
    out["faces"] = (pred, gt, SPACING_ANISO, 3)
    gt, pred = z(), z()
    gt[1:4, 1:5, 1:5] = 1
    gt[8:11, 9:13, 10:15] = 1
    pred[1:5, 2:5, 1:4] = 1
    pred[7:11, 9:12, 11:15] = 1
    out["two_components"] = (pred, gt, SPACING_ANISO, 2)
    pred, gt = ellipsoid_pair((16, 16, 16), 3, 2102)
    out["iso"] = (pred, gt, (1.0, 1.0, 1.0), 3)
    return out


def all_small_cases():
    """fixture key -> (pred, gt, spacing, classes) for case A and every edge case of B."""
    cases = {"A": ellipsoid_pair(CASE_A["shape"], CASE_A["classes"], CASE_A["seed"]) + (CASE_A["spacing"], CASE_A["classes"])}
    cases.update({"B_" + k: v for k, v in edge_cases().items()})
    return cases


# ---- comparisons ------------------------------------------------------------------------------------------------------

def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, got, ref)
    assert np.array_equal(np.isinf(got), np.isinf(ref)), (what, got, ref)
    fin = np.isfinite(ref)
    if fin.any():
        err = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), 1e-300)
        err = np.where(got[fin] == ref[fin], 0.0, err)
        print(f"  {what}: {int(fin.sum())} finite values, largest relative difference {float(err.max()):.3e}")
        assert float(err.max()) <= RTOL, (what, float(err.max()))


def _spacing(g, key):
    return torch.from_numpy(g[key + "_spacing"])          # float32, as the reference's datasets deliver it


def _inputs(dev, pred, gt):
    return torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)


def check_lists(dev):
    """Check 1: per class both lists have the fixture's length, the same multiset of areas (exact) and the same sorted distances."""
    from cbim_amd.metric.surface import surface_distances
    g = load_golden("surface_small")
    for key, (pred, gt, _, classes) in all_small_cases().items():
        assert labels_crc(pred, gt) == int(g[key + "_crc"]), key
        table = g[key + "_table"]
        lists = surface_distances(*_inputs(dev, pred, gt), _spacing(g, key), classes)
        assert len(lists) == classes - 1
        for c in range(1, classes):
            for side, other in (("gt", "pred"), ("pred", "gt")):
                d = lists[c - 1][f"distances_{side}_to_{other}"]
                codes = lists[c - 1][f"codes_{side}"]
                rd, ra = g[f"{key}_c{c}_d_{side}"], g[f"{key}_c{c}_a_{side}"]
                assert d.dtype == np.float64 and len(d) == len(codes) == len(rd), (key, c, side, len(d), len(rd))
                assert np.array_equal(np.sort(table[codes]), np.sort(ra)), (key, c, side)
                _close(np.sort(d), rd, f"{key} class {c} {side}->{other}")


def check_metrics(dev):
    """Check 2: ASD / HD at percentage 95, 50 and 100 for every small case."""
    from cbim_amd.metric.utils import calculate_distance
    g = load_golden("surface_small")
    for key, (pred, gt, _, classes) in all_small_cases().items():
        p, t = _inputs(dev, pred, gt)
        for pct in PERCENTAGES:
            asd, hd = calculate_distance(p, t, _spacing(g, key), classes, pct, area_table=g[key + "_table"])
            assert asd.dtype == np.float64 and asd.shape == hd.shape == (classes - 1,)
            _close(asd, g[f"{key}_ASD"], f"{key} ASD")
            _close(hd, g[f"{key}_HD{pct}"], f"{key} HD{pct}")
    asd, hd = calculate_distance(p, t, _spacing(g, key), classes, area_table=g[key + "_table"])          # default percentage
    _close(hd, g[f"{key}_HD95"], f"{key} HD default")


def check_large(dev):
    """Case C (128^3, 16 classes): metrics, list lengths, sums and a strided sample of the sorted lists."""
    from cbim_amd.metric.surface import surface_distances
    from cbim_amd.metric.utils import calculate_distance
    g = load_golden("surface_large")
    pred, gt = ellipsoid_pair(CASE_C["shape"], CASE_C["classes"], CASE_C["seed"])
    assert labels_crc(pred, gt) == int(g["crc"])
    p, t = _inputs(dev, pred, gt)
    sp, table, classes = torch.from_numpy(g["spacing"]), g["table"], CASE_C["classes"]
    asd, hd = calculate_distance(p, t, sp, classes, area_table=table)
    _close(asd, g["ASD"], "C ASD")
    _close(hd, g["HD95"], "C HD95")
    lists = surface_distances(p, t, sp, classes)
    stride = int(g["stride"])
    for c in range(1, classes):
        for k, (side, other) in enumerate((("gt", "pred"), ("pred", "gt"))):
            d = np.sort(lists[c - 1][f"distances_{side}_to_{other}"])
            a = np.sort(table[lists[c - 1][f"codes_{side}"]])
            assert len(d) == int(g["lengths"][c - 1, k]), (c, side)
            _close(d[::stride], g[f"c{c}_d_{side}"], f"C class {c} {side}->{other} sample")
            assert np.array_equal(a[::stride], g[f"c{c}_a_{side}"]), (c, side)
            fin = np.isfinite(d)
            _close([d[fin].sum(), a.sum()], g["sums"][c - 1, k], f"C class {c} {side} sums")


def check_table_seam(dev):
    """Check 3: the table as an array and as a callable agree; without a table and without the host project: ImportError."""
    import sys
    from cbim_amd.metric.utils import calculate_distance
    g = load_golden("surface_small")
    pred, gt, _, classes = all_small_cases()["A"]
    p, t = _inputs(dev, pred, gt)
    sp, table = _spacing(g, "A"), g["A_table"]
    seen = []

    def make(spacing):
        seen.append(np.asarray(spacing))
        return table.copy()
    a1, h1 = calculate_distance(p, t, sp, classes, area_table=table)
    a2, h2 = calculate_distance(p, t, sp, classes, area_table=make)
    assert np.array_equal(a1, a2) and np.array_equal(h1, h2)
    assert len(seen) == 1 and seen[0].dtype == np.float32 and np.array_equal(seen[0], g["A_spacing"])

    class _NoHostProject:                  # whatever else this process has put on sys.path: `metric` is not importable here
        @staticmethod
        def find_spec(name, path=None, target=None):
            if name == "metric" or name.startswith("metric."):
                raise ImportError("blocked for this check: " + name)
    hidden = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "metric" or k.startswith("metric.")}
    sys.meta_path.insert(0, _NoHostProject)
    try:
        calculate_distance(p, t, sp, classes)
    except ImportError as e:
        assert "area_table=" in str(e), str(e)
    else:
        raise AssertionError("calculate_distance without a table and without metric.lookup_tables must raise ImportError")
    finally:
        sys.meta_path.remove(_NoHostProject)
        sys.modules.update(hidden)
    try:
        calculate_distance(p, t, sp, classes, area_table=table[:16])
    except ValueError:
        pass
    else:
        raise AssertionError("a 16-entry table must be refused")


def check_input_forms(dev):
    """Check 4: int8 / int64, device / host tensors, spacing as float32 tensor or list give the same numbers; 2-D is refused."""
    from cbim_amd.metric.utils import calculate_distance
    g = load_golden("surface_small")
    pred, gt, spacing, classes = all_small_cases()["B_faces"]
    table = g["B_faces_table"]
    p8, t8 = torch.from_numpy(pred), torch.from_numpy(gt)
    ref = calculate_distance(p8.to(dev), t8.to(dev), _spacing(g, "B_faces"), classes, area_table=table)
    forms = [(p8.long().to(dev), t8.long().to(dev), _spacing(g, "B_faces")),
             (p8.to(dev), t8.long().to(dev), list(spacing)),
             (p8, t8, list(spacing)),                                    # host tensors
             (p8.long(), t8, _spacing(g, "B_faces").to(dev)),
             (p8.to(dev).to(torch.int32), t8.to(dev), tuple(spacing))]   # any other integer dtype is widened
    for a, b, s in forms:
        got = calculate_distance(a, b, s, classes, area_table=table)
        assert np.array_equal(got[0], ref[0], equal_nan=True) and np.array_equal(got[1], ref[1], equal_nan=True)
    _close(ref[0], g["B_faces_ASD"], "faces ASD")
    for bad in ((p8[0].to(dev), t8[0].to(dev), list(spacing)[:2]), (p8[0].to(dev), t8[0].to(dev), list(spacing))):
        try:
            calculate_distance(*bad, classes, area_table=table)
        except NotImplementedError:
            pass
        else:
            raise AssertionError("2-D input must raise NotImplementedError")


# ---- validation loop --------------------------------------------------------------------------------------------------------

VAL_SHAPE = (40, 48, 40)
TINY_SHAPE = (4, 16, 16)


def tiny_net(dev):
    """A narrow ResUNet for the host-side executor, where a 32^3 forward of the base-8 net takes half a minute."""
    from cbim_amd.model.dim3 import UNet
    from tests.infer_checks import CLASSES
    torch.manual_seed(9)
    return UNet(1, 4, scale=[[1, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=CLASSES, block="BasicBlock", norm="in").to(dev)


def val_loader(n=2, shape=VAL_SHAPE):
    """[(image [1,1,D,H,W], label [1,1,D,H,W] int8, spacing [1,3])] — blocky labels; class 2 is missing from volume 1's labels."""
    from tests.infer_checks import CLASSES
    D, H, W = shape
    items = []
    for k in range(n):
        gen = torch.Generator().manual_seed(7100 + k)
        img = torch.randn((1, 1) + tuple(shape), generator=gen)
        lab = torch.zeros((1, 1) + tuple(shape), dtype=torch.int8)
        lab[..., D * 3 // 20 + (2 * k if D >= 20 else 0):D * 11 // 20, H // 6:H * 5 // 8, W // 8:W * 21 // 40] = 1
        if k != 1:
            lab[..., D // 2:D * 9 // 10, H // 2:H * 11 // 12 - k, W * 9 // 20:W * 9 // 10] = CLASSES - 1
        items.append((img, lab, torch.tensor([[2.5, 0.8, 1.25]])))
    return items


def val_args(**kw):
    from tests.infer_checks import CLASSES, WINDOW
    a = argparse.Namespace(window_size=WINDOW, classes=CLASSES, dimension="3d", sliding_window=True, distributed=False, proc_idx=0)
    a.__dict__.update(kw)
    return a


def expected_validation(net, items, args, table, dev):
    """The reference's bookkeeping (validation.py:54-85) written out on label maps obtained independently of validation()."""
    from cbim_amd.inference.utils import get_inference
    from cbim_amd.metric.utils import calculate_dice_split, calculate_distance
    n = args.classes - 1
    dice, asd, hd = ([[] for _ in range(n)] for _ in range(3))
    for img, lab, sp in items:
        prob = get_inference(args)(net, img.float().to(dev), args)
        lp = prob.argmax(1).squeeze(0)
        lt = lab.to(dev).squeeze(0).squeeze(0)
        a, h = calculate_distance(lp, lt, sp[0], args.classes, area_table=table)
        a, h = np.clip(np.nan_to_num(a, nan=500), 0, 500), np.clip(np.nan_to_num(h, nan=500), 0, 500)
        d = calculate_dice_split(lp.reshape(-1, 1), lt.reshape(-1, 1), args.classes)[0].cpu().numpy()[1:]
        for c in range(n):
            if bool((lt == c + 1).any()):
                dice[c].append(d[c]); asd[c].append(a[c]); hd[c].append(h[c])
    return tuple(np.array([np.array(v).mean() for v in m]) for m in (dice, asd, hd))


def check_validation(dev, whole_image=False, tiny=False):
    """Check 5: validation() / validation_ddp(distributed=False) against the bookkeeping above.  tiny: the narrow net on
    4x16x16 volumes (whole-image only) — what the host-side executor can afford."""
    import cbim_amd
    from cbim_amd.training.validation import validation, validation_ddp
    from tests.infer_checks import CLASSES, _net
    net = tiny_net(dev) if tiny else _net(dev)[0]
    g = load_golden("surface_small")
    table = lambda spacing: g["A_table"]                       # noqa: E731  (same spacing as case A)
    items = val_loader(2, TINY_SHAPE if tiny else VAL_SHAPE)
    if whole_image and not tiny:
        items = [(i[..., :32, :32, :32].contiguous(), l[..., :32, :32, :32].contiguous(), s) for i, l, s in items]
    args = val_args(sliding_window=not whole_image, area_table=table)
    cbim_amd.set_compute_dtype("fp32")
    try:
        want = expected_validation(net, items, args, table, dev)
        got = validation(net, items, args)
        got_ddp = validation_ddp(net, items, args)
    finally:
        cbim_amd.set_compute_dtype(None)
    for w, a, b, name in zip(want, got, got_ddp, ("dice", "ASD", "HD")):
        assert isinstance(a, np.ndarray) and a.shape == (CLASSES - 1,), (name, a)
        print(f"  validation {name}: {a}")
        assert np.array_equal(a, w, equal_nan=True), (name, a, w)
        assert np.array_equal(a, b, equal_nan=True), (name, a, b)
    assert np.all(np.isfinite(got[0])) and np.all(got[1] <= 500) and np.all(got[2] <= 500)
