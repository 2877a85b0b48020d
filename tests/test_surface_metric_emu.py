"""CPU suite: the surface-distance kernels (csrc/surface_kernels.hip) on the host-side executor, ``calculate_distance`` and the
validation loop, against fixtures the real reference wrote (tests/golden/make_golden_surface.py)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import surface_checks as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = os.environ.get("CBIM_REFERENCE", "/root/reference")


@pytest.fixture(autouse=True)
def _emu_only(dev):
    if dev != "cpu":
        pytest.skip("CPU suite (the -m gpu twin is tests/test_gpu_surface_metric.py)")


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


def test_default_table_comes_from_the_host_project():
    """The default path (no area_table=) in a fresh process with the reference checkout on sys.path as the host project."""
    if not os.path.isfile(os.path.join(REFERENCE, "metric", "lookup_tables.py")):
        pytest.skip("no reference checkout on this machine")
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path[:0] = [{ROOT!r}, {REFERENCE!r}]\n"
        "np.Inf, np.NaN = np.inf, np.nan          # numpy 2: the reference's metric/metrics.py still names them\n"
        "from tests import surface_checks as sc\n"
        "from tests.util import load_golden\n"
        "from cbim_amd.metric.utils import calculate_distance\n"
        "g = load_golden('surface_small')\n"
        "pred, gt, _, classes = sc.all_small_cases()['A']\n"
        "asd, hd = calculate_distance(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(g['A_spacing']), classes)\n"
        "sc._close(asd, g['A_ASD'], 'A ASD'); sc._close(hd, g['A_HD95'], 'A HD95')\n"
        "print('DEFAULT-TABLE-OK')\n")
    env = dict(os.environ)
    assert env.get("CBIM_HIP_LIBRARY"), "CPU suite: the host-side executor library is set by tests/conftest.py"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert "DEFAULT-TABLE-OK" in r.stdout, r.stdout + r.stderr


def test_validation_loop(dev):
    """The narrow net, whole-image inference: a 32^3 forward of the fixtures' base-8 net takes half a minute on the host-side
    executor, the sliding-window loop over it half an hour — that pair runs in the -m gpu twin."""
    sc.check_validation(dev, whole_image=True, tiny=True)


# ---- validation_ddp, world 2 (gloo): the gather and the removal of the sampler's padded sample -------------------------------

class _Loader(list):
    """A list "dataloader" with the .dataset the padded-sample removal reads (validation.py:177)."""
    def __init__(self, items, dataset_len):
        super().__init__(items)
        self.dataset = range(dataset_len)


def _ddp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import cbim_amd
    from cbim_amd.training.validation import validation_ddp
    from tests.util import load_golden
    table = load_golden("surface_small")["A_table"]
    net = sc.tiny_net("cpu")
    items = sc.val_loader(3, sc.TINY_SHAPE)
    # DistributedSampler(shuffle=False) over 3 volumes, world 2: rank 0 -> [0, 2], rank 1 -> [1, 0 (the padded wrap-around)]
    mine = [items[0], items[2]] if rank == 0 else [items[1], items[0]]
    args = sc.val_args(distributed=True, sliding_window=False, area_table=table, proc_idx=rank)
    cbim_amd.set_compute_dtype("fp32")
    out = validation_ddp(net, _Loader(mine, 3), args)
    q.put((rank, [np.asarray(o) for o in out]))
    dist.barrier()
    dist.destroy_process_group()


def test_validation_ddp_gathers_and_drops_the_padded_sample():
    import torch.multiprocessing as mp
    import cbim_amd
    from cbim_amd.training.validation import validation
    from tests.util import load_golden
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=1500) for _ in range(2))
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    net = sc.tiny_net("cpu")
    args = sc.val_args(sliding_window=False, area_table=load_golden("surface_small")["A_table"])
    cbim_amd.set_compute_dtype("fp32")
    try:
        want = validation(net, sc.val_loader(3, sc.TINY_SHAPE), args)              # the three volumes, each exactly once
    finally:
        cbim_amd.set_compute_dtype(None)
    for a, b, w in zip(got[0], got[1], want):
        assert np.array_equal(a, b, equal_nan=True)
        assert np.allclose(a, w, rtol=1e-6, atol=0), (a, w)         # same samples, averaged in gather order [0, 1, 2]


# ---- optional: a randomised property test against a scipy restatement (pinned to the fixtures first) -------------------------

def _scipy_lists(pred, gt, spacing):
    """compute_surface_distances restated on scipy (codes instead of areas): (d_gt, codes_gt, d_pred, codes_pred), unsorted."""
    from scipy import ndimage
    union = np.argwhere(gt | pred)
    if len(union) == 0:
        return (np.zeros(0),) * 4
    lo, hi = union.min(0), union.max(0)
    kernel = np.array([[[128, 64], [32, 16]], [[8, 4], [2, 1]]])
    out = []
    crops = []
    for m in (gt, pred):
        crop = np.zeros(hi - lo + 2, np.uint8)
        crop[:-1, :-1, :-1] = m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]
        code = ndimage.correlate(crop, kernel.astype(np.uint8), mode="constant", cval=0)
        crops.append((code, (code != 0) & (code != 255)))
    for (code, border), (_, other) in ((crops[0], crops[1]), (crops[1], crops[0])):
        dm = ndimage.distance_transform_edt(~other, sampling=spacing) if other.any() else np.full(other.shape, np.inf)
        out += [dm[border], code[border]]
    return tuple(out)


def test_random_masks_against_scipy_restatement(dev):
    pytest.importorskip("scipy")
    from cbim_amd.metric.surface import surface_distances
    from tests.util import load_golden
    g = load_golden("surface_small")
    # pin the restatement to the reference's own output first
    pred, gt, spacing, classes = sc.all_small_cases()["B_faces"]
    sp = g["B_faces_spacing"].astype(np.float64)
    for c in range(1, classes):
        d_gt, c_gt, d_pred, c_pred = _scipy_lists(pred == c, gt == c, sp)
        assert np.array_equal(np.sort(d_gt), g[f"B_faces_c{c}_d_gt"]) and np.array_equal(np.sort(d_pred), g[f"B_faces_c{c}_d_pred"])
        assert np.array_equal(np.sort(g["B_faces_table"][c_gt]), np.sort(g[f"B_faces_c{c}_a_gt"]))
    rng = np.random.default_rng(31)
    for trial in range(6):
        shape = tuple(int(v) for v in rng.integers(3, 40, 3))
        classes = int(rng.integers(2, 5))
        sp32 = rng.uniform(0.4, 3.0, 3).astype(np.float32)
        coarse = rng.integers(0, classes, [(n + 3) // 4 for n in shape])
        gt = np.kron(coarse, np.ones((4, 4, 4), np.int64))[:shape[0], :shape[1], :shape[2]].astype(np.int8)
        pred = gt.copy()
        flip = rng.random(shape) < 0.03
        pred[flip] = rng.integers(0, classes, int(flip.sum()))
        lists = surface_distances(torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(sp32), classes)
        for c in range(1, classes):
            ref = _scipy_lists(pred == c, gt == c, sp32.astype(np.float64))
            for k, key in enumerate(("distances_gt_to_pred", "codes_gt", "distances_pred_to_gt", "codes_pred")):
                got = np.sort(lists[c - 1][key])
                assert len(got) == len(ref[k]), (trial, c, key)
                if k % 2:
                    assert np.array_equal(got, np.sort(ref[k])), (trial, c, key)
                else:
                    sc._close(got, np.sort(ref[k]), f"trial {trial} class {c} {key}")
