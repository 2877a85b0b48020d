"""The channel-slice view contract of the kernel entry points (cbim_amd.ops), shared by the executor suite and the GPU suite.

A 5-D channels-last operand reaches a kernel either as a contiguous tensor or as a "row view": a channel range
``wide[..., a:b]`` of a wider contiguous tensor.  Only the entry points that hand the row stride to the library may take a row
view (``ops._view_ok`` / ``ops._rows_ok``); every other one reads its pointer as dense memory and must refuse the view in
Python (``ops._dev_ok``).  CONTRACT below is the table of both kinds; the checks are

  check_contract_complete   every public callable of ops is in CONTRACT or in EXCLUDED (with a reason)
  check_strided_slot        view against dense with a NaN-poisoned parent: same bits, nothing written beside the view
  check_conv_family         the same for every convolution kernel family and operand slot, with the kernel that ran asserted
  check_dense_slot          a view in a dense-only slot raises before the library is reached (the library is patched out)
  check_misaligned          views the 16-byte chunks of the kernels cannot address raise before the library is reached
  check_autograd            the autograd Functions give the same outputs and gradients on a view as on its contiguous copy
"""
import contextlib
import inspect

import pytest
import torch
import torch.nn.functional as F

from cbim_amd import _lib, ops
from cbim_amd import functional as Fn

F32, BF16 = torch.float32, torch.bfloat16
WHERE = ("lead", "mid", "trail")       # the view starts at channel 0, one chunk in, or ends with the parent

S, D = "strided", "dense-only"

# every public ops function with a 5-D (channels-last or NCDHW) or row-matrix tensor operand -> {operand: kind}
CONTRACT = {
    "instnorm_stats": {"x": S},
    "norm_act_fwd": {"x": S},
    "norm_bwd_sums": {"g": S, "x": S},
    "norm_bwd_apply": {"g": S, "x": S, "add": S},
    "norm_affine_act_fwd": {"x": S},
    "norm_affine_bwd_sums": {"g": S, "x": S},
    "norm_affine_bwd_apply": {"g": S, "x": S},
    "resnorm_fwd": {"a": S, "b": S},
    "resnorm_bwd": {"dy": S, "a": S, "b": S},
    "conv_igemm": {"x": S, "x2": S, "res": S, "mask_x": S, "out": S},
    "conv_fwd": {"x": S, "res": S},
    "conv_dgrad": {"dy": S, "dy2": S, "mask_x": S, "accumulate": S},
    "conv_wgrad": {"x": S, "x2": S, "dy": S, "dy2": S},
    "dwconv": {"x": S},
    "dwconv_wgrad": {"x": S, "dy": S},
    "bidir_attn_fwd": {"qv": S},
    "bidir_attn_bwd": {"qv": S, "dfo": D},
    "bidir_attn_gemm_fwd": {"qv": S},                 # (reshaped into token rows: a view is copied, a dense tensor is not)
    "bidir_attn_gemm_bwd": {"qv": S, "dfo": S},
    "colsoftmax_pool_fwd": {"fw": S},
    "colsoftmax_pool_bwd": {"fw": S},
    "space_to_depth_from": {"g": S},
    "depth_to_space_into": {"t": D, "out": S},
    "token_linear": {"x2d": S, "res": S, "mask": S, "out": S},
    "token_linear_wgrad": {"x2d": S, "dy2d": S},
    "maxpool_fwd": {"x": D},
    "maxpool_bwd": {"dy": D, "idx": D},
    "upcat_fwd": {"low": D, "skip": D},
    "upcat_fwd_stats": {"low": D, "skip": D},
    "up_stats": {"low": D},
    "upcat_act_fwd": {"low": D, "skip": D},
    "upcat_norm_bwd": {"g": D, "low": D, "skip": D},
    "upcat_bwd": {"dout": D},
    "stem_fwd": {"x_ncdhw": D},
    "stem_wgrad": {"x_ncdhw": D, "dy": D},
    "head_fwd": {"x": D},
    "head_bwd": {"x": D, "dlogits": D},
    "dice_ce_fwd": {"logits": D, "labels": D},
    "dice_ce_bwd": {"logits": D, "labels": D},
    "focal_fwd": {"logits": D, "labels": D},
    "focal_bwd": {"logits": D, "labels": D},
    "topk_fwd": {"logits": D, "labels": D},
    "topk_bwd": {"logits": D, "labels": D},
    "ncdhw_to_ndhwc": {"x": D},
    "ndhwc_to_ncdhw": {"x": D},
    "space_to_depth": {"x": D},
    "depth_to_space": {"dy": D},
    "trilinear_planes_fwd": {"x": D},
    "trilinear_planes_bwd": {"dy": D},
    "window_attn_fwd": {"qkv": D},
    "window_attn_bwd": {"qkv": D, "out": D, "dout": D},
    "layernorm_fwd": {"x": D},
    "layernorm_bwd": {"dy": D, "x": D, "add": D},
    "gate_fwd": {"x": D},
    "gate_bwd": {"dy": D, "x": D},
    "colsum": {"x2d": D},
    "awg_rows": {"S": D},
    "awg_cols": {"S": D},
    "awg_ds": {"dP": D, "P": D, "dC": D, "Cs": D},
    "map_gemm": {"A": D, "X": D, "OUT": D},
    "pack_weights": {"w": D},
    "pack_weights_both": {"w": D},
    "lo_weights": {"w": D},
}

# operands that are row matrices [rows, C]: their test view is a column range of a wider matrix
ROW_OPERANDS = {("token_linear", s) for s in CONTRACT["token_linear"]} | {("token_linear_wgrad", s) for s in CONTRACT["token_linear_wgrad"]} | \
    {("colsum", "x2d"), ("awg_rows", "S"), ("awg_cols", "S"), ("map_gemm", "A"), ("map_gemm", "X"), ("map_gemm", "OUT")} | \
    {("awg_ds", s) for s in CONTRACT["awg_ds"]}

EXCLUDED = {
    "ConvGeom": "geometry helper: holds descriptors, takes no tensor",
    "PackedWeights": "weight packer cache: packs contiguous parameters through pack_weights' library calls",
    "packed_weights": "weight packer: makes its weights contiguous before packing",
    "rw48_takes": "geometry helper: asks the library about a descriptor, takes no tensor",
    "slot_of": "gradient-slot plumbing: reads an attribute of a parameter",
    "grad_slot": "gradient-slot plumbing: no kernel",
    "grad_slot_pair": "gradient-slot plumbing: no kernel",
    "linear_geom": "geometry helper: descriptor of a token Linear, takes no tensor",
    "dwconv_wgrad_on_matrix_cores": "switch query: shape and dtype only",
    "awg_eligible": "switch query: shape and dtype only",
    "as_rows": "layout helper: returns the tensor where _view_ok admits it, else a contiguous copy; no kernel",
    "up_adjoint": "called on tensors the up-path entry points allocate themselves; its row stride and channel offset are arguments",
    "stats_finalize": "per-(n, c) partial records [N, P, C, 3] allocated by the calling entry point: no activation operand",
    "stats_restat": "per-(n, c) statistics [N, C, 2]: no activation operand",
    "se_fold_fwd": "per-(n, c) statistics and gates: no activation operand",
    "se_fold_bwd": "per-(n, c) sums and gates: no activation operand",
    "bn_finish_fwd": "per-channel vectors and per-(n, c) statistics: no activation operand",
    "bn_finish_bwd": "per-channel vectors and per-(n, c) sums: no activation operand",
    "map_qv_fwd": "semantic-map matrices [B, C, M] through map_gemm, which takes contiguous float32 tensors only",
    "map_qv_bwd": "semantic-map matrices through map_gemm (contiguous float32 only)",
    "map_out_fwd": "semantic-map matrices through map_gemm (contiguous float32 only)",
    "map_out_bwd": "semantic-map matrices through map_gemm (contiguous float32 only)",
    "se_gate_fwd": "channel means [N, C] and Linear weights: asserts contiguous float32 itself",
    "se_gate_bwd": "channel means [N, C] and Linear weights: contiguous float32 only",
}


def public_callables():
    return sorted(n for n, o in vars(ops).items()
                  if not n.startswith("_") and callable(o) and getattr(o, "__module__", None) == ops.__name__)


def check_contract_complete():
    names = public_callables()
    missing = [n for n in names if n not in CONTRACT and n not in EXCLUDED]
    assert not missing, f"ops callables without a view contract (add them to CONTRACT or EXCLUDED): {missing}"
    stale = [n for n in list(CONTRACT) + list(EXCLUDED) if n not in names]
    assert not stale, f"contract rows without an ops callable: {stale}"
    assert not set(CONTRACT) & set(EXCLUDED)
    for n, slots in CONTRACT.items():
        params = inspect.signature(getattr(ops, n)).parameters
        bad = [s for s in slots if s not in params]
        assert not bad, f"ops.{n} has no operand named {bad}"
        assert all(k in (S, D) for k in slots.values())
    assert all(r.strip() for r in EXCLUDED.values())
    # what the table rests on: the plain guard admits contiguous tensors only, the opt-in forms admit an aligned channel range
    dev = "cpu" if _lib.backend() == "emu" else "cuda"
    v5, v2 = _view5(dev), _view2(dev)
    for t in (v5, v2):
        with pytest.raises(RuntimeError, match="non-contiguous"):
            ops._dev_ok(t)
    ops._view_ok(v5, v5.contiguous(), None)
    ops._rows_ok(v2, v2.contiguous(), None)
    with pytest.raises(RuntimeError, match="non-contiguous"):
        ops._view_ok(v5.transpose(1, 2))


# ------------------------------------------------------------------------------------------------
# views
# ------------------------------------------------------------------------------------------------

def chunk(dtype):
    return 16 // torch.empty(0, dtype=dtype).element_size()


def poisoned_view(dense, where):
    """(view, parent): `dense` [..., C] as a channel range of a parent two 16-byte chunks wider whose other channels are NaN"""
    ch = chunk(dense.dtype)
    Cc = int(dense.shape[-1])
    off = {"lead": 0, "mid": ch, "trail": 2 * ch}[where]
    parent = torch.full(tuple(dense.shape[:-1]) + (Cc + 2 * ch,), float("nan"), dtype=dense.dtype, device=dense.device)
    parent[..., off:off + Cc] = dense
    v = parent[..., off:off + Cc]
    assert not v.is_contiguous() and v.data_ptr() % 16 == 0
    return v, parent


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def untouched_outside(parent, view, what):
    """the channels of `parent` beside `view` still hold the NaN pattern they were filled with, bit for bit"""
    off = (view.data_ptr() - parent.data_ptr()) // parent.element_size()
    Cc = int(view.shape[-1])
    ref = torch.full((1,), float("nan"), dtype=parent.dtype, device=parent.device)
    for lo, hi in ((0, off), (off + Cc, int(parent.shape[-1]))):
        if hi > lo:
            got = bits(parent[..., lo:hi])
            assert bool((got == bits(ref)).all()), f"{what}: channels [{lo}, {hi}) of the parent were written"


def same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} vs {b.shape} {b.dtype}"
    assert bool(torch.isfinite(a.float()).all()), f"{what}: non-finite output on the view (poison was read)"
    assert torch.equal(a, b), f"{what}: view and dense differ, max abs {float((a.float() - b.float()).abs().max()):.3e}"


def rnd(shape, dtype, dev, seed, shift=0.0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(dtype).to(dev)


# ------------------------------------------------------------------------------------------------
# (b) strided slots: one case per entry point (or kernel path of it).  A case is
#   (ops function name, dtypes, build(dev, dtype) -> (call(**operands) -> outputs, operands {slot: dense tensor}, written {slot}))
# `written` slots are outputs handed in by the caller: their parent must stay untouched beside the view.
# ------------------------------------------------------------------------------------------------

_N, _DHW, _C = 2, (5, 6, 7), 24
ACT = ops.ACT


def _act5(dev, dtype, seed, C=_C, dhw=_DHW, N=_N, shift=0.3):
    return rnd((N,) + tuple(dhw) + (C,), dtype, dev, seed, shift)


def _case_instnorm(dev, dtype):
    return (lambda x: (ops.instnorm_stats(x),)), {"x": _act5(dev, dtype, 1)}, ()


def _case_norm_act(dev, dtype):
    x = _act5(dev, dtype, 2)
    st = ops.instnorm_stats(x)
    return (lambda x: (ops.norm_act_fwd(x, st, ACT["relu"]),)), {"x": x}, ()


def _case_norm_bwd_sums(dev, dtype):
    x, g = _act5(dev, dtype, 3), _act5(dev, dtype, 4, shift=0.0)
    st = ops.instnorm_stats(x)
    return (lambda g, x: (ops.norm_bwd_sums(g, x, st, ACT["relu"], True),)), {"g": g, "x": x}, ()


def _case_norm_bwd_apply(dev, dtype):
    x, g, add = _act5(dev, dtype, 5), _act5(dev, dtype, 6, shift=0.0), _act5(dev, dtype, 7, shift=0.0)
    st = ops.instnorm_stats(x)
    sums = ops.norm_bwd_sums(g, x, st, ACT["relu"], True)
    return (lambda g, x, add: (ops.norm_bwd_apply(g, x, st, sums, ACT["relu"], True, add=add),)), {"g": g, "x": x, "add": add}, ()


def _affine(dev):
    return torch.stack([torch.linspace(0.5, 1.5, _C), torch.linspace(-0.3, 0.3, _C)], 1).contiguous().to(dev)


def _case_affine_fwd(dev, dtype):
    x = _act5(dev, dtype, 8)
    st, af = ops.instnorm_stats(x), _affine(dev)
    return (lambda x: (ops.norm_affine_act_fwd(x, st, af, ACT["elu"]),)), {"x": x}, ()


def _case_affine_sums(dev, dtype):
    x, g = _act5(dev, dtype, 9), _act5(dev, dtype, 10, shift=0.0)
    st, af = ops.instnorm_stats(x), _affine(dev)
    return (lambda g, x: (ops.norm_affine_bwd_sums(g, x, st, af, ACT["elu"], True),)), {"g": g, "x": x}, ()


def _case_affine_apply(dev, dtype):
    x, g = _act5(dev, dtype, 11), _act5(dev, dtype, 12, shift=0.0)
    st, af = ops.instnorm_stats(x), _affine(dev)
    sums = ops.norm_affine_bwd_sums(g, x, st, af, ACT["elu"], True)
    return (lambda g, x: (ops.norm_affine_bwd_apply(g, x, st, af, sums, ACT["elu"], True),)), {"g": g, "x": x}, ()


def _case_resnorm_fwd(dev, dtype):
    a, b = _act5(dev, dtype, 13), _act5(dev, dtype, 14)
    sa, sb = ops.instnorm_stats(a), ops.instnorm_stats(b)
    return (lambda a, b: (ops.resnorm_fwd(a, sa, b, sb, ACT["lrelu"]), ops.resnorm_fwd(a, sa, b, None, ACT["lrelu"]))), {"a": a, "b": b}, ()


def _case_resnorm_bwd(dev, dtype):
    a, b, dy = _act5(dev, dtype, 15), _act5(dev, dtype, 16), _act5(dev, dtype, 17, shift=0.0)
    sa, sb = ops.instnorm_stats(a), ops.instnorm_stats(b)
    return (lambda dy, a, b: ops.resnorm_bwd(dy, a, sa, b, sb, ACT["lrelu"]) + ops.resnorm_bwd(dy, a, sa, b, None, ACT["lrelu"])), \
        {"dy": dy, "a": a, "b": b}, ()


def _case_dwconv(dev, dtype):
    x = _act5(dev, dtype, 18, C=16)
    w = rnd((16, 27), F32, dev, 19, scale=0.2)
    st = ops.instnorm_stats(x)
    return (lambda x: (ops.dwconv(x, w, (3, 3, 3)), ops.dwconv(x, w, (3, 3, 3), in_stats=st, act=ACT["relu"]))), {"x": x}, ()


def _case_dwconv_wgrad(dev, dtype):
    x, dy = _act5(dev, dtype, 20, C=16), _act5(dev, dtype, 21, C=16, shift=0.0)
    st = ops.instnorm_stats(x)
    return (lambda x, dy: (ops.dwconv_wgrad(x, None, 0, dy, (3, 3, 3)), ops.dwconv_wgrad(x, st, ACT["relu"], dy, (3, 3, 3)))), \
        {"x": x, "dy": dy}, ()


def _case_dwconv_wgrad_mfma(dev, dtype):
    x, dy = _act5(dev, dtype, 22, C=32, dhw=(8, 8, 9), N=1), _act5(dev, dtype, 23, C=32, dhw=(8, 8, 9), N=1, shift=0.0)
    assert ops.dwconv_wgrad_on_matrix_cores(x, (3, 3, 3))
    return (lambda x, dy: (ops.dwconv_wgrad(x, None, 0, dy, (3, 3, 3)),)), {"x": x, "dy": dy}, ()


_HEADS, _DH, _M = 2, 8, 8


def _attn_operands(dev, dtype):
    inner = _HEADS * _DH
    qv = _act5(dev, dtype, 24, C=2 * inner, shift=0.0)
    mq, mv = rnd((_N, _M, inner), F32, dev, 25), rnd((_N, _M, inner), F32, dev, 26)
    return qv, mq, mv, inner


def _case_attn_fwd(dev, dtype):
    qv, mq, mv, _ = _attn_operands(dev, dtype)
    return (lambda qv: ops.bidir_attn_fwd(qv, mq, mv, _HEADS, _DH ** -0.5)), {"qv": qv}, ()


def _case_attn_bwd(dev, dtype):
    qv, mq, mv, inner = _attn_operands(dev, dtype)
    fo, mo, cs = ops.bidir_attn_fwd(qv, mq, mv, _HEADS, _DH ** -0.5)
    dfo, dmo = _act5(dev, dtype, 27, C=inner, shift=0.0), rnd((_N, _M, inner), F32, dev, 28)
    return (lambda qv: ops.bidir_attn_bwd(qv, mq, mv, cs, mo, dfo, dmo, _HEADS, _DH ** -0.5)), {"qv": qv}, ()


def _gemm_attn_operands(dev):
    inner, M = 64, 64
    qv = _act5(dev, BF16, 29, C=2 * inner, dhw=(8, 8, 8), N=1, shift=0.0)
    mq, mv = rnd((1, M, inner), F32, dev, 30), rnd((1, M, inner), F32, dev, 31)
    return qv, mq, mv, inner, M


def _case_attn_gemm_fwd(dev, dtype):
    qv, mq, mv, inner, _ = _gemm_attn_operands(dev)
    return (lambda qv: ops.bidir_attn_gemm_fwd(qv, mq, mv, 1, inner ** -0.5)), {"qv": qv}, ()


def _case_attn_gemm_bwd(dev, dtype):
    qv, mq, mv, inner, M = _gemm_attn_operands(dev)
    fo, mo, P, Cs = ops.bidir_attn_gemm_fwd(qv, mq, mv, 1, inner ** -0.5)
    dfo, dmo = _act5(dev, BF16, 32, C=inner, dhw=(8, 8, 8), N=1, shift=0.0), rnd((1, M, inner), F32, dev, 33)
    return (lambda qv, dfo: ops.bidir_attn_gemm_bwd(qv, mq, mv, P, Cs, mo, dfo, dmo, 1, inner ** -0.5)), {"qv": qv, "dfo": dfo}, ()


def _case_mappool_fwd(dev, dtype):
    fw = _act5(dev, dtype, 34, C=_C + 8, shift=0.0)
    return (lambda fw: ops.colsoftmax_pool_fwd(fw, _C)), {"fw": fw}, ()


def _case_mappool_bwd(dev, dtype):
    fw = _act5(dev, dtype, 35, C=_C + 8, shift=0.0)
    mp, cs = ops.colsoftmax_pool_fwd(fw, _C)
    dmap = rnd((_N, _C, 8), F32, dev, 36)

    def call(fw):
        out = [ops.colsoftmax_pool_bwd(fw, _C, mp, cs, dmap)]          # the two library GEMMs (few voxels per image)
        old = ops.MAPPOOL_BWD_GEMM
        ops.MAPPOOL_BWD_GEMM = False
        try:
            out.append(ops.colsoftmax_pool_bwd(fw, _C, mp, cs, dmap))  # k_mappool_bwd
        finally:
            ops.MAPPOOL_BWD_GEMM = old
        return out
    return call, {"fw": fw}, ()


def _case_s2d_from(dev, dtype):
    g = _act5(dev, dtype, 37, C=16, dhw=(4, 6, 8))
    return (lambda g: (ops.space_to_depth_from(g, 8, (2, 2, 2)), ops.space_to_depth_from(g, 16, (2, 2, 2)))), {"g": g}, ()


def _case_d2s_into(dev, dtype):
    t = _act5(dev, dtype, 38, C=8 * 8, dhw=(2, 3, 4))
    out = _act5(dev, dtype, 39, C=16, dhw=(4, 6, 8))
    return (lambda out: (ops.depth_to_space_into(t, out, 8, (2, 2, 2)),)), {"out": out}, ("out",)


_ROWS, _CIN, _COUT = 77, 48, 144


def _lin_w(dev, seed=40):
    w = rnd((_COUT, _CIN), F32, dev, seed, scale=0.1)
    return ops.pack_weights(w.view(_COUT, _CIN, 1, 1, 1), ops.linear_geom(_CIN, _COUT), 0)


def _case_token_linear_res(dev, dtype):
    wp, bias = _lin_w(dev), rnd((_COUT,), F32, dev, 41)
    x, res, out = rnd((_ROWS, _CIN), dtype, dev, 42), rnd((_ROWS, _COUT), F32, dev, 43), rnd((_ROWS, _COUT), F32, dev, 44)
    return (lambda x2d, res, out: (ops.token_linear(x2d, wp, bias, _COUT, res=res, out_dtype=F32, out=out),)), \
        {"x2d": x, "res": res, "out": out}, ("out",)


def _case_token_linear_mask(dev, dtype):
    wp = _lin_w(dev, 45)
    x, mask, out = rnd((_ROWS, _CIN), dtype, dev, 46), rnd((_ROWS, _COUT), BF16, dev, 47), rnd((_ROWS, _COUT), BF16, dev, 48)
    act_in = ACT["gelu"] if dtype == BF16 else 0            # (the activation on load takes bf16 rows)
    return (lambda x2d, mask, out: (ops.token_linear(x2d, wp, None, _COUT, act_in=act_in, mask=mask, mask_act=ACT["gelu"], out=out),)), \
        {"x2d": x, "mask": mask, "out": out}, ("out",)


def _case_token_linear_wgrad(dev, dtype):
    x, dy = rnd((_ROWS, _CIN), dtype, dev, 49), rnd((_ROWS, _COUT), dtype, dev, 50)
    act_in = ACT["gelu"] if dtype == BF16 else 0
    return (lambda x2d, dy2d: (ops.token_linear_wgrad(x2d, dy2d), ops.token_linear_wgrad(x2d, dy2d, act_in=act_in))), \
        {"x2d": x, "dy2d": dy}, ()


BOTH = (F32, BF16)
STRIDED_CASES = {
    "instnorm_stats": ("instnorm_stats", BOTH, _case_instnorm),
    "norm_act_fwd": ("norm_act_fwd", BOTH, _case_norm_act),
    "norm_bwd_sums": ("norm_bwd_sums", BOTH, _case_norm_bwd_sums),
    "norm_bwd_apply": ("norm_bwd_apply", BOTH, _case_norm_bwd_apply),
    "norm_affine_act_fwd": ("norm_affine_act_fwd", BOTH, _case_affine_fwd),
    "norm_affine_bwd_sums": ("norm_affine_bwd_sums", BOTH, _case_affine_sums),
    "norm_affine_bwd_apply": ("norm_affine_bwd_apply", BOTH, _case_affine_apply),
    "resnorm_fwd": ("resnorm_fwd", BOTH, _case_resnorm_fwd),
    "resnorm_bwd": ("resnorm_bwd", BOTH, _case_resnorm_bwd),
    "dwconv": ("dwconv", BOTH, _case_dwconv),
    "dwconv_wgrad": ("dwconv_wgrad", BOTH, _case_dwconv_wgrad),
    "dwconv_wgrad[matrix cores]": ("dwconv_wgrad", (BF16,), _case_dwconv_wgrad_mfma),
    "bidir_attn_fwd": ("bidir_attn_fwd", BOTH, _case_attn_fwd),
    "bidir_attn_bwd": ("bidir_attn_bwd", BOTH, _case_attn_bwd),
    "bidir_attn_gemm_fwd": ("bidir_attn_gemm_fwd", (BF16,), _case_attn_gemm_fwd),
    "bidir_attn_gemm_bwd": ("bidir_attn_gemm_bwd", (BF16,), _case_attn_gemm_bwd),
    "colsoftmax_pool_fwd": ("colsoftmax_pool_fwd", BOTH, _case_mappool_fwd),
    "colsoftmax_pool_bwd": ("colsoftmax_pool_bwd", BOTH, _case_mappool_bwd),
    "space_to_depth_from": ("space_to_depth_from", BOTH, _case_s2d_from),
    "depth_to_space_into": ("depth_to_space_into", BOTH, _case_d2s_into),
    "token_linear[res]": ("token_linear", BOTH, _case_token_linear_res),
    "token_linear[mask]": ("token_linear", BOTH, _case_token_linear_mask),
    "token_linear_wgrad": ("token_linear_wgrad", BOTH, _case_token_linear_wgrad),
}
STRIDED_IDS = [(k, dt) for k, (_, dts, _) in STRIDED_CASES.items() for dt in dts]
CONV_ENTRIES = ("conv_igemm", "conv_fwd", "conv_dgrad", "conv_wgrad")     # their slots: check_conv_family


def check_strided_cases_cover_contract():
    """every strided slot of CONTRACT is exercised by a case of STRIDED_CASES or by the convolution families"""
    covered = set()
    for fn, _, build in STRIDED_CASES.values():
        covered |= {(fn, s) for s in _slots_of(build)}
    want = {(fn, s) for fn, slots in CONTRACT.items() for s, k in slots.items() if k == S and fn not in CONV_ENTRIES}
    assert want <= covered, f"strided slots without a view-against-dense case: {sorted(want - covered)}"
    assert covered <= want, f"cases for slots the contract does not mark strided: {sorted(covered - want)}"


def _slots_of(build):
    return _SLOTS[build]


# operand slots of every case, without building it (the builders launch kernels)
_SLOTS = {
    _case_instnorm: ("x",), _case_norm_act: ("x",), _case_norm_bwd_sums: ("g", "x"), _case_norm_bwd_apply: ("g", "x", "add"),
    _case_affine_fwd: ("x",), _case_affine_sums: ("g", "x"), _case_affine_apply: ("g", "x"), _case_resnorm_fwd: ("a", "b"),
    _case_resnorm_bwd: ("dy", "a", "b"), _case_dwconv: ("x",), _case_dwconv_wgrad: ("x", "dy"), _case_dwconv_wgrad_mfma: ("x", "dy"),
    _case_attn_fwd: ("qv",), _case_attn_bwd: ("qv",), _case_attn_gemm_fwd: ("qv",), _case_attn_gemm_bwd: ("qv", "dfo"),
    _case_mappool_fwd: ("fw",), _case_mappool_bwd: ("fw",), _case_s2d_from: ("g",), _case_d2s_into: ("out",),
    _case_token_linear_res: ("x2d", "res", "out"), _case_token_linear_mask: ("x2d", "mask", "out"),
    _case_token_linear_wgrad: ("x2d", "dy2d"),
}


def _run_on_views(call, operands, written, as_view, where_of, what):
    """call with the operands in `as_view` replaced by poisoned views; -> outputs, checked for untouched parents"""
    args, parents = {}, {}
    for s, t in operands.items():
        if s in as_view:
            args[s], parents[s] = poisoned_view(t, where_of[s])
        else:
            args[s] = t.clone() if s in written else t
    out = list(call(**args))
    for s in written:
        if s in parents:
            untouched_outside(parents[s], args[s], f"{what} [{s} @ {where_of[s]}]")
    for s in operands:               # inputs are never written
        if s in parents and s not in written:
            assert torch.equal(bits(args[s]), bits(operands[s])), f"{what}: input view {s} was modified"
    return out, args


def check_strided_slot(dev, case, dtype):
    fn, _, build = STRIDED_CASES[case]
    call, operands, written = build(dev, dtype)
    assert tuple(operands) == _SLOTS[build]
    assert all(CONTRACT[fn][s] == S for s in operands)
    ref, ref_args = _run_on_views(call, operands, written, (), {}, case)
    for t in ref:
        assert t is None or bool(torch.isfinite(t.float()).all()), f"{case}: the dense run is not finite"
    for s in operands:
        for where in WHERE:
            what = f"{case} {dtype} [{s} @ {where}]"
            got, args = _run_on_views(call, operands, written, (s,), {s: where}, what)
            assert len(got) == len(ref)
            for i, (a, b) in enumerate(zip(got, ref)):
                same(a, b, f"{what} output {i}")
            for w_ in written:      # a written operand holds the same values as the dense run's, wherever it lives
                same(args[w_].contiguous(), ref_args[w_], f"{what} written operand {w_}")
    # and all slots at once, each at another offset
    where_of = {s: WHERE[i % 3] for i, s in enumerate(operands)}
    got, args = _run_on_views(call, operands, written, tuple(operands), where_of, f"{case} {dtype} [all slots]")
    for i, (a, b) in enumerate(zip(got, ref)):
        same(a, b, f"{case} {dtype} [all slots] output {i}")


# ------------------------------------------------------------------------------------------------
# (c) convolution families
# ------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def switches(r32_min_voxels=None, rw=None, rw48=None, pw=None, wgrad_waves=None):
    """set kernel-selection switches of the library for the block, restore them afterwards"""
    L = _lib.lib()
    old = {}
    try:
        if r32_min_voxels is not None:
            old["mv"] = L.cbim_conv_r32_min_voxels(r32_min_voxels)
        if rw is not None:
            old["rw"] = L.cbim_conv_rw_enable(rw, -1)
        if rw48 is not None:
            old["rw48"] = L.cbim_conv_rw48_enable(rw48)
        if pw is not None:
            old["pw"] = L.cbim_conv_pw_enable(pw)
        if wgrad_waves is not None:
            L.cbim_wgrad_r32_waves(wgrad_waves)
        yield L
    finally:
        if "mv" in old:
            L.cbim_conv_r32_min_voxels(old["mv"])
        if "rw" in old:
            L.cbim_conv_rw_enable(old["rw"] & 1, old["rw"] >> 1)
        if "rw48" in old:
            L.cbim_conv_rw48_enable(old["rw48"])
        if "pw" in old:
            L.cbim_conv_pw_enable(old["pw"])
        if wgrad_waves is not None:
            L.cbim_wgrad_r32_waves(8)


KERNEL_NAMES = {0: "k_conv_igemm", 1: "k_conv3_r32", 2: "k_conv3_rw", 3: "k_conv3_rw split-K + finish", 4: "k_conv_pw", 5: "k_conv3_rw48"}
WGRAD_NAMES = {0: "k_conv_wgrad", 1: "k_wgrad_r32", 2: "k_pw_wgrad"}

# family -> dict(dtype, N, Cin, Cout, dhw, k, act, sw = switches(), fwd = forward kernel | None (forward / dgrad not part of the
# family), wgrad = weight-gradient kernel | None, xsplit / dysplit = channel split of the two-tensor operands (0: one tensor))
CONV_FAMILIES = {
    "igemm-f32 8->12": dict(dtype=F32, N=2, Cin=8, Cout=12, dhw=(5, 6, 7), k=3, act="relu", sw={}, fwd=0, wgrad=0),
    "igemm-bf16 40->72": dict(dtype=BF16, N=1, Cin=40, Cout=72, dhw=(6, 9, 10), k=3, act="relu", sw={}, fwd=0, wgrad=0, xsplit=32),
    "r32 32->32": dict(dtype=BF16, N=2, Cin=32, Cout=32, dhw=(9, 16, 11), k=3, act="relu", sw=dict(r32_min_voxels=0, rw=0), fwd=1),
    "rw 32->32": dict(dtype=BF16, N=2, Cin=32, Cout=32, dhw=(9, 16, 11), k=3, act="relu", sw=dict(r32_min_voxels=0, rw=1), fwd=2),
    "r32 96->64 x2@32": dict(dtype=BF16, N=1, Cin=96, Cout=64, dhw=(8, 9, 8), k=3, act="relu", sw=dict(r32_min_voxels=0, rw=0), fwd=1,
                             xsplit=32, dysplit=32),
    "rw 96->64 x2@32": dict(dtype=BF16, N=1, Cin=96, Cout=64, dhw=(8, 9, 8), k=3, act="relu", sw=dict(r32_min_voxels=0, rw=1), fwd=2,
                            xsplit=32, dysplit=32),
    "split-K 64->64": dict(dtype=BF16, N=1, Cin=64, Cout=64, dhw=(8, 8, 8), k=3, act="relu", sw=dict(rw=1), fwd=3, xsplit=32, dysplit=32),
    "split-K 128->64": dict(dtype=BF16, N=1, Cin=128, Cout=64, dhw=(9, 8, 8), k=3, act="relu", sw=dict(rw=1), fwd=3, xsplit=32, dysplit=32),
    "rw48 48->48": dict(dtype=BF16, N=1, Cin=48, Cout=48, dhw=(8, 9, 16), k=3, act="lrelu", sw=dict(rw48=2), fwd=5, xsplit=32, dysplit=32),
    "pw 64->96": dict(dtype=BF16, N=2, Cin=64, Cout=96, dhw=(5, 6, 7), k=1, act="relu", sw=dict(pw=1), fwd=4, wgrad=2),
    "wgrad 20->40": dict(dtype=F32, N=2, Cin=20, Cout=40, dhw=(5, 9, 11), k=3, act="relu", sw={}, fwd=None, wgrad=0),
    "wgrad-r32 32->32 8 waves": dict(dtype=BF16, N=1, Cin=32, Cout=32, dhw=(8, 16, 8), k=3, act="relu", sw=dict(wgrad_waves=8), fwd=None, wgrad=1),
    "wgrad-r32 32->32 4 waves": dict(dtype=BF16, N=1, Cin=32, Cout=32, dhw=(8, 16, 8), k=3, act="relu", sw=dict(wgrad_waves=4), fwd=None, wgrad=1),
    "wgrad-r32 96->48 8 waves": dict(dtype=BF16, N=1, Cin=96, Cout=48, dhw=(17, 24, 33), k=3, act="relu", sw=dict(wgrad_waves=8), fwd=None,
                                     wgrad=1, xsplit=32, dysplit=32),
    "wgrad-r32 96->48 4 waves": dict(dtype=BF16, N=1, Cin=96, Cout=48, dhw=(17, 24, 33), k=3, act="relu", sw=dict(wgrad_waves=4), fwd=None,
                                     wgrad=1, xsplit=32, dysplit=32),
}


def _tol(dtype, f32, bf16):
    """op_checks.tol"""
    return bf16 if dtype == BF16 else f32


def _relerr(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def _cl(t):            # channels-last -> NCDHW float64 on the CPU
    return t.detach().double().cpu().permute(0, 4, 1, 2, 3)


def _split(t, at):
    return (t[..., :at].contiguous(), t[..., at:].contiguous()) if at else (t, None)


def _compare(op, got, ref, k_got, k_ref, f64, tols, names, what, record):
    """same kernel: the same bits; another kernel for the view (its eligibility depends on the row stride): both runs against the
    float64 evaluation `f64` with op_checks' tolerance for the op"""
    record.append((what, names.get(k_ref, k_ref), names.get(k_got, k_got)))
    if k_got == k_ref:
        for i, (a, b) in enumerate(zip(got, ref)):
            same(a, b, f"{what} output {i}")
        return
    for run, outs in (("view", got), ("dense", ref)):
        for i, (a, r, t) in enumerate(zip(outs, f64, tols)):
            if r is not None:
                e = _relerr(a.cpu(), r)
                print(f"{what} [{run}, {names.get(k_got if run == 'view' else k_ref)}] output {i}: rel err {e:.3e} (limit {t:.1e})")
                assert e < t, f"{what} [{run}] output {i} against float64: {e:.3e} >= {t:.1e}"


def check_conv_family(dev, family, record=None):
    """forward (x, x2, res, y), plain dgrad with an accumulate tensor (dy, dy2, accumulate), masked dgrad (dy, dy2, mask_x) and
    weight gradient (x, x2, dy, dy2) of one kernel family: every operand as a view, at each of the three offsets, against the
    dense call"""
    f = CONV_FAMILIES[family]
    record = [] if record is None else record
    dtype, N, Cin, Cout, dhw, act = f["dtype"], f["N"], f["Cin"], f["Cout"], f["dhw"], f["act"]
    k, pad = (f["k"],) * 3, (f["k"] // 2,) * 3
    xs, dys = f.get("xsplit", 0), f.get("dysplit", 0)
    geom = ops.ConvGeom(dtype, N, dhw, Cin, Cout, k, pad, ACT[act])
    w = rnd((Cout, Cin) + k, F32, dev, 60, scale=0.1)
    slope = 0.01
    a_full = rnd((N,) + dhw + (Cin,), F32, dev, 61, shift=0.3)
    a_full = (torch.relu(a_full) if act == "relu" else F.leaky_relu(a_full, slope)).to(dtype)    # an activated tensor: input and dgrad mask
    dy_full = rnd((N,) + dhw + (Cout,), dtype, dev, 62)
    res, acc = rnd((N,) + dhw + (Cout,), dtype, dev, 63, shift=2.0), rnd((N,) + dhw + (Cin,), dtype, dev, 64)
    xa, xb = _split(a_full, xs)
    dya, dyb = _split(dy_full, dys)
    wr = (w.to(dtype) if dtype == BF16 else w).double().cpu()
    t_out = _tol(dtype, 2e-5, 1e-2)          # op_checks.check_conv / check_conv_r32 / check_conv_rw: forward, dgrad
    t_w = 1e-3 if dtype == BF16 else 5e-5    # op_checks.check_conv / check_wgrad_r32: weight gradient
    with switches(**f["sw"]) as L:
        if f["fwd"] is not None:
            wp, wpd = ops.pack_weights(w, geom, 0), ops.pack_weights(w, geom, 1)
            out_shape = (N,) + dhw + (Cout,)
            y0 = rnd(out_shape, dtype, dev, 65)
            last = []

            def fwd(x, res, out, x2=None):
                y, part = ops.conv_igemm(geom.fwd, x, wp, out_shape, res=res, want_partials=True, x2=x2, out=out)
                last.append(L.cbim_conv3d_last_kernel())
                return y, part

            def dgrad_acc(dy, accumulate, dy2=None):
                g, _ = ops.conv_dgrad(dy, wpd, geom, accumulate=accumulate, dy2=dy2)
                last.append(L.cbim_conv3d_last_kernel())
                return (g,)

            def dgrad_mask(dy, mask_x, dy2=None):
                g, sums = ops.conv_dgrad(dy, wpd, geom, mask_x=mask_x, mask_stats=None, dy2=dy2)
                last.append(L.cbim_conv3d_last_kernel())
                return g, sums

            yr = F.conv3d(_cl(a_full), wr, None, 1, pad)
            gr = F.conv_transpose3d(_cl(dy_full), wr, None, 1, pad)
            af = _cl(a_full)
            gm = gr * (af > 0) if act == "relu" else torch.where(af > 0, gr, slope * gr)
            ncl = lambda t: t.permute(0, 2, 3, 4, 1)
            calls = [
                ("forward", fwd, {"x": xa, "x2": xb, "res": res, "out": y0}, ("out",), (ncl(yr + _cl(res)), None), (t_out, None)),
                ("dgrad + accumulate", dgrad_acc, {"dy": dya, "dy2": dyb, "accumulate": acc}, (), (ncl(gr + _cl(acc)),), (t_out,)),
                ("masked dgrad", dgrad_mask, {"dy": dya, "dy2": dyb, "mask_x": a_full}, (), (ncl(gm), None), (t_out, None)),
            ]
            for nm, call, operands, written, f64, tols in calls:
                operands = {s: t for s, t in operands.items() if t is not None}
                what = f"{family}: {nm}"
                ref, ref_args = _run_on_views(call, operands, written, (), {}, what)
                k_ref = last[-1]
                if nm == "forward":
                    assert k_ref == f["fwd"], f"{what}: {KERNEL_NAMES[k_ref]} ran on the dense call, not {KERNEL_NAMES[f['fwd']]}"
                slots = tuple(operands)
                runs = [((s,), {s: "mid"}) for s in slots]                                                  # one operand at a time
                runs += [(slots, {s: WHERE[(i + r) % 3] for i, s in enumerate(slots)}) for r in range(3)]   # all, every slot at every offset
                for as_view, where_of in runs:
                    tag = f"{what} [{', '.join(f'{s} @ {where_of[s]}' for s in as_view)}]"
                    got, args = _run_on_views(call, operands, written, as_view, where_of, tag)
                    for w_ in written:
                        got = got + [args[w_].contiguous()]
                    _compare(nm, got, ref + [ref_args[w_] for w_ in written], last[-1], k_ref, f64 + f64[:len(written)],
                             tols + tols[:len(written)], KERNEL_NAMES, tag, record)
        if f.get("wgrad") is not None or f["fwd"] is not None:
            lastw = []

            def wgrad(x, dy, x2=None, dy2=None):
                dw = ops.conv_wgrad(x, None, dy, geom, dy2=dy2, x2=x2)
                lastw.append(L.cbim_conv3d_wgrad_last_kernel())
                return (dw,)

            # (a second input / gradient tensor is taken by k_wgrad_r32 with channel counts in multiples of 32 only)
            two = dtype == BF16 and f["k"] == 3 and Cin % 32 == 0 and Cout % 32 == 0
            wxa, wxb = (xa, xb) if two else (a_full, None)
            wda, wdb = (dya, dyb) if two else (dy_full, None)
            operands = {s: t for s, t in {"x": wxa, "x2": wxb, "dy": wda, "dy2": wdb}.items() if t is not None}
            what = f"{family}: wgrad"
            ref, _ = _run_on_views(wgrad, operands, (), (), {}, what)
            k_ref = lastw[-1]
            if f.get("wgrad") is not None:
                assert k_ref == f["wgrad"], f"{what}: {WGRAD_NAMES[k_ref]} ran on the dense call, not {WGRAD_NAMES[f['wgrad']]}"
            wz = torch.zeros(Cout, Cin, *k, dtype=torch.float64, requires_grad=True)
            F.conv3d(_cl(a_full), wz, None, 1, pad).backward(_cl(dy_full))
            slots = tuple(operands)
            runs = [(slots, {s: WHERE[(i + r) % 3] for i, s in enumerate(slots)}) for r in range(3)]    # every slot at every offset
            for as_view, where_of in runs:
                tag = f"{what} [{', '.join(f'{s} @ {where_of[s]}' for s in as_view)}]"
                got, _ = _run_on_views(wgrad, operands, (), as_view, where_of, tag)
                _compare("wgrad", got, ref, lastw[-1], k_ref, (wz.grad,), (t_w,), WGRAD_NAMES, tag, record)
    return record


# ------------------------------------------------------------------------------------------------
# (d), (e): rejected before the library is reached
# ------------------------------------------------------------------------------------------------

class NoLibrary:
    """stands in for the loaded library: touching any entry of it fails the test"""

    def __call__(self):
        return self

    def __getattr__(self, name):
        raise AssertionError(f"the kernel library was reached ({name})")


@contextlib.contextmanager
def library_patched_out(monkeypatch):
    name = _lib.backend()
    with monkeypatch.context() as m:
        m.setattr(_lib, "backend", lambda: name)
        m.setattr(_lib, "lib", NoLibrary())
        yield


def _view5(dev, dtype=F32, C=16, off=8, wide=32, shape=(1, 4, 4, 6)):
    return torch.zeros(shape + (wide,), dtype=dtype, device=dev)[..., off:off + C]


def _view2(dev, dtype=F32, C=16, off=8, wide=32, rows=12):
    return torch.zeros((rows, wide), dtype=dtype, device=dev)[:, off:off + C]


DENSE_IDS = [(fn, s) for fn, slots in CONTRACT.items() for s, k in slots.items() if k == D]


def _call_with(fn, slot, value, dev):
    """ops.<fn> with `value` in `slot`, small dense tensors in its other contract slots and None everywhere else: the guard is the
    first thing an entry point does, so nothing else is looked at before it raises"""
    params = inspect.signature(getattr(ops, fn)).parameters
    kw = {}
    for p, spec in params.items():
        if p == slot:
            kw[p] = value
        elif p in CONTRACT[fn]:
            kw[p] = torch.zeros((12, 16) if (fn, p) in ROW_OPERANDS else (1, 4, 4, 6, 16), device=dev)
        elif p == "geom":            # (conv_fwd / conv_dgrad read the geometry on their way to conv_igemm's guard)
            kw[p] = ops.ConvGeom(F32, 1, (4, 4, 6), 16, 16, (3, 3, 3), (1, 1, 1), 0)
        elif spec.default is inspect.Parameter.empty:
            kw[p] = None
    return getattr(ops, fn)(**kw)


def check_dense_slot(dev, fn, slot, monkeypatch):
    v = _view2(dev) if (fn, slot) in ROW_OPERANDS else _view5(dev)
    assert not v.is_contiguous()
    with library_patched_out(monkeypatch):
        with pytest.raises(RuntimeError, match="non-contiguous"):
            _call_with(fn, slot, v, dev)


def misaligned_views(dev):
    """(name, 5-D view, 2-D row view) the 16-byte chunks cannot address"""
    return [
        ("bf16 view 4 channels in", _view5(dev, BF16, 16, 4), _view2(dev, BF16, 16, 4)),
        ("fp32 view 2 channels in", _view5(dev, F32, 16, 2), _view2(dev, F32, 16, 2)),
        ("bf16 row stride of 36 channels", _view5(dev, BF16, 16, 0, wide=36), _view2(dev, BF16, 16, 0, wide=36)),
        ("fp32 row stride of 18 channels", _view5(dev, F32, 16, 0, wide=18), _view2(dev, F32, 16, 0, wide=18)),
        ("bf16 view of 12 channels", _view5(dev, BF16, 12, 8), _view2(dev, BF16, 12, 8)),
        ("fp32 view of 6 channels", _view5(dev, F32, 6, 4), _view2(dev, F32, 6, 4)),
    ]


def check_misaligned(dev, monkeypatch):
    strided5 = [(fn, s) for fn, slots in CONTRACT.items() for s, k in slots.items() if k == S and (fn, s) not in ROW_OPERANDS
                and not fn.startswith("bidir_attn_gemm")]
    strided2 = [(fn, s) for fn, slots in CONTRACT.items() for s, k in slots.items() if k == S and (fn, s) in ROW_OPERANDS]
    with library_patched_out(monkeypatch):
        for name, v5, v2 in misaligned_views(dev):
            assert not v5.is_contiguous() and not v2.is_contiguous()
            with pytest.raises(RuntimeError, match="non-contiguous"):
                ops._view_ok(v5)
            with pytest.raises(RuntimeError, match="non-contiguous"):
                ops._rows_ok(v2)
            assert ops.as_rows(v5).is_contiguous(), f"{name}: as_rows must copy what the kernels cannot address"
            for fn, s in strided5:
                with pytest.raises(RuntimeError, match="non-contiguous"):
                    _call_with(fn, s, v5, dev)
            for fn, s in strided2:
                with pytest.raises(RuntimeError, match="non-contiguous"):
                    _call_with(fn, s, v2, dev)
        # and the aligned forms of the same views pass the guards
        ops._view_ok(_view5(dev, BF16, 16, 8), _view5(dev, F32, 16, 4), None)
        ops._rows_ok(_view2(dev, BF16, 16, 8), _view2(dev, F32, 16, 4), None)
        with pytest.raises(RuntimeError, match="non-contiguous"):
            ops._dev_ok(_view5(dev, BF16, 16, 8))


# ------------------------------------------------------------------------------------------------
# (f) autograd Functions
# ------------------------------------------------------------------------------------------------

def _stats(t):
    return ops.instnorm_stats(t.detach())


def _w(dev, shape, seed, scale=0.1):
    return rnd(shape, F32, dev, seed, scale=scale)


def _autograd_cases(dev, dtype):
    """name -> (fn(x) -> outputs, dense input x [..., C]); x is the operand that arrives as a view"""
    c = {}
    relu, lrelu, elu = ACT["relu"], ACT["lrelu"], ACT["elu"]
    x16 = _act5(dev, dtype, 70, C=16, dhw=(4, 6, 8), N=1)
    w16, w16b, w1x = _w(dev, (16, 16, 3, 3, 3), 71), _w(dev, (16, 16, 3, 3, 3), 72), _w(dev, (16, 16, 1, 1, 1), 73)
    w32, w32b, w32sc = _w(dev, (32, 16, 3, 3, 3), 74), _w(dev, (32, 32, 3, 3, 3), 75), _w(dev, (32, 16, 3, 3, 3), 76)
    c["BasicBlockFn identity"] = (lambda x: Fn.BasicBlockFn.apply(x, _stats(x), w16, w16b, None, relu, True)[:1], x16)
    c["BasicBlockFn conv1|shortcut"] = (lambda x: Fn.BasicBlockFn.apply(x, _stats(x), w32, w32b, w32sc, relu, False)[:1], x16)
    c["BasicBlockFn gelu"] = (lambda x: Fn.BasicBlockFn.apply(x, _stats(x), w16, w16b, w1x, ACT["gelu"], False)[:1], x16)
    low = _act5(dev, dtype, 77, C=16, dhw=(2, 3, 4), N=1)
    wu1, wu2, wusc = _w(dev, (16, 32, 3, 3, 3), 78), _w(dev, (16, 16, 3, 3, 3), 79), _w(dev, (16, 32, 1, 1, 1), 80)
    c["UpBlockFirstFn low"] = (lambda t: Fn.UpBlockFirstFn.apply(t, x16, _stats(x16), wu1, wu2, wusc, relu, False, True)[:1], low)
    c["UpBlockFirstFn skip"] = (lambda t: Fn.UpBlockFirstFn.apply(low, t, _stats(t), wu1, wu2, wusc, relu, False, True)[:1], x16)
    c["SingleConvFn"] = (lambda x: (Fn.SingleConvFn.apply(x, w16, relu, True),), x16)
    c["MaxPoolFn"] = (lambda x: (Fn.MaxPoolFn.apply(x, (2, 2, 2)),), x16)
    c["UpCatFn low"] = (lambda t: Fn.UpCatFn.apply(t, x16, True, True)[:1], low)
    c["UpCatFn skip"] = (lambda t: (Fn.UpCatFn.apply(low, t, False),), x16)
    wh, bh = _w(dev, (3, 16, 1, 1, 1), 81), _w(dev, (3,), 82)
    c["HeadFn"] = (lambda x: (Fn.HeadFn.apply(x, wh, bh),), x16)
    c["NormConvFn"] = (lambda x: Fn.NormConvFn.apply(x, _stats(x), w16, relu, None, True, None, ops.IN_EPS)[:1], x16)
    c["NormConvFn res"] = (lambda r: Fn.NormConvFn.apply(x16, None, w16, 0, r, False, None, ops.IN_EPS)[:1], x16 * 0.5)
    c["DualRawConvFn"] = (lambda x: Fn.DualRawConvFn.apply(x, w16, w1x, 1e-5)[::2], x16)
    wdw = _w(dev, (16, 1, 3, 3, 3), 83, 0.2)
    c["DWConvFn"] = (lambda x: Fn.DWConvFn.apply(x, _stats(x), wdw, relu, True)[:2], x16)
    c["ChannelMeanFn"] = (lambda x: (Fn.ChannelMeanFn.apply(x, _stats(x)),), x16)
    c["SpaceToDepthFn"] = (lambda x: (Fn.SpaceToDepthFn.apply(x, (2, 2, 2)),), x16)
    qv, mq, mv, inner = _attn_operands(dev, dtype)
    c["BidirAttnFn"] = (lambda t: Fn.BidirAttnFn.apply(t, mq, mv, _HEADS, _DH ** -0.5), qv)
    c["MapPoolFn"] = (lambda t: (Fn.MapPoolFn.apply(t, 16),), _act5(dev, dtype, 84, C=24, dhw=(4, 6, 8), N=1, shift=0.0))
    c["ResNormFn a"] = (lambda t: (Fn.ResNormFn.apply(t, _stats(t), x16, _stats(x16), lrelu),), x16 * 0.7)
    c["ResNormFn b"] = (lambda t: (Fn.ResNormFn.apply(x16, _stats(x16), t, None, lrelu),), x16 * 0.7)
    t8 = _act5(dev, dtype, 85, C=8 * 8, dhw=(2, 3, 4), N=1)
    c["DepthToSpaceFn"] = (lambda x: (Fn.DepthToSpaceFn.apply(x, (2, 2, 2)),), t8)
    c["UpCatSkipFn t"] = (lambda t: (Fn.UpCatSkipFn.apply(t, x16, (2, 2, 2)),), t8)
    c["UpCatSkipFn skip"] = (lambda t: (Fn.UpCatSkipFn.apply(t8, t, (2, 2, 2)),), x16)
    c["NormActFn"] = (lambda x: (Fn.NormActFn.apply(x, _stats(x), relu),), x16)
    c["ActFn"] = (lambda x: (Fn.ActFn.apply(x, elu),), x16)
    bias16 = _w(dev, (16,), 86, 1.0)
    c["BiasAddFn"] = (lambda x: (Fn.BiasAddFn.apply(x, bias16.clone().requires_grad_()),), x16)
    gam, bet = _w(dev, (16,), 87, 1.0), _w(dev, (16,), 88, 1.0)
    c["BatchNormActFn"] = (lambda x: (Fn.BatchNormActFn.apply(x, gam, bet, torch.zeros(16, device=dev), torch.ones(16, device=dev), 0.1, 1e-5,
                                                                elu, True),), x16)
    w5, b5 = _w(dev, (16, 16, 5, 5, 5), 89, 0.03), _w(dev, (16,), 90)
    c["ConvSlicesFn"] = (lambda x: (Fn.ConvSlicesFn.apply(x, w5, b5),), x16)
    g133 = ops.ConvGeom(dtype, 1, (4, 6, 8), 16, 16, (1, 3, 3), (0, 1, 1), 0)
    w133 = _w(dev, (16, 16, 1, 3, 3), 91)
    c["RawConvFn"] = (lambda x: (Fn.RawConvFn.apply(x, w133, g133),), x16)
    psi = torch.sigmoid(rnd((1, 4, 6, 8), F32, dev, 92))
    c["GateFn"] = (lambda x: (Fn.GateFn.apply(x, psi),), x16)
    wl, bl = _w(dev, (40, 16), 93), _w(dev, (40,), 94)
    c["TokenLinearFn"] = (lambda x: (Fn.token_linear(x, wl, bl),), x16)
    if dtype == F32:     # the float32 residual stream / image operands
        lg, lb = _w(dev, (16,), 95, 1.0), _w(dev, (16,), 96)
        c["LayerNormFn"] = (lambda x: (Fn.layer_norm(x, lg, lb, 1e-5, BF16),), x16)
        c["LayerNormResFn"] = (lambda x: Fn.LayerNormResFn.apply(x, lg, lb, 1e-5, F32), x16)
        c["TokenLinearFn res"] = (lambda r: (Fn.token_linear(x16.bfloat16(), wl, bl, res=r),), _act5(dev, F32, 97, C=40, dhw=(4, 6, 8), N=1))
        ws = _w(dev, (8, 2, 3, 3, 3), 98)
        c["StemFn"] = (lambda x: (Fn.StemFn.apply(x, ws, BF16),), rnd((1, 2, 5, 6, 8), F32, dev, 99))
    qkv = _act5(dev, dtype, 100, C=72, dhw=(9, 8, 7), N=1, shift=0.0)
    qb, tbl = _w(dev, (72,), 101), _w(dev, (13 ** 3, 3), 102)
    c["WindowAttnFn"] = (lambda t: (Fn.WindowAttnFn.apply(t, qb, tbl, 3, (7, 7, 7), (3, 3, 3), (7, 7, 7)),), qkv)
    return c


AUTOGRAD_NAMES = (
    "BasicBlockFn identity", "BasicBlockFn conv1|shortcut", "BasicBlockFn gelu", "UpBlockFirstFn low", "UpBlockFirstFn skip", "SingleConvFn",
    "MaxPoolFn", "UpCatFn low", "UpCatFn skip", "HeadFn", "NormConvFn", "NormConvFn res", "DualRawConvFn", "DWConvFn", "ChannelMeanFn",
    "SpaceToDepthFn", "DepthToSpaceFn", "BidirAttnFn", "MapPoolFn", "ResNormFn a", "ResNormFn b", "UpCatSkipFn t", "UpCatSkipFn skip",
    "NormActFn", "ActFn", "BiasAddFn", "BatchNormActFn", "ConvSlicesFn", "RawConvFn", "GateFn", "TokenLinearFn", "WindowAttnFn")
AUTOGRAD_F32_ONLY = ("LayerNormFn", "LayerNormResFn", "TokenLinearFn res", "StemFn")
AUTOGRAD_IDS = [(n, dt) for n in AUTOGRAD_NAMES for dt in BOTH] + [(n, F32) for n in AUTOGRAD_F32_ONLY]

# every autograd.Function of functional.py is either exercised above or takes no activation tensor
AUTOGRAD_NO_ACTIVATION = {
    "DiceCEFn": "NCDHW logits, made contiguous float32 first", "FocalFn": "NCDHW logits, made contiguous float32 first",
    "TopKCEFn": "NCDHW logits, made contiguous float32 first", "DicePerClassFn": "NCDHW logits, made contiguous float32 first",
    "SEGateFn": "channel means [N, C]", "MapQVFn": "semantic map [B, C, M]", "MapOutFn": "semantic map [B, C, M]",
    "TrilinearPlanesFn": "NCDHW float32 logits planes, made contiguous first", "_GradAwareFunction": "base class",
}


def check_autograd_cases_complete():
    fns = [n for n, o in vars(Fn).items() if inspect.isclass(o) and issubclass(o, torch.autograd.Function) and o.__module__ == Fn.__name__]
    names = AUTOGRAD_NAMES + AUTOGRAD_F32_ONLY
    missing = [n for n in fns if n not in AUTOGRAD_NO_ACTIVATION and not any(c.split(" ")[0] == n for c in names)]
    assert not missing, f"autograd Functions without a view case: {missing}"


_CASES_CACHE = {}


def check_autograd(dev, name, dtype):
    key = (dev, dtype)
    if key not in _CASES_CACHE:
        _CASES_CACHE[key] = _autograd_cases(dev, dtype)
    fn, x = _CASES_CACHE[key][name]
    ch = chunk(x.dtype)
    Cc = int(x.shape[-1])
    assert Cc % ch == 0
    wide0 = rnd(tuple(x.shape[:-1]) + (Cc + 2 * ch,), x.dtype, x.device, 7)

    def diff(outs):
        return [o for o in outs if o.requires_grad]

    def grads_for(outs):
        return [rnd(tuple(o.shape), o.dtype, o.device, 200 + i) for i, o in enumerate(outs)]

    for where, off in zip(WHERE, (0, ch, 2 * ch)):
        wide0[..., off:off + Cc] = x
        # reference: the same graph with .contiguous() inserted
        wr = wide0.clone().requires_grad_()
        outs_r = list(fn(wr[..., off:off + Cc].contiguous()))
        gs = grads_for(diff(outs_r))
        torch.autograd.backward(diff(outs_r), gs)
        # the view itself
        wv = wide0.clone().requires_grad_()
        xv = wv[..., off:off + Cc]
        assert not xv.is_contiguous()
        outs_v = list(fn(xv))
        torch.autograd.backward(diff(outs_v), gs)
        what = f"{name} {dtype} [view @ {where}]"
        assert len(outs_v) == len(outs_r)
        for i, (a, b) in enumerate(zip(outs_v, outs_r)):
            assert torch.equal(a, b), f"{what}: output {i} differs from the contiguous graph, max abs {float((a.float() - b.float()).abs().max()):.3e}"
        if wr.grad is None:         # (StemFn: the image gets no gradient)
            assert wv.grad is None
            continue
        assert torch.equal(wv.grad, wr.grad), f"{what}: gradient differs, max abs {float((wv.grad.float() - wr.grad.float()).abs().max()):.3e}"
    if wr.grad is None:
        return
    # downstream torch.cat: every output's gradient arrives as a channel slice, one chunk in
    wc = wide0.clone().requires_grad_()
    outs_c = diff(list(fn(wc[..., 2 * ch:2 * ch + Cc].contiguous())))
    cats, gcats = [], []
    for o, g in zip(outs_c, gs):
        pad = torch.zeros(tuple(o.shape[:-1]) + (chunk(o.dtype),), dtype=o.dtype, device=o.device)
        cats.append(torch.cat([pad, o, pad], -1))
        gcats.append(torch.cat([pad, g, pad], -1))
    torch.autograd.backward(cats, gcats)
    assert torch.equal(wc.grad, wr.grad), \
        f"{name} {dtype} [gradient through torch.cat]: differs, max abs {float((wc.grad.float() - wr.grad.float()).abs().max()):.3e}"
