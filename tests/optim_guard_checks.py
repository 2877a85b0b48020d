"""The guarded FusedAdamW step — clipping by the global gradient norm, torch.amp.GradScaler's grad_scale / found_inf protocol and
the skip of a non-finite step (cbim_adamw_ema_step_guarded: k_grad_sumsq, k_grad_ctl, the guarded k_adamw_ema) — against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(eps=1e-5) + the restated EMA loop.  Shared by the CPU suite (host-side executor,
tests/test_optim_guard_emu.py) and the -m gpu suite (tests/test_gpu_optim_guard.py).

Shapes: tensors of 1, 4095, 4096 and 4097 elements (one element, one short of a chunk, a chunk, a chunk and one: every path of
k_grad_sumsq — float4 body, element-wise last group, second block) and, in the parity case, one of 300 * 4096 + 1 elements, which
gives k_grad_ctl 304 partial sums for its 256 threads.

Gradient magnitudes: the parity case clips at 1000 and 250 with gradient norms of 10x and 0.1x the limit, so that with 1.2 M
elements a clipped element is O(0.1 .. 1) and the moments O(1e-3 .. 1): the RELATIVE part of the tolerance 2e-6 * max + 1e-8 is the
one that binds for parameters, exp_avg and exp_avg_sq alike (with unit-norm gradients the 1e-8 would swallow exp_avg_sq whole)."""
import copy
import ctypes
import functools

import torch
import torch.nn as nn

from cbim_amd import _lib
from cbim_amd.training.optim import FusedAdamW
from tests.optim_checks import _ema_ref

SMALL = (1, 4095, 4096, 4097)
SIZES = SMALL + (300 * 4096 + 1,)
KW = dict(lr=6e-4, betas=(0.9, 0.999), weight_decay=0.05, eps=1e-5)
ALPHA = 0.99
# (max_grad_norm, norm of the gradients) of the four parity steps; before step 2 the lr drops to 3e-4 and the limit to 250
PARITY_STEPS = ((1000.0, 1.0e4), (1000.0, 100.0), (250.0, 2500.0), (250.0, 25.0))
# grad_norm against the float64 norm.  Roundings on the longest path of the reduction (csrc/optim_kernels.hip): the unscale
# multiply counts twice in the square and the product once (3), 15 additions of the thread's 16 squares, 6 butterfly steps over the
# wave, 3 additions over the four waves = 27 on the sum of squares (the partials are added in double), halved by the square root
# = 13.5, + 1 for the float result of the root = 14.5 roundings of 2^-24; 15 * 2^-24 = 8.94e-7 leaves room for the second-order terms.
NORM_RTOL = 15 * 2.0 ** -24


class Params(nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.w = nn.ParameterList([nn.Parameter(t) for t in tensors])


def make_model(dev, sizes, seed=41):
    g = torch.Generator().manual_seed(seed)
    return Params([torch.randn(n, generator=g) for n in sizes]).to(dev)


def make_grads(sizes, seed, norm):
    """CPU float32 gradients whose float64 L2 norm is `norm` (to float32 rounding), and that norm of the values as stored."""
    g = torch.Generator().manual_seed(seed)
    gs = [torch.randn(n, generator=g, dtype=torch.float64) for n in sizes]
    tot = sum(float((x * x).sum()) for x in gs) ** 0.5
    gs = [(x * (norm / tot)).float() if tot > 0 else x.float() for x in gs]
    return gs, norm64(gs)


def norm64(grads):
    return sum(float((x.double().cpu() ** 2).sum()) for x in grads if x is not None) ** 0.5


def set_grads(model, grads, dev, scale=1.0):
    for p, g in zip(model.parameters(), grads):
        p.grad = None if g is None else (g * scale).to(dev)        # a power-of-two scale is exact


def close(a, b):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()) + 1e-8


def bits(opt, model, ema):
    """Everything a step may write, cloned: parameters, EMA, moments, the published step counter."""
    sd = opt.state_dict()["state"]
    return ([p.detach().clone() for p in model.parameters()], [e.detach().clone() for e in ema.parameters()],
            [sd[i][k].clone() for i in sorted(sd) for k in ("exp_avg", "exp_avg_sq")], [sd[i]["step"].clone() for i in sorted(sd)])


def same_bits(a, b):
    return all(len(x) == len(y) and all(torch.equal(s, t) for s, t in zip(x, y)) for x, y in zip(a, b))


def clip_ref(model, max_norm):
    """torch.nn.utils.clip_grad_norm_ on the model's gradients, evaluated on float64 copies of them and stored back as float32.
    In float32 on the CPU the function's own norm is not good enough to be the reference at 2e-6: it adds the 1.2 M squares of the
    parity case lane by lane in float32 and comes out 1.5e-5 low (9999.848 for gradients whose float64 norm is 10000.0000003,
    measured with torch 2.10), an error that goes straight into the coefficient and from there into exp_avg and exp_avg_sq."""
    ps = [p for p in model.parameters() if p.grad is not None]
    holders = [torch.zeros_like(p.grad, dtype=torch.float64) for p in ps]
    for h, p in zip(holders, ps):
        h.grad = p.grad.double()
    torch.nn.utils.clip_grad_norm_(holders, max_norm)
    for h, p in zip(holders, ps):
        p.grad = h.grad.float()


def ref_step(ref, ema_ref, opt_ref, grads, max_norm, step, dev):
    """clip_grad_norm_ -> torch.optim.AdamW.step -> update_ema_variables, on unscaled gradients."""
    set_grads(ref, grads, dev)
    if max_norm is not None:
        clip_ref(ref, max_norm)
    opt_ref.step()
    _ema_ref(ref, ema_ref, ALPHA, step)


# ---- 1. parity with torch, clipping on (and 4a: the same through grad_scale = 65536) ----------------------------------------------

@functools.lru_cache(maxsize=None)
def parity_reference(dev):
    """The torch trajectory of the parity case, computed once: per step (parameters, EMA, float64 gradient norm), final moments."""
    ref = make_model(dev, SIZES)
    ema_ref = copy.deepcopy(ref)
    opt_ref = torch.optim.AdamW(ref.parameters(), **KW)
    steps = []
    for s, (limit, norm) in enumerate(PARITY_STEPS):
        if s == 2:
            opt_ref.param_groups[0]["lr"] = 3e-4
        grads, n64 = make_grads(SIZES, 100 + s, norm)
        assert abs(n64 / limit - 1.0) > 1e-3          # no case within 1e-3 relative of the limit
        ref_step(ref, ema_ref, opt_ref, grads, limit, s, dev)
        steps.append(([p.detach().clone() for p in ref.parameters()], [e.detach().clone() for e in ema_ref.parameters()], n64))
    sd = opt_ref.state_dict()["state"]
    return steps, [(sd[i]["exp_avg"], sd[i]["exp_avg_sq"]) for i in range(len(SIZES))]


def check_parity(dev, scale=None):
    """Returns the worst relative error of grad_norm against the float64 norm."""
    steps, moments = parity_reference(dev)
    net = make_model(dev, SIZES)
    ema = copy.deepcopy(net)
    opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=ALPHA, max_grad_norm=PARITY_STEPS[0][0], **KW)
    assert opt.param_groups[0]["max_grad_norm"] == PARITY_STEPS[0][0]
    if scale is not None:
        opt.grad_scale = torch.tensor(float(scale), device=dev)
        opt.found_inf = torch.tensor(0.0, device=dev)
    worst = 0.0
    for s, (limit, norm) in enumerate(PARITY_STEPS):
        if s == 2:                                    # the scheduler changes the lr, the user the limit: both reach the device
            opt.param_groups[0]["lr"] = 3e-4
            opt.param_groups[0]["max_grad_norm"] = limit
        grads, n64 = make_grads(SIZES, 100 + s, norm)
        set_grads(net, grads, dev, 1.0 if scale is None else float(scale))
        kept = [p.grad.clone() for p in net.parameters()]
        opt.step()
        rp, re, rn = steps[s]
        err = abs(float(opt.grad_norm) - rn) / rn
        worst = max(worst, err)
        print(f"optim_guard parity step {s}: grad_norm {float(opt.grad_norm):.9g} float64 {rn:.9g} rel err {err:.3e} (bound {NORM_RTOL:.3e})")
        assert err <= NORM_RTOL, (s, err)
        assert opt.grad_norm.dim() == 0 and opt.grad_norm.device.type == torch.device(dev).type
        for p, q in zip(net.parameters(), rp):
            assert close(p, q), s
        for e, f in zip(ema.parameters(), re):
            assert close(e, f), s
        for p, k in zip(net.parameters(), kept):      # p.grad is not rewritten: it keeps what backward produced
            assert torch.equal(p.grad, k)
    sd = opt.state_dict()["state"]
    for i, (m, v) in enumerate(moments):
        assert close(sd[i]["exp_avg"], m) and close(sd[i]["exp_avg_sq"], v), i
        assert float(sd[i]["step"]) == len(PARITY_STEPS)
    assert float(opt.skipped_steps) == 0.0
    return worst


# ---- 2. a huge limit is no limit, bit for bit; all-zero gradients ---------------------------------------------------------------------

def _run(dev, sizes, grads_per_step, **opt_kw):
    net = make_model(dev, sizes)
    ema = copy.deepcopy(net)
    opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=ALPHA, **KW, **opt_kw)
    for grads in grads_per_step:
        set_grads(net, grads, dev)
        opt.step()
    return opt, net, ema


def check_huge_limit_is_no_limit(dev):
    gs = [make_grads(SMALL, 200 + s, 3.0)[0] for s in range(3)]
    a = _run(dev, SMALL, gs, max_grad_norm=None)
    b = _run(dev, SMALL, gs, max_grad_norm=1e30)
    assert a[0].grad_norm is None or float(a[0].grad_norm) == 0.0      # the unguarded step computes no norm
    assert same_bits(bits(*a), bits(*b))
    assert float(b[0].state_dict()["state"][0]["step"]) == 3.0 and float(b[0].skipped_steps) == 0.0
    z = _run(dev, SMALL, [[torch.zeros(n) for n in SMALL]], max_grad_norm=1.0)
    assert float(z[0].grad_norm) == 0.0 and float(z[0].skipped_steps) == 0.0
    assert float(z[0].state_dict()["state"][0]["step"]) == 1.0
    assert all(torch.isfinite(p).all() for p in z[1].parameters()) and all(torch.isfinite(e).all() for e in z[2].parameters())
    ref = make_model(dev, SMALL)                      # weight decay alone moves the weights: the step WAS taken
    assert all(not torch.equal(p, q) for p, q in zip(z[1].parameters(), ref.parameters()))


# ---- 3. a non-finite gradient without a scaler skips the step ---------------------------------------------------------------------------

def check_nonfinite_skips(dev):
    limit = 5.0
    net, ref = make_model(dev, SMALL), make_model(dev, SMALL)
    ema, ema_ref = copy.deepcopy(net), copy.deepcopy(ref)
    opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=ALPHA, max_grad_norm=limit, **KW)
    opt_ref = torch.optim.AdamW(ref.parameters(), **KW)
    t = 0

    def good_step():
        nonlocal t
        grads, _ = make_grads(SMALL, 300 + t, 50.0 if t % 2 == 0 else 0.5)
        set_grads(net, grads, dev)
        opt.step()
        ref_step(ref, ema_ref, opt_ref, grads, limit, t, dev)
        t += 1
        for p, q in zip(net.parameters(), ref.parameters()):
            assert close(p, q), t
        for e, f in zip(ema.parameters(), ema_ref.parameters()):
            assert close(e, f), t
        assert float(opt.state_dict()["state"][0]["step"]) == t

    good_step()
    skipped = 0
    for bad in (float("inf"), float("nan")):
        for tensor, pos in ((3, 4096), (0, 0)):       # the last element of the 4097 tensor (its second block), the 1-element tensor
            before = bits(opt, net, ema)
            grads, _ = make_grads(SMALL, 350 + skipped, 1.0)
            grads[tensor][pos] = bad
            set_grads(net, grads, dev)
            opt.step()
            skipped += 1
            assert same_bits(before, bits(opt, net, ema)), (bad, tensor)
            assert float(opt.skipped_steps) == skipped
            assert not torch.isfinite(opt.grad_norm)
            good_step()                               # equals the reference's step t, which never saw the bad one
    assert t == 5


# ---- 4. the AMP protocol: grad_scale / found_inf as attributes ------------------------------------------------------------------------------

def check_amp_protocol(dev):
    limit = 5.0
    net, ref = make_model(dev, SMALL), make_model(dev, SMALL)
    ema, ema_ref = copy.deepcopy(net), copy.deepcopy(ref)
    opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=ALPHA, max_grad_norm=limit, **KW)
    opt_ref = torch.optim.AdamW(ref.parameters(), **KW)
    grads, n64 = make_grads(SMALL, 400, 50.0)
    # found_inf = 1 with finite gradients: skipped
    before = bits(opt, net, ema)
    opt.grad_scale, opt.found_inf = torch.tensor(65536.0, device=dev), torch.tensor(1.0, device=dev)
    set_grads(net, grads, dev, 65536.0)
    opt.step()
    first = bits(opt, net, ema)
    assert same_bits(before[:2], first[:2]) and all(float(m.abs().max()) == 0.0 for m in first[2])
    assert float(first[3][0]) == 0.0 and float(opt.skipped_steps) == 1.0
    assert abs(float(opt.grad_norm) - n64) <= NORM_RTOL * n64      # the norm of the UNSCALED gradients
    # grad_scale = None (the user ran scaler.unscale_) with found_inf = 0: stepped, gradients taken as they are
    opt.grad_scale, opt.found_inf = None, torch.tensor(0.0, device=dev)
    set_grads(net, grads, dev)
    opt.step()
    ref_step(ref, ema_ref, opt_ref, grads, limit, 0, dev)
    for p, q in zip(net.parameters(), ref.parameters()):
        assert close(p, q)
    assert float(opt.state_dict()["state"][0]["step"]) == 1.0 and float(opt.skipped_steps) == 1.0
    # unscaled gradients of magnitude 3e14 under scale 2^16: the scaled values are finite, their squares are not.  The norm is
    # taken after the unscale, so the step is TAKEN, like the reference's scaler.unscale_ -> clip_grad_norm_ -> step
    g = torch.Generator().manual_seed(401)
    big = [3e14 * (torch.randint(0, 2, (n,), generator=g).float() * 2 - 1) * (1 + 0.25 * torch.rand(n, generator=g)) for n in SMALL]
    scaled = [x * 65536.0 for x in big]
    assert all(torch.isfinite(x).all() and not torch.isfinite(x * x).any() for x in scaled)
    opt.grad_scale, opt.found_inf = torch.tensor(65536.0, device=dev), torch.tensor(0.0, device=dev)
    set_grads(net, scaled, dev)
    opt.step()
    unscaled = [x * (1.0 / 65536.0) for x in scaled]                # scaler.unscale_: a multiply by the reciprocal
    ref_step(ref, ema_ref, opt_ref, unscaled, limit, 1, dev)
    assert float(opt.skipped_steps) == 1.0 and float(opt.state_dict()["state"][0]["step"]) == 2.0
    n64 = norm64(unscaled)
    assert abs(float(opt.grad_norm) - n64) <= NORM_RTOL * n64
    for p, q in zip(net.parameters(), ref.parameters()):
        assert close(p, q)
    for e, f in zip(ema.parameters(), ema_ref.parameters()):
        assert close(e, f)
    sd, rsd = opt.state_dict()["state"], opt_ref.state_dict()["state"]
    for i in range(len(SMALL)):
        assert close(sd[i]["exp_avg"], rsd[i]["exp_avg"]) and close(sd[i]["exp_avg_sq"], rsd[i]["exp_avg_sq"])
    assert getattr(FusedAdamW, "_step_supports_amp_scaling") is True


# ---- 5. misaligned base pointers ------------------------------------------------------------------------------------------------------------

def _flat_views(dev, tensors, lead):
    """`tensors` as consecutive views into one flat buffer that starts `lead` elements in (a flat all-reduce bucket); lead None:
    one allocation each, which the allocators align to 64 bytes or more."""
    if lead is None:
        return [t.detach().clone().to(dev) for t in tensors]
    flat = torch.zeros(lead + sum(t.numel() for t in tensors), dtype=torch.float32, device=dev)
    out, o = [], lead
    for t in tensors:
        v = flat[o:o + t.numel()]
        v.copy_(t)
        out.append(v)
        o += t.numel()
    return out


def check_misaligned(dev):
    sizes = SMALL + (2 * 4096 + 3,)
    runs = []
    for lead in (None, 1):
        src = make_model("cpu", sizes)
        ws = _flat_views(dev, [p.detach() for p in src.parameters()], lead)
        net = Params(ws)
        for p, w in zip(net.parameters(), ws):
            assert p.data_ptr() == w.data_ptr()
        ema = Params(_flat_views(dev, ws, lead))
        opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=ALPHA, max_grad_norm=5.0, **KW)
        zeros = [torch.zeros(n) for n in sizes]
        ms, vs = _flat_views(dev, zeros, lead), _flat_views(dev, zeros, lead)
        for p, m, v in zip(net.parameters(), ms, vs):
            opt.state[p] = {"step": torch.zeros((), dtype=torch.float32, device=dev), "exp_avg": m, "exp_avg_sq": v}
        for s in range(2):
            grads, _ = make_grads(sizes, 500 + s, 50.0 if s == 0 else 0.5)
            gv = _flat_views(dev, grads, lead)
            for p, g in zip(net.parameters(), gv):
                p.grad = g
            for p, m, v, e in zip(net.parameters(), ms, vs, ema.parameters()):
                # lead 1: the tensors start 1, 2, 4097, 8193 and 12290 elements into the bucket, none on a 16-byte boundary
                assert all((t.data_ptr() % 16 == 0) == (lead is None) and t.data_ptr() % 4 == 0 for t in (p, p.grad, m, v, e))
            opt.step()
        runs.append((bits(opt, net, ema), opt.grad_norm.clone(), opt._ctl.clone()))
    assert same_bits(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


# ---- 6. reproducible ----------------------------------------------------------------------------------------------------------------------------

def check_reproducible(dev):
    sizes = SMALL + (9 * 4096 + 5,)
    gs = [make_grads(sizes, 600 + s, 50.0 if s == 0 else 0.5)[0] for s in range(2)]
    a, b = _run(dev, sizes, gs, max_grad_norm=5.0), _run(dev, sizes, gs, max_grad_norm=5.0)
    assert torch.equal(a[0]._ctl, b[0]._ctl) and same_bits(bits(*a), bits(*b))


# ---- 7. parameters without a gradient -----------------------------------------------------------------------------------------------------------

def check_inactive_parameter(dev):
    limit = 5.0
    net, ref = make_model(dev, SMALL), make_model(dev, SMALL)
    ema, ema_ref = copy.deepcopy(net), copy.deepcopy(ref)
    opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=ALPHA, max_grad_norm=limit, **KW)
    opt_ref = torch.optim.AdamW(ref.parameters(), **KW)
    grads, _ = make_grads(SMALL, 700, 50.0)
    grads[1] = None                                   # the 4095-element tensor takes no part: clip_grad_norm_ ignores it too
    n64 = norm64(grads)
    set_grads(net, grads, dev)
    opt.step()
    assert abs(float(opt.grad_norm) - n64) <= NORM_RTOL * n64
    set_grads(ref, grads, dev)
    clip_ref(ref, limit)
    opt_ref.step()
    for i, (p, q, e, e0) in enumerate(zip(net.parameters(), ref.parameters(), ema.parameters(), ema_ref.parameters())):
        assert close(p, q), i
        if i == 1:
            assert torch.equal(p, e0) and torch.equal(e, e0)        # untouched


# ---- 8. bad arguments -------------------------------------------------------------------------------------------------------------------------

def check_bad_arguments(dev):
    net = make_model(dev, SMALL)
    for bad in (-1.0, -1e-3, 0.0, float("nan")):
        try:
            FusedAdamW(net.parameters(), max_grad_norm=bad, **KW)
            raise AssertionError(f"FusedAdamW accepted max_grad_norm={bad}")
        except ValueError as e:
            assert "max_grad_norm" in str(e)
    opt = FusedAdamW(net.parameters(), max_grad_norm=1.0, **KW)
    set_grads(net, make_grads(SMALL, 800, 1.0)[0], dev)
    opt.step()
    opt.param_groups[0]["max_grad_norm"] = -2.0       # a live edit is checked as well, before anything is launched
    before = [p.detach().clone() for p in net.parameters()]
    try:
        opt.step()
        raise AssertionError("FusedAdamW.step accepted a negative max_grad_norm")
    except ValueError:
        pass
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), before))
    opt.param_groups[0]["max_grad_norm"] = 1.0
    L = _lib.lib()
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    from cbim_amd.ops import _stream
    st = _stream(opt._hyper)

    def guarded(table=opt._table, partial=opt._partial, ctl=opt._ctl, hyper=opt._hyper, nblocks=opt._nblocks):
        return L.cbim_adamw_ema_step_guarded(p(table), p(opt._blk_tensor), p(opt._blk_chunk), nblocks, p(hyper), p(partial), p(ctl),
                                             None, None, st)

    def norm(table=opt._table, partial=opt._partial, out=opt._ctl, nblocks=opt._nblocks):
        return L.cbim_grad_norm(p(table), p(opt._blk_tensor), p(opt._blk_chunk), nblocks, p(partial), p(out), st)

    EINVAL = -1
    assert guarded(partial=None) == EINVAL and guarded(ctl=None) == EINVAL and guarded(table=None) == EINVAL
    assert guarded(hyper=None) == EINVAL and guarded(nblocks=0) == EINVAL
    assert norm(partial=None) == EINVAL and norm(out=None) == EINVAL and norm(table=None) == EINVAL and norm(nblocks=0) == EINVAL
    assert all(torch.equal(p_, q) for p_, q in zip(net.parameters(), before))      # a refused call launched nothing
    opt.grad_scale = torch.tensor([65536.0, 1.0], device=dev)
    try:
        opt.step()
        raise AssertionError("FusedAdamW.step accepted a two-element grad_scale")
    except RuntimeError as e:
        assert "grad_scale" in str(e)


# ---- the Python surface around it ----------------------------------------------------------------------------------------------------------------

def check_surface(dev):
    """training.utils.grad_norm (cbim_grad_norm) and max_grad_norm through both get_optimizer entry points."""
    import argparse
    from cbim_amd.training import optim as to, utils as tu
    net = make_model(dev, SMALL + (3 * 4096 + 2,))
    grads, n64 = make_grads(SMALL + (3 * 4096 + 2,), 900, 7.0)
    grads[2] = None
    n64 = norm64(grads)
    set_grads(net, grads, dev)
    gn = tu.grad_norm(net.parameters())
    assert gn.dim() == 0 and gn.device.type == torch.device(dev).type and abs(float(gn) - n64) <= NORM_RTOL * n64
    assert torch.equal(gn, tu.grad_norm(list(net.parameters())))
    args = argparse.Namespace(optimizer="adamw", base_lr=6e-4, betas=[0.9, 0.999], weight_decay=0.05, momentum=0.9)
    for get in (lambda a: tu.get_optimizer(a, net), lambda a: to.get_optimizer(a, net, None)):
        assert get(args).param_groups[0]["max_grad_norm"] is None           # the shipped yaml files have no such key
        args.max_grad_norm = 12
        opt = get(args)
        assert isinstance(opt, FusedAdamW) and opt.param_groups[0]["max_grad_norm"] == 12
        del args.max_grad_norm
    opt.step()
    assert abs(float(opt.grad_norm) - n64) <= NORM_RTOL * n64
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] == 12
    del sd["param_groups"][0]["max_grad_norm"]        # a checkpoint written before the option existed loads, and does not clip
    opt.load_state_dict(sd)
    opt.step()
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0
