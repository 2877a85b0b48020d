"""Timing of the guarded FusedAdamW step (cbim_adamw_ema_step_guarded: global-norm clipping, GradScaler protocol, skip of a
non-finite step) on the GPU next to the unguarded step and the compositions it replaces:
    python tools/bench_optim.py [--reps 30] [--warmup 5] [--out profiles/optim.json]
Parameter sets: the ResUNet headline model of bench.py (UNet base 32, 16 classes: 45 tensors, 40.56 M parameters) and MedFormer with
the AMOS yaml (278 tensors), fp32, no EMA model (as bench.py runs them), random gradients.  Every variant owns its parameters,
gradients and moments (four tensors per parameter, far more than the Infinity Cache holds) and is one optimizer step:
  unguarded            FusedAdamW().step()                                          k_optim_tick + k_adamw_ema, as before
  guarded_clip         FusedAdamW(max_grad_norm=12).step()                          k_grad_sumsq + k_grad_ctl + guarded k_adamw_ema
  guarded_clip_scale   the same with grad_scale = 65536 / found_inf = 0 attributes  the same three kernels
  clip_then_unguarded  torch.nn.utils.clip_grad_norm_(params, 12); FusedAdamW().step()        what guarded_clip replaces
  scaler_generic       GradScaler.step + update on a FusedAdamW WITHOUT the protocol (the optimizer before this option existed):
                       foreach unscale that rewrites every gradient, found_inf.item(), the unguarded step     what the protocol replaces
  scaler_protocol      GradScaler.step + update on FusedAdamW(max_grad_norm=12): torch's own inf check over the gradients, then the
                       guarded step, no host round trip
The variants alternate inside every repetition (same process), each timed window is BATCH consecutive steps between one pair of HIP
events right after an untimed step of the same variant, and the figure is the median over --reps repetitions after --warmup, per
step, host side of the step included (at 278 tensors the Python of step() and of torch's foreach calls is a large part of it).
GB/s is algorithm bytes over that time — not a kernel's rate: the unguarded step reads p, g, m, v and writes p, m, v = 28 bytes per
parameter, the guarded step reads g once more = 32 bytes per parameter.  scaler_generic / clip_then_unguarded are charged the
guarded step's 32 bytes (the work they stand for), whatever they actually move.
The GradScaler variants run at scale 1 (init_scale=1.0): the same kernels and bytes as at 65536, and the in-place unscale of
scaler_generic then leaves the gradients as they are instead of shrinking them by 2^16 per step.
grad_norm of the guarded step is compared with the float64 norm of the same gradients at both sets, and the worst case of the parity
case of tests/optim_guard_checks.py is recorded next to the bound derived there."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import cbim_amd  # noqa: E402,F401
from cbim_amd.training.optim import FusedAdamW  # noqa: E402

MEDFORMER_AMOS = dict(base_chan=32, map_size=[4, 4, 4], conv_block="BasicBlock", conv_num=[2, 1, 0, 0, 0, 1, 2, 2],
                      trans_num=[0, 1, 4, 6, 4, 1, 0, 0], chan_num=[64, 128, 256, 320, 256, 128, 64, 32],
                      num_heads=[1, 4, 8, 10, 8, 4, 1, 1], fusion_depth=2, fusion_dim=320, fusion_heads=10,
                      expansion=4, attn_drop=0., proj_drop=0., proj_type="depthwise", norm="in", act="relu",
                      kernel_size=[[3, 3, 3]] * 5, scale=[[2, 2, 2]] * 4, aux_loss=True)  # config/amos_ct/medformer_3d.yaml
KW = dict(lr=6e-4, betas=(0.9, 0.999), weight_decay=0.05, eps=1e-5)
MAX_NORM = 12.0
BATCH = 10
BYTES_UNGUARDED, BYTES_GUARDED = 28, 32


class NoProtocolAdamW(FusedAdamW):
    """FusedAdamW as GradScaler saw it before the protocol: the scaler unscales, syncs on found_inf and calls a plain step()."""
    _step_supports_amp_scaling = False


def shapes_of(name):
    from cbim_amd.model.dim3 import MedFormer, UNet
    torch.manual_seed(2023)
    if name == "medformer":
        net = MedFormer(1, 16, **MEDFORMER_AMOS)
    else:
        net = UNet(1, 32, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=16, block="BasicBlock", norm="in")
    return [p.detach().clone() for p in net.parameters() if p.requires_grad]


def one_set(name, reps, warmup):
    init = shapes_of(name)
    gen = torch.Generator(device="cuda").manual_seed(7)

    def params():
        ps = [torch.nn.Parameter(t.cuda()) for t in init]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen, device="cuda") * 1e-2
        return ps

    variants = {}
    ps = params()
    opt = FusedAdamW(ps, **KW)
    variants["unguarded"] = opt.step
    ps = params()
    guarded = FusedAdamW(ps, max_grad_norm=MAX_NORM, **KW)
    guarded_params = ps
    variants["guarded_clip"] = guarded.step
    ps = params()
    opt = FusedAdamW(ps, max_grad_norm=MAX_NORM, **KW)
    opt.grad_scale, opt.found_inf = torch.tensor(65536.0, device="cuda"), torch.tensor(0.0, device="cuda")
    variants["guarded_clip_scale"] = opt.step
    ps = params()
    opt = FusedAdamW(ps, **KW)

    def clip_then(ps=ps, opt=opt):
        torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()

    variants["clip_then_unguarded"] = clip_then
    for key, cls, kw in (("scaler_generic", NoProtocolAdamW, {}), ("scaler_protocol", FusedAdamW, {"max_grad_norm": MAX_NORM})):
        ps = params()
        opt = cls(ps, **KW, **kw)
        scaler = torch.amp.GradScaler("cuda", init_scale=1.0, growth_interval=1 << 30)
        scaler.scale(torch.zeros((), device="cuda"))            # creates the scale tensor, as the first scaler.scale(loss) does

        def through_scaler(opt=opt, scaler=scaler):
            scaler.step(opt)
            scaler.update()

        variants[key] = through_scaler
    # the norm the guarded step reports against float64, on this set's gradients
    guarded.step()
    n64 = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in guarded_params)))
    norm_err = abs(float(guarded.grad_norm) - n64) / n64
    ms = {k: [] for k in variants}
    for it in range(reps + warmup):
        for k, f in variants.items():
            f()                  # untimed: every timed window follows a step of its own variant
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                f()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[k].append(e0.elapsed_time(e1) / BATCH)
    n = sum(t.numel() for t in init)
    res = {"tensors": len(init), "parameters": n, "blocks": guarded._nblocks, "unguarded_algorithm_bytes": n * BYTES_UNGUARDED,
           "guarded_algorithm_bytes": n * BYTES_GUARDED, "grad_norm": float(guarded.grad_norm), "grad_norm_float64": n64,
           "grad_norm_rel_err": norm_err, "skipped_steps": float(guarded.skipped_steps)}
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in variants:
        nbytes = n * (BYTES_UNGUARDED if k == "unguarded" else BYTES_GUARDED)
        res[f"{k}_ms"] = round(med[k], 4)
        res[f"{k}_min_max_ms"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
        res[f"{k}_GBps"] = round(nbytes / med[k] / 1e6, 1)
    res["guarded_clip_over_unguarded"] = round(med["guarded_clip"] / med["unguarded"], 4)
    res["clip_then_unguarded_over_guarded_clip"] = round(med["clip_then_unguarded"] / med["guarded_clip"], 3)
    res["scaler_generic_over_guarded_clip_scale"] = round(med["scaler_generic"] / med["guarded_clip_scale"], 3)
    res["scaler_generic_over_scaler_protocol"] = round(med["scaler_generic"] / med["scaler_protocol"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sets", default="resunet,medformer")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: needs a GPU")
    res = {"bench": "optim", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "batch": BATCH,
           "max_grad_norm": MAX_NORM,
           "timed": f"{BATCH} consecutive optimizer steps between one pair of HIP events, per step, host side included; median; "
                    "variants alternate inside each repetition", "sets": {}}
    for name in a.sets.split(","):
        res["sets"][name] = one_set(name, a.reps, a.warmup)
    try:
        from tests import optim_guard_checks as gc
        res["parity_case_grad_norm_worst_rel_err"] = max(gc.check_parity("cuda"), gc.check_parity("cuda", scale=65536.0))
        res["grad_norm_rel_err_bound"] = gc.NORM_RTOL
    except ImportError:
        pass
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
