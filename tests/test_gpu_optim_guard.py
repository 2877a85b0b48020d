"""-m gpu: the guarded FusedAdamW step (global-norm clipping, the GradScaler protocol, skipped non-finite steps) on the MI355X,
against torch's clip_grad_norm_ + AdamW (checks in tests/optim_guard_checks.py); on top, the step driven by a real
torch.amp.GradScaler as /root/reference/train.py:188-203 drives it, and captured in a graph."""
import copy

import pytest
import torch

from tests import optim_guard_checks as gc

pytestmark = pytest.mark.gpu


def test_parity_with_clip_grad_norm_and_adamw(dev):
    gc.check_parity(dev)


def test_huge_limit_is_no_limit_bit_for_bit(dev):
    gc.check_huge_limit_is_no_limit(dev)


def test_nonfinite_gradient_skips_the_step(dev):
    gc.check_nonfinite_skips(dev)


def test_parity_through_grad_scale_65536(dev):
    gc.check_parity(dev, scale=65536.0)


def test_amp_protocol_attributes(dev):
    gc.check_amp_protocol(dev)


def test_misaligned_base_pointers(dev):
    gc.check_misaligned(dev)


def test_reproducible(dev):
    gc.check_reproducible(dev)


def test_parameter_without_gradient(dev):
    gc.check_inactive_parameter(dev)


def test_bad_arguments(dev):
    gc.check_bad_arguments(dev)


def test_grad_norm_and_get_optimizer_surface(dev):
    gc.check_surface(dev)


def test_through_gradscaler_as_train_py_does(dev):
    """The 8-channel UNet at 32^3 of tests/test_gpu_amp_seam.py under autocast(fp16) + GradScaler: FusedAdamW(max_grad_norm=12)
    through scaler.step alone against torch.optim.AdamW through scaler.unscale_ + clip_grad_norm_ + scaler.step, from the same
    weights and the same scaled gradients (the twin's own backward is replaced by a copy of them, so that the comparison is of
    the two optimizer paths and not of two backward passes).  Then an inf in one gradient element: the step is skipped on the
    device, the scaler halves the scale."""
    import cbim_amd
    from cbim_amd.model.dim3 import UNet
    from cbim_amd.training.losses import DiceLoss
    from cbim_amd.training.optim import FusedAdamW
    assert dev == "cuda"
    cbim_amd.set_compute_dtype(None)
    d = torch.device("cuda", 0)
    torch.manual_seed(11)
    net = UNet(1, 8, scale=[[2, 2, 2]] * 4, kernel_size=[[3, 3, 3]] * 5, num_classes=4, block="BasicBlock", norm="in").to(d)
    twin = copy.deepcopy(net)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 1, 32, 32, 32, generator=g).to(d)
    lab = torch.randint(0, 4, (1, 1, 32, 32, 32), generator=g).to(d)
    criterion = torch.nn.CrossEntropyLoss(weight=torch.tensor([0.5, 1.0, 1.0, 1.0]).to(d))
    criterion_dl = DiceLoss()
    kw = dict(lr=6e-4, betas=(0.9, 0.999), weight_decay=0.05, eps=1e-5)
    optimizer = FusedAdamW(net.parameters(), max_grad_norm=12, **kw)
    optimizer_ref = torch.optim.AdamW(twin.parameters(), **kw)
    scaler, scaler_ref = torch.amp.GradScaler("cuda"), torch.amp.GradScaler("cuda")

    def backward(model, sc):
        with torch.autocast(device_type="cuda", dtype=torch.float16):
            result = model(x)
            loss = criterion(result, lab.squeeze(1)) + criterion_dl(result, lab)
            sc.scale(loss).backward()
        return loss

    # --- first iteration: a finite step -----------------------------------------------------------------------------
    optimizer.zero_grad()
    optimizer_ref.zero_grad()
    backward(net, scaler)
    backward(twin, scaler_ref)
    for p, q in zip(net.parameters(), twin.parameters()):
        q.grad.copy_(p.grad)
    scaled = [p.grad.clone() for p in net.parameters()]
    w_init = [p.detach().clone() for p in net.parameters()]
    scaler.step(optimizer)
    scaler.update()
    scaler_ref.unscale_(optimizer_ref)
    ref_norm = torch.nn.utils.clip_grad_norm_(twin.parameters(), 12)
    scaler_ref.step(optimizer_ref)
    scaler_ref.update()
    assert scaler.get_scale() == 65536.0 and scaler_ref.get_scale() == 65536.0
    assert float(optimizer.skipped_steps) == 0.0
    n64 = gc.norm64([s / 65536.0 for s in scaled])
    print(f"gradscaler step: grad_norm {float(optimizer.grad_norm):.9g} float64 {n64:.9g} torch {float(ref_norm):.9g}")
    assert abs(float(optimizer.grad_norm) - n64) <= gc.NORM_RTOL * n64
    for p, q, s in zip(net.parameters(), twin.parameters(), scaled):
        assert gc.close(p.detach(), q.detach())
        assert torch.equal(p.grad, s)                 # still the scaled, unclipped gradient
    assert all(not torch.equal(p.detach(), w) for p, w in zip(net.parameters(), w_init))      # the step was taken
    # --- second iteration: inf in one gradient element (a data value) -----------------------------------------------------
    optimizer.zero_grad()
    backward(net, scaler)
    list(net.parameters())[3].grad.view(-1)[0] = float("inf")
    w0 = [p.detach().clone() for p in net.parameters()]
    st0 = optimizer.state_dict()["state"][0]["step"].clone()
    scaler.step(optimizer)
    scaler.update()
    assert all(torch.equal(p.detach(), w) for p, w in zip(net.parameters(), w0))
    assert torch.equal(optimizer.state_dict()["state"][0]["step"], st0)
    assert scaler.get_scale() == 32768.0
    assert float(optimizer.skipped_steps) == 1.0


def test_graph_capture_replays_bit_equal(dev):
    """opt.step() with max_grad_norm and persistent grad_scale / found_inf tensors captured on one stream and replayed three times
    from static gradient buffers, one replay with found_inf = 1: bit-equal to the same three eager steps.  That the capture
    succeeds is the evidence that the step has no host round trip."""
    from cbim_amd.training.optim import FusedAdamW
    assert dev == "cuda"
    sizes = gc.SMALL + (2 * 4096 + 3,)
    grads = [gc.make_grads(sizes, 1000 + s, 50.0 if s != 1 else 0.5)[0] for s in range(3)]
    found = (0.0, 1.0, 0.0)

    def build():
        net = gc.make_model(dev, sizes)
        ema = copy.deepcopy(net)
        opt = FusedAdamW(net.parameters(), ema_model=ema, ema_alpha=gc.ALPHA, max_grad_norm=5.0, **gc.KW)
        opt.grad_scale = torch.tensor(65536.0, device=dev)
        opt.found_inf = torch.tensor(1.0, device=dev)
        for p in net.parameters():
            p.grad = torch.ones_like(p)               # the static gradient buffers
        opt.step()                                    # builds the tables; found_inf = 1: skipped, no state is touched
        return opt, net, ema

    def load(opt, net, s):
        for p, gsrc in zip(net.parameters(), grads[s]):
            p.grad.copy_((gsrc * 65536.0).to(dev))
        opt.found_inf.fill_(found[s])

    eager = build()
    for s in range(3):
        load(eager[0], eager[1], s)
        eager[0].step()
    torch.cuda.synchronize()

    opt, net, ema = build()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    for s in range(3):
        load(opt, net, s)
        graph.replay()
    torch.cuda.synchronize()
    assert gc.same_bits(gc.bits(opt, net, ema), gc.bits(*eager))
    assert torch.equal(opt._ctl, eager[0]._ctl)
    assert float(opt.skipped_steps) == 2.0 and float(opt.state_dict()["state"][0]["step"]) == 2.0
