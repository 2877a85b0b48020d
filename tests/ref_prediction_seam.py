"""Subprocess helper of tests/test_prediction_emu.py: the reference's own prediction.py (init_model, prediction — its text
unmodified) driven through the seam, with `model.utils.get_model` and `inference.utils.get_inference` resolved to the engine's.
A two-checkpoint ensemble is saved, loaded by the reference's init_model and predicted by the reference's prediction(); the label
map must be the engine's own.  Runs on the host-side executor, where `.cuda()` is the identity.
    python tests/ref_prediction_seam.py <reference checkout> <scratch dir>"""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def main():
    ref, scratch = sys.argv[1], sys.argv[2]
    sys.path.insert(0, ROOT)
    import torch
    import cbim_amd
    from cbim_amd import _lib
    from cbim_amd import prediction as engine_prediction
    from cbim_amd.inference import utils as amd_inference_utils
    from cbim_amd.model import utils as amd_model_utils
    assert _lib.backend() == "emu"

    sys.path.insert(0, ref)
    for name, attr, fn in (("model", "get_model", amd_model_utils.get_model),
                           ("inference", "get_inference", amd_inference_utils.get_inference)):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(ref, name)]
        sys.modules[name] = pkg
        shim = types.ModuleType(name + ".utils")
        setattr(shim, attr, fn)
        sys.modules[name + ".utils"] = shim
    for name in ("SimpleITK", "skimage", "skimage.measure", "torchvision", "torchvision.transforms"):
        sys.modules.setdefault(name, _Stub(name))
    import training  # noqa: F401  (the reference's package)
    ds = types.ModuleType("training.dataset.utils")
    ds.get_dataset = lambda args, mode, **kw: None
    dpk = types.ModuleType("training.dataset")
    dpk.__path__ = []
    sys.modules["training.dataset"] = dpk
    sys.modules["training.dataset.utils"] = ds
    import matplotlib
    matplotlib.use("Agg")
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    import prediction as ref_prediction                      # the reference's prediction.py
    assert os.path.samefile(ref_prediction.__file__, os.path.join(ref, "prediction.py"))

    args = argparse.Namespace(dimension="3d", model="unet", in_chan=1, base_chan=4, classes=3, down_scale=[[1, 2, 2]] * 4,
                              norm="in", kernel_size=[[3, 3, 3]] * 5, block="BasicBlock", training_size=[4, 16, 16],
                              window_size=[4, 16, 16], sliding_window=True, ema=True, load=[])
    for k, seed in enumerate((31, 32)):
        torch.manual_seed(seed)
        net = amd_model_utils.get_model(args)
        torch.manual_seed(seed + 100)
        other = amd_model_utils.get_model(args)              # what must NOT be loaded when args.ema is set
        path = os.path.join(scratch, f"ckpt{k}.pth")
        torch.save({"ema_model_state_dict": net.state_dict(), "model_state_dict": other.state_dict()}, path)
        args.load.append(path)
    gen = torch.Generator().manual_seed(3)
    img = torch.rand((6, 16, 24), generator=gen)
    cbim_amd.set_compute_dtype("fp32")
    models = ref_prediction.init_model(args)
    assert len(models) == 2
    got = ref_prediction.prediction(models, img, args)       # reference loop: engine inference, torch add, torch.max
    want = engine_prediction.prediction(engine_prediction.init_model(args), img, args)
    assert tuple(got.shape) == (6, 16, 24) and torch.equal(got.to(torch.uint8), want)
    args.ema = False
    other = engine_prediction.prediction(engine_prediction.init_model(args), img, args)
    assert not torch.equal(other, want), "ema_model_state_dict and model_state_dict must select different weights"
    print("PREDICTION-SEAM-OK", int((want > 0).sum()))


if __name__ == "__main__":
    main()
