"""Record what the two "oracle vs live reference" tests of tests/test_oracle.py compare against, by EXECUTING THE REAL
REFERENCE on CPU, so that they run where the reference tree is not mounted.  Run in the build container only:

    python tests/golden/make_golden_live.py

  live_unet_b4.npz : UNet(1, 4, num_classes=5, BasicBlock, norm in) under torch.manual_seed(11): the checksum of its weights
                     (the oracle's constructor redraws them from the seed), input, labels, logits at every second voxel of
                     each axis and DiceLoss in its three reductions (test_oracle_vs_live_reference)
  live_vnet_b4.npz : VNet(2, 3, baseChans=4) in eval mode under torch.manual_seed(23): the checksum of its state_dict (the
                     engine's constructor redraws it from the seed), input and logits (test_vnet_oracle_vs_live_reference)
No reference source is copied; only tensors it produced.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.unet_ref import state_dict_checksum


def unet_case():
    """the draws and calls of test_oracle_vs_live_reference, in its order"""
    from tests.golden.make_golden import import_reference
    UNet, DiceLoss = import_reference()
    torch.manual_seed(11)
    ks = [[3, 3, 3]] * 5
    sc = [[2, 2, 2]] * 4
    net = UNet(1, 4, scale=sc, kernel_size=ks, num_classes=5, block="BasicBlock", norm="in")
    x = torch.randn(1, 1, 32, 32, 32)
    lab = torch.randint(0, 5, (1, 1, 32, 32, 32))
    out = dict(sd_checksum=np.float64(state_dict_checksum(net.state_dict())), keys=np.array(list(net.state_dict())))
    ref = net(x).detach()      # (after the checksum: the forward moves the running statistics of VNet's batch norms)
    out.update(x=x.numpy(), label=lab.numpy().astype(np.int8), logits_s2=ref[..., ::2, ::2, ::2].numpy(),
               dice=np.float64(DiceLoss()(ref, lab)), dice_sum=np.float64(DiceLoss(size_average=False)(ref, lab)),
               dice_none=DiceLoss(reduce=False)(ref, lab).detach().numpy())
    return out


def vnet_case():
    """the draws and calls of test_vnet_oracle_vs_live_reference, in its order"""
    from tests.golden.make_golden import import_reference
    import_reference()
    VNet = importlib.import_module("model.dim3.vnet").VNet
    torch.manual_seed(23)
    sc = [[2, 2, 2]] * 4
    net = VNet(2, 3, scale=sc, baseChans=4).eval()
    x = torch.randn(2, 2, 16, 16, 32)
    out = dict(sd_checksum=np.float64(state_dict_checksum(net.state_dict())), keys=np.array(list(net.state_dict())))
    ref = net(x).detach()      # (after the checksum: the forward moves the running statistics of VNet's batch norms)
    out.update(x=x.numpy(), logits=ref.numpy())
    return out


if __name__ == "__main__":
    for name, fn in (("live_unet_b4", unet_case), ("live_vnet_b4", vnet_case)):
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **fn())
        print(path, os.path.getsize(path))
