"""Loss modules with the reference's call surface (/root/reference/training/losses.py:8-98,
/root/reference/train.py:80-81,212), computed by the fused HIP Dice+CE and focal kernels, and the top-k cross entropy (hard-example mining) on the same kernel family."""
import torch
import torch.nn as nn

from .. import functional as Fn


class DiceLoss(nn.Module):
    """DiceLoss()(preds[B,C,...], targets[B,1,...] int64) — losses.py:8-58 (size_average, reduce
    defaults; alpha/beta constructor arguments are overwritten by the adaptive alpha, :38-42)."""

    def __init__(self, alpha=0.5, beta=0.5, size_average=True, reduce=True):
        super().__init__()
        self.size_average, self.reduce = size_average, reduce

    def forward(self, preds, targets):
        with torch.autocast(device_type=preds.device.type, enabled=False):
            if not self.reduce:                    # losses.py:48-50: the per-class vector 1 - dice_c
                return Fn.DicePerClassFn.apply(preds, targets)
            loss = Fn.DiceCEFn.apply(preds, targets, None)[1]
            # losses.py:52-56: the sum over classes, divided by C only under size_average
            return loss if self.size_average else loss * int(preds.shape[1])


class DiceCELoss(nn.Module):
    """criterion(result, label.squeeze(1)) + criterion_dl(result, label) of train.py:212 in one
    pass; ``weight`` is the class weight of nn.CrossEntropyLoss (train.py:80)."""

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else torch.as_tensor(weight, dtype=torch.float32))

    def forward(self, logits, label):
        with torch.autocast(device_type=logits.device.type, enabled=False):
            return Fn.DiceCEFn.apply(logits, label, self.weight)[2]


def _focal_args(class_num, alpha, gamma):
    gamma = float(gamma)
    if not gamma >= 0.0 or gamma == float("inf"):
        raise ValueError(f"gamma must be a finite number >= 0 (got {gamma})")
    if alpha is not None:
        alpha = torch.as_tensor(alpha, dtype=torch.float32).detach().clone().reshape(-1)
        if class_num is None or int(alpha.numel()) != int(class_num):
            raise ValueError(f"alpha has {int(alpha.numel())} entries for class_num = {class_num}")
    return alpha, gamma


class FocalLoss(nn.Module):
    """FocalLoss(class_num, alpha, gamma, size_average)(preds[B,C,...], targets[B,...] int64) — losses.py:60-98: the mean (or the
    sum) over all voxels of -alpha[y] (1 - p)^gamma log p.  The target has NO channel axis here (the reference's convention for
    this module, unlike DiceLoss); a [B,1,...] target is viewed as [B,...]."""

    def __init__(self, class_num, alpha=None, gamma=2, size_average=True):
        super().__init__()
        alpha, self.gamma = _focal_args(class_num, alpha, gamma)
        self.class_num, self.size_average = int(class_num), size_average
        self.register_buffer("alpha", alpha)

    def forward(self, preds, targets):
        if int(preds.shape[1]) != self.class_num:
            raise ValueError(f"FocalLoss(class_num={self.class_num}) called with {int(preds.shape[1])} channels")
        with torch.autocast(device_type=preds.device.type, enabled=False):
            out = Fn.FocalFn.apply(preds, targets, self.alpha, self.gamma, False)
            return out[1] if self.size_average else out[0]


class DiceFocalLoss(nn.Module):
    """FocalLoss(class_num, alpha, gamma)(logits, label.squeeze(1)) + DiceLoss()(logits, label) in one pass: the focal + Dice
    recipe as a drop-in for DiceCELoss (label [B,1,...])."""

    def __init__(self, class_num=None, alpha=None, gamma=2):
        super().__init__()
        alpha, self.gamma = _focal_args(class_num, alpha, gamma)
        self.class_num = None if class_num is None else int(class_num)
        self.register_buffer("alpha", alpha)

    def forward(self, logits, label):
        if self.class_num is not None and int(logits.shape[1]) != self.class_num:
            raise ValueError(f"DiceFocalLoss(class_num={self.class_num}) called with {int(logits.shape[1])} channels")
        with torch.autocast(device_type=logits.device.type, enabled=False):
            out = Fn.FocalFn.apply(logits, label, self.alpha, self.gamma, True)
            return out[4]


def _topk_args(weight, k):
    k = float(k)
    if not 0.0 < k <= 100.0:
        raise ValueError(f"k must lie in (0, 100] percent (got {k})")
    return (None if weight is None else torch.as_tensor(weight, dtype=torch.float32).detach().clone().reshape(-1)), k


class TopKLoss(nn.Module):
    """TopKLoss(weight, k)(preds[B,C,...], targets[B,...] or [B,1,...] int64): nn.CrossEntropyLoss(weight, reduction="none")
    averaged over the hardest ``k`` percent of all voxels of the batch — K = int(B*S*k/100) of them, the sum of the K largest
    terms divided by K (nnU-Net's TopKLoss; k = 100 is the mean cross entropy).  Voxels tied at the threshold share evenly."""

    def __init__(self, weight=None, k=10):
        super().__init__()
        weight, self.k = _topk_args(weight, k)
        self.register_buffer("weight", weight)

    def forward(self, preds, targets):
        with torch.autocast(device_type=preds.device.type, enabled=False):
            return Fn.TopKCEFn.apply(preds, targets, self.weight, self.k, False)[1]


class DiceTopKLoss(nn.Module):
    """TopKLoss(weight, k)(logits, label) + DiceLoss()(logits, label) in one pass (nnU-Net's DC_and_topk_loss recipe) as a drop-in
    for DiceCELoss (label [B,1,...]; summed over the outputs of a deep-supervision net like it)."""

    def __init__(self, weight=None, k=10):
        super().__init__()
        weight, self.k = _topk_args(weight, k)
        self.register_buffer("weight", weight)

    def forward(self, logits, label):
        with torch.autocast(device_type=logits.device.type, enabled=False):
            return Fn.TopKCEFn.apply(logits, label, self.weight, self.k, True)[4]


def check_labels(reset: bool = True) -> int:
    """Call once per epoch / validation pass: raises IndexError if any label outside [0, classes) reached the loss since the last
    call (the per-step check of the first calls is not repeated every step: it is a device synchronisation)."""
    return Fn.check_labels(reset)
