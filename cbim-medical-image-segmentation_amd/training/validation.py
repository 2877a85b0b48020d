"""The reference's evaluation loop (training/validation.py:16-87 ``validation``, :92-209 ``validation_ddp``) with the same
signatures and return values: per foreground class the mean Dice, ASD and HD95 over the volumes whose ground truth holds
the class.  Forward, argmax, Dice counts and the surface distances run on the device; the label volumes never leave it.

The surfel-area table of the distance metrics is an input (``metric.utils.calculate_distance``): ``args.area_table`` when the
caller sets it (256 values or a callable spacing -> table), else ``metric.lookup_tables`` of the host project.
No progress bar and no SimpleITK: neither is part of the computation.

Mirror test-time augmentation and Gaussian window weights are switched on through ``args`` (tta_mirror_axes, window_weight,
window_sigma_scale, tta_batch: see inference/inference3d.py); both loops pick them up through ``get_inference(args)``.
"""
import logging

import numpy as np
import torch

from ..inference.utils import get_inference
from ..metric.utils import calculate_dice_split, calculate_distance


def _device():
    from .. import _lib
    return torch.device("cpu") if _lib.backend() == "emu" else torch.device("cuda", torch.cuda.current_device())


def _predict(net, inference, images, labels, args, device):
    """One volume: (label_pred [D,H,W], labels [D,H,W]) on the device (validation.py:37-51)."""
    if args.dimension == "2d":
        raise NotImplementedError("cbim_amd: 2-D validation is outside the model/dim3 hot path")
    inputs = images.float().to(device)
    labels = labels.to(device)
    if getattr(args, "sliding_window", False):
        _, label_pred = inference(net, inputs, args, return_labels=True)      # argmax from the same pass (validation.py:44)
    else:
        _, label_pred = torch.max(inference(net, inputs, args), dim=1)
    return label_pred.squeeze(0), labels.squeeze(0).squeeze(0)


def _distances(label_pred, labels, spacing, args):
    asd, hd = calculate_distance(label_pred, labels, spacing[0], args.classes, area_table=getattr(args, "area_table", None))
    return np.clip(np.nan_to_num(asd, nan=500), 0, 500), np.clip(np.nan_to_num(hd, nan=500), 0, 500)


def validation(net, dataloader, args):
    net.eval()
    n = args.classes - 1                       # background is not included in validation
    dice_list, ASD_list, HD_list = ([[] for _ in range(n)] for _ in range(3))
    inference = get_inference(args)
    device = _device()
    logging.info("Evaluating")
    with torch.no_grad():
        for (images, labels, spacing) in dataloader:
            label_pred, labels = _predict(net, inference, images, labels.to(torch.int8), args, device)
            label_pred = label_pred.to(torch.int8)
            tmp_ASD_list, tmp_HD_list = _distances(label_pred, labels, spacing, args)
            dice, _, _ = calculate_dice_split(label_pred.reshape(-1, 1), labels.reshape(-1, 1), args.classes)
            dice = dice.cpu().numpy()[1:]
            unique_cls = torch.unique(labels)
            for cls in range(n):
                if cls + 1 in unique_cls:      # only classes that appear in the ground truth are evaluated
                    ASD_list[cls].append(tmp_ASD_list[cls])
                    HD_list[cls].append(tmp_HD_list[cls])
                    dice_list[cls].append(dice[cls])
    out_dice = [np.array(dice_list[cls]).mean() for cls in range(n)]
    out_ASD = [np.array(ASD_list[cls]).mean() for cls in range(n)]
    out_HD = [np.array(HD_list[cls]).mean() for cls in range(n)]
    return np.array(out_dice), np.array(out_ASD), np.array(out_HD)


def validation_ddp(net, dataloader, args):
    from .utils import concat_all_gather
    net.eval()
    dice_list, ASD_list, HD_list, unique_labels_list = [], [], [], []
    inference = get_inference(args)
    device = _device()
    logging.info("Evaluating")
    with torch.no_grad():
        for (images, labels, spacing) in dataloader:
            label_pred, labels = _predict(net, inference, images, labels.long(), args, device)
            tmp_ASD_list, tmp_HD_list = _distances(label_pred, labels, spacing, args)
            tmp_dice_list, _, _ = calculate_dice_split(label_pred.reshape(-1, 1), labels.reshape(-1, 1), args.classes)

            unique_labels = torch.unique(labels).cpu().numpy()
            # padded to a fixed length: all_gather needs the same shape on every rank (validation.py:140-142)
            unique_labels = np.pad(unique_labels, (100 - len(unique_labels), 0), "constant", constant_values=0)
            tmp_dice_list = tmp_dice_list.unsqueeze(0)
            unique_labels = np.expand_dims(unique_labels, axis=0)
            tmp_ASD_list = np.expand_dims(tmp_ASD_list, axis=0)
            tmp_HD_list = np.expand_dims(tmp_HD_list, axis=0)
            if args.distributed:
                tmp_dice_list = concat_all_gather(tmp_dice_list)
                unique_labels = concat_all_gather(torch.from_numpy(unique_labels).to(device)).cpu().numpy()
                tmp_ASD_list = concat_all_gather(torch.from_numpy(tmp_ASD_list).to(device)).cpu().numpy()
                tmp_HD_list = concat_all_gather(torch.from_numpy(tmp_HD_list).to(device)).cpu().numpy()
            tmp_dice_list = tmp_dice_list.cpu().numpy()[:, 1:]      # exclude background
            for idx in range(len(tmp_dice_list)):
                ASD_list.append(tmp_ASD_list[idx])
                HD_list.append(tmp_HD_list[idx])
                dice_list.append(tmp_dice_list[idx])
                unique_labels_list.append(unique_labels[idx])

    # DistributedSampler pads the dataset so that every rank gets the same number of samples: drop the padded ones
    if args.distributed:
        import torch.distributed as dist
        world_size = dist.get_world_size()
        dataset_len = len(dataloader.dataset)
        padding_size = 0 if (dataset_len % world_size) == 0 else world_size - (dataset_len % world_size)
        for _ in range(padding_size):
            ASD_list.pop()
            HD_list.pop()
            dice_list.pop()
            unique_labels_list.pop()

    n = args.classes - 1
    out_dice, out_ASD, out_HD = ([[] for _ in range(n)] for _ in range(3))
    for idx in range(len(dice_list)):
        for cls in range(n):
            if cls + 1 in unique_labels_list[idx]:
                out_dice[cls].append(dice_list[idx][cls])
                out_ASD[cls].append(ASD_list[idx][cls])
                out_HD[cls].append(HD_list[idx][cls])
    return (np.array([np.array(v).mean() for v in out_dice]), np.array([np.array(v).mean() for v in out_ASD]),
            np.array([np.array(v).mean() for v in out_HD]))
