"""prediction.py of the reference (/root/reference/prediction.py:35-224) with the volume resident on the device from the raw
float32 array to the uint8 label map on the original grid.  File I/O stays with the caller: where the reference passes a SimpleITK
image, these functions take the array plus its geometry ``(spacing, origin, direction)`` in SimpleITK's x, y, z order (see
inference/resample.py for the axis-order rule).

    model_list = init_model(args)                                   # args.load: checkpoint paths, args.ema
    label = predict_volume(model_list, img, spacing, args)          # uint8 [D, H, W] on the grid of img

Differences to the reference that a caller can see: ``prediction`` returns uint8 (the reference returns the int64 indices of
torch.max and casts them to uint8 in postprocess); 2-D raises NotImplementedError like ``model.utils.get_model``.
"""
import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .inference import inference3d
from .inference.components import filter_components
from .inference.resample import (IDENTITY, _device, percentile, resample_label_to_ref, resample_probabilities_to_ref,
                                 resample_xyz_axis)
from .inference.utils import get_inference
from .model.utils import get_model
from .ops import _dev_ok, _p, _stream


def _check_dim(args):
    if args.dimension == "2d":
        raise NotImplementedError("cbim_amd: 2-D prediction is outside the model/dim3 hot path")
    if args.dimension != "3d":
        raise ValueError("Error in image dimension")


def ensemble_finalize(prob_sum, counter, total, labels, first, last):
    """One model's share of the ensemble tail (cbim_ensemble_finalize): prob_sum [K, D, H, W] summed window probabilities (left as
    they are), counter [D, H, W] or None, total [K, D, H, W] running float32 sum (None for a one-model ensemble), labels uint8
    [D, H, W], written on the last model."""
    _dev_ok(prob_sum, counter, total, labels)
    K = int(prob_sum.shape[0])
    S = prob_sum.numel() // K
    _lib.check(_lib.lib().cbim_ensemble_finalize(_p(prob_sum), _p(counter), _p(total), _p(labels), K, S, int(first), int(last),
                                                 _stream(prob_sum)), "ensemble_finalize")


def prediction(model_list, tensor_img, args, return_total=False):
    """Ensemble prediction of one preprocessed volume [D, H, W] (prediction.py:35-62): every model's window-averaged
    probabilities are summed in list order in float32 and the first maximum over the classes is the label.  The sliding-window
    accumulators feed the ensemble kernel directly; no model's probabilities are written out on their own.  The compute dtype is
    the engine's (``cbim_amd.set_compute_dtype``).  The optional keys args.tta_mirror_axes, args.window_weight,
    args.window_sigma_scale and args.tta_batch (mirror test-time augmentation and Gaussian window weights, see
    inference/inference3d.py) apply to every model; the count handed to the ensemble kernel is then the sum of weights.
    Returns uint8 [D, H, W] (with return_total also the summed probabilities)."""
    _check_dim(args)
    get_inference(args)
    inference3d._label_gate()
    img = torch.as_tensor(tensor_img)
    img = img.to(_device(img)).float()
    if img.dim() != 3:
        raise ValueError(f"prediction takes one [D, H, W] volume, not {tuple(img.shape)}")
    D, H, W = map(int, img.shape)
    x = img[None, None].contiguous()
    M = len(model_list)
    if M == 0:
        raise ValueError("prediction needs at least one model")
    total = labels = None
    with torch.no_grad():
        for m, model in enumerate(model_list):
            if args.sliding_window:
                acc, counter, _ = inference3d._sliding_window_accumulate(model, x, args)
                acc, counter = acc[0], counter[0, 0]
            else:
                acc, counter = inference3d.inference_whole_image(model, x, args)[0], None    # under TTA already the variant mean
            if total is None and (M > 1 or return_total):
                total = torch.empty_like(acc)
            if labels is None:
                labels = torch.empty(acc.shape[1:], dtype=torch.uint8, device=acc.device)
            ensemble_finalize(acc, counter, total, labels, m == 0, m == M - 1)
    labels = labels[:D, :H, :W]                  # a volume smaller than one window was padded at the far ends
    if return_total:
        return labels, total[:, :D, :H, :W]
    return labels


def pad_to_training_size(np_img, args):
    """prediction.py:65-122 for a numpy array or a tensor: an axis shorter than args.training_size is zero-padded on both sides by
    (training_size + 2 - n) // 2 (the reference's `+2`).  Returns (padded, [z_start, z_end, y_start, y_end, x_start, x_end])."""
    _check_dim(args)
    shape = tuple(int(v) for v in np_img.shape)
    pads, idx = [], []
    for a in range(3):
        n = shape[a]
        if n < args.training_size[a]:
            diff = (args.training_size[a] + 2 - n) // 2
            pads.append((diff, diff))
            idx += [diff, diff + n]
        else:
            pads.append((0, 0))
            idx += [0, n]
    if torch.is_tensor(np_img):
        if any(p != (0, 0) for p in pads):
            np_img = F.pad(np_img, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    else:
        for a in range(3):                        # axis by axis like the reference (np.pad returns a copy each time)
            if pads[a] != (0, 0):
                np_img = np.pad(np_img, [pads[b] if b == a else (0, 0) for b in range(3)])
    return np_img, idx


def unpad_img(np_pred, original_idx, args):
    """prediction.py:127-138."""
    _check_dim(args)
    z_start, z_end, y_start, y_end, x_start, x_end = original_idx
    return np_pred[z_start:z_end, y_start:y_end, x_start:x_end]


def _normalize(img, normalize):
    if normalize is None or normalize == "none":
        return img
    if normalize == "percentile":                 # prediction.py:169-171
        max98 = float(percentile(img, 98))
        return torch.clamp(img, 0.0, max98) / max98
    if isinstance(normalize, dict):               # the recipe of the CT datasets: clip, subtract the mean, divide by the std
        if "clip" in normalize:
            img = torch.clamp(img, float(normalize["clip"][0]), float(normalize["clip"][1]))
        if "mean" in normalize:
            img = img - float(normalize["mean"])
        if "std" in normalize:
            img = img / float(normalize["std"])
        return img
    if callable(normalize):
        return normalize(img)
    raise ValueError(f"unknown normalisation {normalize!r}")


def preprocess(img, spacing, target_spacing, args, normalize="percentile"):
    """prediction.py:141-177 on a device tensor: resample to the training spacing (cubic B-spline) when the spacing differs,
    normalise the intensities, pad to the training size.  img raw [D, H, W]; spacing / target_spacing (x, y, z).
    normalize: 'percentile' (the reference's default recipe), {'clip': (lo, hi), 'mean': m, 'std': s}, a callable, or None.
    Returns (tensor, original_idx)."""
    _check_dim(args)
    img = torch.as_tensor(img)
    img = img.to(_device(img)).float()
    if tuple(spacing) != tuple(target_spacing):
        img = resample_xyz_axis(img, spacing, target_spacing, interp="bspline")
    img = _normalize(img, normalize)
    return pad_to_training_size(img, args)


def _filter_components(label, components):
    unknown = set(components) - {"keep_largest", "min_size", "connectivity"}
    if unknown:
        raise ValueError(f"components: unknown keys {sorted(unknown)}")
    return filter_components(label.contiguous(), **components)


def postprocess(label, original_idx, geom, ref_geom, ref_shape, args, components=None, probabilities=None, counter=None):
    """prediction.py:180-199: cut the padding off and, when the training spacing is not the scan's, bring the label map back onto
    the scan's grid by nearest neighbour.  geom: the geometry of the label map (None: args.target_spacing with the scan's origin
    and direction, as the reference sets it); ref_geom / ref_shape: the scan's.  components (not in the reference): None, or
    {"keep_largest": ..., "min_size": ..., "connectivity": ...} for ``inference.components.filter_components``, applied last, on
    the scan's own grid.  probabilities (not in the reference): the class probabilities [K, D, H, W] of the padded volume
    (``prediction(..., return_total=True)``, or the sliding-window sums with their ``counter`` [D, H, W]); when the spacings
    differ the label map on the scan's grid is then the first maximum of the trilinearly interpolated probabilities
    (``inference.resample.resample_probabilities_to_ref``, original_idx as its crop) and `label` may be None; with equal
    spacings `label` — their argmax already — is used as always.  Returns uint8 [*ref_shape] on the device."""
    _check_dim(args)
    if geom is None:
        geom = (tuple(args.target_spacing), ref_geom[1], ref_geom[2])
    if probabilities is not None and tuple(geom[0]) != tuple(ref_geom[0]):
        label = resample_probabilities_to_ref(probabilities, geom, ref_geom, ref_shape, counter=counter, crop=original_idx)
    else:
        label = unpad_img(torch.as_tensor(label).to(torch.uint8), original_idx, args)
        if tuple(geom[0]) != tuple(ref_geom[0]):
            label = resample_label_to_ref(label, geom, ref_geom, ref_shape)
    if components is not None:
        label = _filter_components(label, components)
    return label


def _window_sums(model, tensor_img, args):
    """One model's probabilities of a preprocessed volume as prediction() hands them to the ensemble kernel: (sums [K, D, H, W],
    window count [D, H, W] or None), both of the volume padded up to one window, not yet divided."""
    _check_dim(args)
    get_inference(args)
    inference3d._label_gate()
    img = torch.as_tensor(tensor_img)
    x = img.to(_device(img)).float()[None, None].contiguous()
    with torch.no_grad():
        if args.sliding_window:
            acc, counter, _ = inference3d._sliding_window_accumulate(model, x, args)
            return acc[0], counter[0, 0]
        return inference3d.inference_whole_image(model, x, args)[0], None


def predict_volume(model_list, img, spacing, args, origin=(0.0, 0.0, 0.0), direction=IDENTITY, normalize="percentile",
                   components=None, resample="nearest"):
    """The loop body of the reference's __main__ (prediction.py:277-286) for one raw scan: preprocess, prediction, postprocess.
    img float32 [D, H, W], spacing (x, y, z); args.target_spacing is the training spacing.  Returns the uint8 label map on the
    scan's own grid, on the device; with ``components`` (see postprocess) after connected-component clean-up on that grid.
    resample: how the result comes back onto the scan's grid when the spacings differ — 'nearest' (the reference: the label map
    by nearest neighbour) or 'probabilities' (not in the reference: the class probabilities are interpolated trilinearly onto
    the scan's grid and the argmax is taken there, in one kernel; a single model's sliding-window sums and counts go to it as
    they are, an ensemble's through ``prediction(..., return_total=True)``)."""
    if resample not in ("nearest", "probabilities"):
        raise ValueError(f"predict_volume: resample is 'nearest' or 'probabilities', not {resample!r}")
    ref_geom = (tuple(spacing), tuple(origin), tuple(direction))
    ref_shape = tuple(int(v) for v in img.shape)
    tensor_img, original_idx = preprocess(img, spacing, args.target_spacing, args, normalize=normalize)
    if resample == "nearest" or tuple(args.target_spacing) == tuple(spacing):
        label = prediction(model_list, tensor_img, args)
        return postprocess(label, original_idx, None, ref_geom, ref_shape, args, components=components)
    if len(model_list) == 1:
        prob, counter = _window_sums(model_list[0], tensor_img, args)
    else:
        prob, counter = prediction(model_list, tensor_img, args, return_total=True)[1], None
    return postprocess(None, original_idx, None, ref_geom, ref_shape, args, components=components, probabilities=prob, counter=counter)


def init_model(args):
    """prediction.py:204-224: one model per checkpoint of args.load, EMA weights when args.ema."""
    device = _device(None)
    model_list = []
    for ckp_path in args.load:
        model = get_model(args)
        pth = torch.load(ckp_path, map_location=torch.device("cpu"))
        if args.ema:
            model.load_state_dict(pth["ema_model_state_dict"])
        else:
            model.load_state_dict(pth["model_state_dict"])
        model.to(device)
        model_list.append(model)
        print(f"Model loaded from {ckp_path}")
    return model_list
