"""Whole-image and sliding-window inference with the reference's call surface
(/root/reference/inference/inference3d.py:8-99).  The network forward runs on the HIP kernels; the per-window
softmax + accumulate + count and the final normalisation are fused kernels (csrc/inference_kernels.hip).

Beyond the reference, four optional ``args`` attributes (read with getattr; absent or at their defaults the code path, the
launches and the bits are the reference-shaped ones above):

    tta_mirror_axes     subset of (0, 1, 2) = (D, H, W): the probabilities are averaged over ALL subsets of these axes flipped
                        (2^n variants, ascending flip code, identity first)                                      default ()
    window_weight       'constant' | 'gaussian': a window's centre counts more than its rim (sliding window only)
                                                                                                          default 'constant'
    window_sigma_scale  Gaussian sigma as a fraction of the window length per axis                            default 0.125
    tta_batch           variants per forward pass, 1 .. number of variants                              default all variants

A flip code is 3 bits: bit 0 reverses D, bit 1 H, bit 2 W.  Per window: one cbim_window_gather_mirror, ceil(variants /
tta_batch) forwards and one cbim_softmax_accumulate_tta per forward (variants summed in ascending order); the counter becomes
the sum of weights, which cbim_prob_finalize / cbim_ensemble_finalize divide by as before."""
import ctypes as C

import numpy as np
import torch
import torch.nn.functional as F

from .. import _lib
from ..ops import _dev_ok, _p, _stream
from .utils import split_idx


def _logits(net, x):
    pred = net(x)
    if isinstance(pred, (tuple, list)):     # deep-supervision nets return [out, aux_out]
        pred = pred[0]
    return pred.contiguous().float()


def _accumulate(logits, acc, counter, d0, h0, w0):
    _dev_ok(logits, acc, counter)
    B, K, wd, wh, ww = map(int, logits.shape)
    _, _, D, H, W = map(int, acc.shape)
    _lib.check(_lib.lib().cbim_softmax_accumulate(_p(logits), _p(acc), _p(counter), B, K, wd, wh, ww, D, H, W, d0, h0, w0,
                                                  _stream(logits)), "softmax_accumulate")


def mirror_variants(axes):
    """Flip codes of mirror test-time augmentation over `axes`, a subset of (0, 1, 2) = (D, H, W): every subset of the axes,
    2^n codes in ascending order, the identity (0) first."""
    axes = [int(a) for a in axes]
    if any(a not in (0, 1, 2) for a in axes):
        raise ValueError(f"tta_mirror_axes: axes are 0, 1, 2 (D, H, W), not {axes}")
    if len(set(axes)) != len(axes):
        raise ValueError(f"tta_mirror_axes: duplicate axis in {axes}")
    mask = sum(1 << a for a in axes)
    return [c for c in range(8) if c & ~mask == 0]


def window_weights(window_size, mode="constant", sigma_scale=0.125, device="cpu"):
    """The separable window weight: None for 'constant'; for 'gaussian' three float32 vectors (wz, wy, wx) with, per axis of
    length n, w[i] = max(exp(-0.5 * ((i - (n-1)/2) / (sigma_scale * n))**2), 1e-3), evaluated in float64.  The floor keeps the
    product of three above 1e-9, so the sum of weights never underflows whatever sigma_scale is."""
    if mode == "constant":
        return None
    if mode != "gaussian":
        raise ValueError(f"window_weight: 'constant' or 'gaussian', not {mode!r}")
    sigma_scale = float(sigma_scale)
    if not sigma_scale > 0:
        raise ValueError(f"window_sigma_scale must be positive, not {sigma_scale}")
    out = []
    for n in window_size:
        n = int(n)
        i = np.arange(n, dtype=np.float64)
        w = np.maximum(np.exp(-0.5 * ((i - (n - 1) / 2.0) / (sigma_scale * n)) ** 2), 1e-3)
        out.append(torch.from_numpy(w.astype(np.float32)).to(device))
    return tuple(out)


class _Tta:
    """The validated keys of one call; `on` is False when every key is at its default (the unchanged path)."""

    def __init__(self, args, window_size, device, weighted=True):
        self.codes = mirror_variants(getattr(args, "tta_mirror_axes", None) or ())
        mode = getattr(args, "window_weight", "constant")
        self.weights = window_weights(window_size, mode, getattr(args, "window_sigma_scale", 0.125), device)
        if not weighted:                      # whole image: one window, every weight cancels
            self.weights = None
        batch = getattr(args, "tta_batch", None)
        self.batch = len(self.codes) if batch is None else int(batch)
        if self.batch < 1:
            raise ValueError(f"tta_batch must be at least 1, not {batch}")
        self.batch = min(self.batch, len(self.codes))
        self.on = len(self.codes) > 1 or self.weights is not None


def _codes_arg(codes):
    return (C.c_int * len(codes))(*codes)


def _gather_mirror(img, codes, d0, h0, w0, window_size):
    """[V*B, C, wd, wh, ww]: the window of img at (d0, h0, w0), once per flip code (cbim_window_gather_mirror)."""
    _dev_ok(img)
    B, Cc, D, H, W = map(int, img.shape)
    wd, wh, ww = map(int, window_size)
    out = torch.empty((len(codes) * B, Cc, wd, wh, ww), dtype=torch.float32, device=img.device)
    _lib.check(_lib.lib().cbim_window_gather_mirror(_p(img), _p(out), _codes_arg(codes), len(codes), B, Cc, wd, wh, ww, D, H, W,
                                                    d0, h0, w0, _stream(img)), "window_gather_mirror")
    return out


def _accumulate_tta(logits, codes, weights, acc, wsum, d0, h0, w0):
    """acc[window] += w * sum over the variants of softmax(un-mirrored logits), wsum[window] += w * V
    (cbim_softmax_accumulate_tta); logits [V*B, K, wd, wh, ww], weights (wz, wy, wx) or None."""
    wz, wy, wx = weights if weights is not None else (None, None, None)
    _dev_ok(logits, acc, wsum, wz, wy, wx)
    VB, K, wd, wh, ww = map(int, logits.shape)
    B, _, D, H, W = map(int, acc.shape)
    if VB != len(codes) * B:
        raise ValueError(f"{VB} logit volumes for {len(codes)} variants of batch {B}")
    if wz is not None and (wz.numel(), wy.numel(), wx.numel()) != (wd, wh, ww):
        raise ValueError(f"weight vectors of {wz.numel()}, {wy.numel()}, {wx.numel()} for a {wd} x {wh} x {ww} window")
    _lib.check(_lib.lib().cbim_softmax_accumulate_tta(_p(logits), _codes_arg(codes), len(codes), _p(wz), _p(wy), _p(wx), _p(acc),
                                                      _p(wsum), B, K, wd, wh, ww, D, H, W, d0, h0, w0, _stream(logits)),
               "softmax_accumulate_tta")


def _window_tta(net, img, tta, acc, wsum, d0, h0, w0, window_size):
    """One window under mirror TTA / window weights: one gather, ceil(V / tta.batch) forwards, one accumulate per forward.
    acc / wsum None: allocated (zeros, the size of img) once the class count is known.  Returns (acc, wsum)."""
    B = int(img.shape[0])
    x = _gather_mirror(img, tta.codes, d0, h0, w0, window_size)
    for c0 in range(0, len(tta.codes), tta.batch):
        codes = tta.codes[c0:c0 + tta.batch]
        logits = _logits(net, x[c0 * B:(c0 + len(codes)) * B])
        if acc is None:
            acc = torch.zeros((B, int(logits.shape[1])) + tuple(img.shape[2:]), dtype=torch.float32, device=img.device)
            wsum = torch.zeros((B, 1) + tuple(img.shape[2:]), dtype=torch.float32, device=img.device)
        _accumulate_tta(logits, codes, tta.weights, acc, wsum, d0, h0, w0)
    return acc, wsum


def _finalize(acc, counter, want_labels=False):
    B, K = int(acc.shape[0]), int(acc.shape[1])
    S = acc.numel() // (B * K)
    labels = torch.empty((B,) + tuple(acc.shape[2:]), dtype=torch.int64, device=acc.device) if want_labels else None
    _lib.check(_lib.lib().cbim_prob_finalize(_p(acc), _p(counter), _p(labels), B, K, S, _stream(acc)), "prob_finalize")
    return labels


def _label_gate():
    """The validation entry points are the engine's per-epoch hook for the deferred label check (functional.check_labels): the
    fused loss counts out-of-range labels on the device — also inside a replayed hipGraph — and this is where the count is read
    (one synchronisation per validated volume) and raised as the reference's CrossEntropyLoss / scatter_ would have at the
    offending training step."""
    from .. import functional as Fn
    if Fn._CHECK_LABELS not in ("", "0"):
        Fn.check_labels()


def inference_whole_image(net, img, args=None):
    """softmax(net(img), 1) — inference3d.py:8-26.  With args.tta_mirror_axes the mean of that over the mirror variants (the
    window is the volume).  args.window_weight is ignored here: with one window every weight cancels."""
    _label_gate()
    net.eval()
    tta = _Tta(args, img.shape[2:], img.device, weighted=False) if args is not None else None
    with torch.no_grad():
        if tta is not None and tta.on:
            acc, wsum = _window_tta(net, img.contiguous().float(), tta, None, None, 0, 0, 0, img.shape[2:])
            _finalize(acc, wsum)                                      # wsum is the number of variants everywhere
            return acc
        logits = _logits(net, img)
        acc = torch.zeros_like(logits)
        _accumulate(logits, acc, None, 0, 0, 0)
    return acc


def _sliding_window_accumulate(net, img, args):
    """The window loop of inference_sliding_window up to, not including, the division by the window count: returns the summed
    window probabilities [B, classes, D, H, W], the count [B, 1, D, H, W] (both of the volume padded up to one window) and the
    unpadded size, or None when nothing was padded (inference3d.py:28-86).  Under args.tta_mirror_axes / args.window_weight
    the same window grid, the sum carries every variant weighted by the window weight and the count is the sum of weights."""
    net.eval()
    B, Cc, D, H, W = img.shape
    win_d, win_h, win_w = args.window_size
    hd, hh, hw = win_d // 2, win_h // 2, win_w // 2
    tta = _Tta(args, (2 * hd, 2 * hh, 2 * hw), img.device)       # the extent of a split_idx window; raises before any launch
    origin = None
    if D < win_d or H < win_h or W < win_w:
        origin = (D, H, W)
        img = F.pad(img, (0, max(0, win_w - W), 0, max(0, win_h - H), 0, max(0, win_d - D)))
        B, Cc, D, H, W = img.shape
    if tta.on:
        img = img.contiguous().float()
    acc = torch.zeros((B, args.classes, D, H, W), dtype=torch.float32, device=img.device)
    counter = torch.zeros((B, 1, D, H, W), dtype=torch.float32, device=img.device)
    with torch.no_grad():
        for i in range(D // hd):
            for j in range(H // hh):
                for k in range(W // hw):
                    d0, d1 = split_idx(hd, D, i)
                    h0, h1 = split_idx(hh, H, j)
                    w0, w1 = split_idx(hw, W, k)
                    if tta.on:
                        _window_tta(net, img, tta, acc, counter, d0, h0, w0, (d1 - d0, h1 - h0, w1 - w0))
                        continue
                    logits = _logits(net, img[:, :, d0:d1, h0:h1, w0:w1].contiguous())
                    _accumulate(logits, acc, counter, d0, h0, w0)
    return acc, counter, origin


def inference_sliding_window(net, img, args, return_labels=False):
    """Half-overlapping windows of args.window_size, probabilities averaged over the windows covering a voxel
    (inference3d.py:28-99).  With return_labels also the argmax map of validation.py:44 from the same pass.
    args.tta_mirror_axes, args.window_weight, args.window_sigma_scale, args.tta_batch: see the module docstring; the average
    is then over windows and mirror variants, weighted by the window weight."""
    _label_gate()
    acc, counter, origin = _sliding_window_accumulate(net, img, args)
    with torch.no_grad():
        labels = _finalize(acc, counter, return_labels)
    if origin is not None:
        acc = acc[:, :, :origin[0], :origin[1], :origin[2]]
        if labels is not None:
            labels = labels[:, :origin[0], :origin[1], :origin[2]]
    return (acc, labels) if return_labels else acc
