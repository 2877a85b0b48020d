"""Golden fixture for the fused probability resampling (cbim_resample_argmax).   python tests/golden/make_golden_prob_resample.py

numpy and scipy only.  Inputs are smooth softmax fields: random logits on a grid a third the size, zoomed cubically, times 4,
softmax over the classes; for two models the sum of two such fields.  The destination grid reaches 0.7 of a source voxel past
the source's edges on every resampled axis (the outside rule -0.5 <= c < n - 0.5 and the clamped half-voxel rim are both hit).
The expectation is scipy.ndimage.map_coordinates(order=1, mode='nearest') per class in float64, argmax (first maximum), 0
outside, stored with the float64 top-two margin.
  prob_resample.npz   per case: prob float32 [K, D, H, W], map float64 [3, 4], shape, label64 uint8, margin64 float32 (rounded
                      up, so a stored margin above the bar is a float64 margin above it), inside bool
"""
import os

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
OVERSHOOT = 0.7
# name -> (K, source shape, destination shape, models, seed)
CASES = {
    "a": (3, (5, 6, 7), (11, 13, 37), 1, 9101),         # K no multiple of anything
    "b": (16, (9, 14, 17), (20, 23, 31), 2, 9104),      # two models summed
    "c": (17, (6, 20, 20), (31, 20, 20), 1, 9103),      # one axis only, K one past 16
}


def softmax_field(rng, K, shape):
    small = tuple(max(2, -(-n // 3)) for n in shape)
    logits = rng.standard_normal((K,) + small)
    z = np.stack([ndimage.zoom(logits[k], [n / s for n, s in zip(shape, small)], order=3) for k in range(K)])
    assert z.shape == (K,) + tuple(shape), z.shape
    z = 4.0 * z
    e = np.exp(z - z.max(0))
    return e / e.sum(0)


def index_map(src, dst):
    """Destination index -> continuous source index: axes of equal length are left alone, the others run from -0.7 to
    n - 1 + 0.7."""
    m = np.zeros((3, 4), np.float64)
    for a in range(3):
        if src[a] == dst[a]:
            m[a, a] = 1.0
        else:
            m[a, a] = (src[a] - 1 + 2 * OVERSHOOT) / (dst[a] - 1)
            m[a, 3] = -OVERSHOOT
    return m


def coords(m, shape):
    k, j, i = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.stack([((m[a, 0] * k + m[a, 1] * j) + m[a, 2] * i) + m[a, 3] for a in range(3)])


def expectation(prob, co):
    src = prob.shape[1:]
    inside = np.ones(co.shape[1:], bool)
    for a in range(3):
        inside &= (co[a] >= -0.5) & (co[a] < src[a] - 0.5)
    vals = np.stack([ndimage.map_coordinates(prob[k].astype(np.float64), co, order=1, mode="nearest") for k in range(prob.shape[0])])
    vals = np.where(inside, vals, 0.0)
    top = np.sort(vals, axis=0)
    margin = top[-1] - top[-2]
    return np.where(inside, vals.argmax(0), 0).astype(np.uint8), margin, inside


def main():
    out = {}
    for name, (K, src, dst, models, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        prob = sum(softmax_field(rng, K, src) for _ in range(models)).astype(np.float32)
        m = index_map(src, dst)
        label, margin, inside = expectation(prob, coords(m, dst))
        low = int((inside & (margin <= 1e-5)).sum())
        assert (~inside).any() and low <= 1e-3 * inside.sum(), (name, low)
        margin32 = margin.astype(np.float32)
        margin32 = np.where(margin32 < margin, np.nextafter(margin32, np.float32(np.inf)), margin32)
        out[f"{name}_prob"], out[f"{name}_map"], out[f"{name}_shape"] = prob, m, np.asarray(dst, np.int64)
        out[f"{name}_label64"], out[f"{name}_margin64"], out[f"{name}_inside"] = label, margin32, inside
        print(f"  {name}: K {K} {src} -> {dst}: inside {int(inside.sum())} of {inside.size}, float64 margin <= 1e-5 on {low}, "
              f"classes present {len(np.unique(label[inside]))}")
    path = os.path.join(HERE, "prob_resample.npz")
    np.savez_compressed(path, **out)
    print(f"  prob_resample.npz {os.path.getsize(path) / 1024:.0f} KB")
    assert os.path.getsize(path) < 900 * 1024


if __name__ == "__main__":
    main()
