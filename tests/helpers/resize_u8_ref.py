"""A numpy model of PIL's 8-bit bilinear resampling, `Image.resize((nw, nh), Image.BILINEAR)` on an RGB image: the
arithmetic csrc/resize_tables.h and csrc/resize.hip repeat.

Per axis a table: for every output sample a window [xmin, xmin + n) of source samples and n triangle weights in IEEE
double, normalised by their sum and rounded to 22-bit fixed point.  Then two integer passes, horizontal first, with a
uint8 intermediate: byte = clip(((1 << 21) + sum of coeff * source byte) >> 22, 0, 255).  Python floats are IEEE
doubles and every operation below is rounded on its own, as in PIL's C."""
import math

import numpy as np

PRECISION_BITS = 22


def ksize_of(in_size, out_size):
    scale = in_size / out_size
    fs = max(scale, 1.0)
    return int(math.ceil(1.0 * fs)) * 2 + 1


def tables(in_size, out_size):
    """(bounds int32 [out][2] = {xmin, n}, coeff int32 [out][ksize]) of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coeff = np.zeros((out_size, ksize), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)      # int() truncates toward zero, as C's (int)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = []
        ww = 0.0
        for x in range(n):
            v = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - v if v < 1.0 else 0.0)
            ww += w[-1]
        for x in range(n):
            k = w[x] / ww if ww != 0.0 else w[x]
            coeff[xx, x] = int(-0.5 + k * 4194304.0) if k < 0 else int(0.5 + k * 4194304.0)
        bounds[xx] = (xmin, n)
    return bounds, coeff


def resample_axis(img, axis, bounds, coeff):
    """One pass along `axis` of a uint8 array: the integer sums, rounded and clipped."""
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for xx in range(bounds.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = coeff[xx, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (1 << (PRECISION_BITS - 1)) + (k * src[xmin:xmin + n]).sum(axis=0)
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, nh, nw):
    """img [H][W][3] (or [N][H][W][3]) uint8 -> [nh][nw][3]: horizontal pass, uint8 intermediate, vertical pass."""
    img = np.asarray(img, dtype=np.uint8)
    ax_h, ax_w = img.ndim - 3, img.ndim - 2
    mid = resample_axis(img, ax_w, *tables(img.shape[ax_w], nw))
    return resample_axis(mid, ax_h, *tables(img.shape[ax_h], nh))


def pil_resize(img, nh, nw):
    """The judge: PIL itself."""
    from PIL import Image
    return np.asarray(Image.fromarray(np.asarray(img, dtype=np.uint8), "RGB").resize((nw, nh), Image.BILINEAR),
                      dtype=np.uint8).copy()


def make_image(seed, h, w):
    """Random bytes with blocks of pure 0 and 255 (the rounded coefficients can sum above 2^22: the clip is
    reached on saturated areas)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if h >= 4 and w >= 4:
        img[: h // 3, : w // 2] = 255
        img[h - h // 3:, w // 2:] = 0
        img[h // 3: h // 2, : w // 4, 1] = 255
    elif seed % 2:
        img[...] = 255
    return img
