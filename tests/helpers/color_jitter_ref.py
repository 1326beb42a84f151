"""Reference for the device colour jitter (openibl_amd/csrc/augment.hip), two independent ways:

  * `model_jitter`: a numpy model of the arithmetic the kernel implements, rounding by rounding (fp32 where PIL's C code
    computes in `float`, double where it promotes), and
  * `pil_jitter`: the oracle — what torchvision's ColorJitter does to a PIL image, rebuilt from the PIL calls torchvision
    delegates to (ImageEnhance.Brightness / Contrast / Color, and the hue shift through PIL's HSV mode).

tests/test_color_jitter_cpu.py holds the model to PIL (all 2^24 colours through both HSV directions, random images
through the blends); the fixture tests/golden/color_jitter.npz stores PIL's outputs, and the GPU tests hold the kernel
to the fixture bit for bit.

A record (one per image, 32 bytes, eight int32 words): words 0..3 the op codes in application order (0 brightness,
1 contrast, 2 saturation, 3 hue, -1 skip), words 4..6 the bits of the fp32 brightness / contrast / saturation factors,
word 7 the hue shift byte 0..255."""
import numpy as np

f32, f64 = np.float32, np.float64
BRIGHTNESS, CONTRAST, SATURATION, HUE, SKIP = 0, 1, 2, 3, -1


def hue_byte(hue):
    """torchvision adds uint8(hue * 255) to the H plane with wrap-around: truncation toward zero, mod 256."""
    return int(hue * 255) % 256


def pack_records(orders, factors, hue_bytes):
    """orders [N][4] op codes, factors [N][3] (brightness, contrast, saturation), hue_bytes [N] -> int32 [N][8]."""
    orders = np.asarray(orders, dtype=np.int32).reshape(-1, 4)
    n = orders.shape[0]
    rec = np.zeros((n, 8), dtype=np.int32)
    rec[:, :4] = orders
    rec[:, 4:7] = np.asarray(factors, dtype=f32).reshape(n, 3).view(np.int32)
    rec[:, 7] = np.asarray(hue_bytes, dtype=np.int64).reshape(n) & 255
    return rec


def unpack_record(rec):
    rec = np.asarray(rec, dtype=np.int32).reshape(8)
    return [int(c) for c in rec[:4]], [float(v) for v in rec[4:7].view(f32)], int(rec[7])


# ---- the numpy model ---------------------------------------------------------------------------------------------
def luma(img):
    """PIL's RGB -> L: (19595 R + 38470 G + 7471 B + 32768) >> 16."""
    x = img.astype(np.int64)
    return ((19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 32768) >> 16).astype(np.int32)


def blend(d, x, factor):
    """Image.blend(degenerate, image, factor) per byte: fp32, each operation rounded on its own; the result is
    truncated, and clipped only when the factor is outside [0, 1] (inside, PIL does not clip: it cannot overflow)."""
    a = f32(factor)
    df, xf = d.astype(f32), x.astype(f32)
    t = (df + (a * (xf - df)).astype(f32)).astype(f32)
    out = np.trunc(t).astype(np.int32)
    if not (f32(0) <= a <= f32(1)):
        out = np.where(t <= 0, 0, np.where(t >= 255, 255, out))
    return out.astype(np.uint8)


def contrast_mean(img):
    """int(mean(L) + 0.5) with the sum exact and the division in double (ImageStat + ImageEnhance.Contrast)."""
    L = luma(img)
    return int(float(int(L.sum())) / float(L.size) + 0.5)


def rgb_to_hsv(x):
    r, g, b = (x[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    cr = (maxc - minc).astype(f32)
    crs = np.where(cr == 0, f32(1), cr)
    s = cr / np.where(maxc == 0, 1, maxc).astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / crs for c in (r, g, b))
    rc64, gc64, bc64 = rc.astype(f64), gc.astype(f64), bc.astype(f64)
    h0 = np.where(r == maxc, (bc - gc).astype(f64),
                  np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(f32)
    h1 = np.fmod(h0.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h1.astype(f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    grey = maxc == minc
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def hsv_to_rgb(x):
    h, s, v = (x[..., c].astype(np.int32) for c in range(3))
    fh = (h.astype(f64) * 6.0 / 255.0).astype(f32)
    i = np.floor(fh).astype(np.int32)
    f = (fh - i.astype(f32)).astype(f32)
    fs = (s.astype(f64) / 255.0).astype(f32)
    vf, F, S = v.astype(f64), f.astype(f64), fs.astype(f64)

    def rnd(t):
        return np.clip(np.floor(t.astype(f32) + f32(0.5)).astype(np.int32), 0, 255)

    p, q, t = rnd(vf * (1.0 - S)), rnd(vf * (1.0 - S * F)), rnd(vf * (1.0 - S * (1.0 - F)))
    i = i % 6
    R = np.choose(i, [v, q, p, p, t, v])
    G = np.choose(i, [t, v, v, q, p, p])
    B = np.choose(i, [p, p, t, v, v, q])
    out = np.stack([R, G, B], -1)
    return np.where((s == 0)[..., None], np.stack([v, v, v], -1), out).astype(np.uint8)


def model_jitter(img, order, factors, hue_shift):
    """img [H][W][3] uint8; order: four op codes; factors (brightness, contrast, saturation); hue_shift: the byte."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    for op in order:
        if op == BRIGHTNESS:
            img = blend(np.zeros_like(img), img, factors[0])
        elif op == CONTRAST:
            img = blend(np.full_like(img, contrast_mean(img)), img, factors[1])
        elif op == SATURATION:
            L = luma(img).astype(np.uint8)
            img = blend(np.repeat(L[..., None], 3, -1), img, factors[2])
        elif op == HUE:
            hsv = rgb_to_hsv(img)
            hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(hue_shift)) % 256
            img = hsv_to_rgb(hsv)
        elif op != SKIP:
            raise ValueError(f"unknown op code {op}")
    return img


def model_jitter_records(x, records):
    """x [N][H][W][3] uint8, records int32 [N][8] -> [N][H][W][3] uint8."""
    return np.stack([model_jitter(x[n], *unpack_record(records[n])) for n in range(x.shape[0])])


# ---- the oracle: PIL ----------------------------------------------------------------------------------------------
def pil_jitter(img, order, factors, hue):
    """The same chain through PIL, as torchvision's functional_pil applies it.  `hue` is the hue FACTOR in
    [-0.5, 0.5] (torchvision's argument), or an int: the shift byte itself."""
    from PIL import Image, ImageEnhance
    shift = hue if isinstance(hue, (int, np.integer)) else hue_byte(hue)
    im = Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8), mode="RGB")
    for op in order:
        if op == BRIGHTNESS:
            im = ImageEnhance.Brightness(im).enhance(float(f32(factors[0])))
        elif op == CONTRAST:
            im = ImageEnhance.Contrast(im).enhance(float(f32(factors[1])))
        elif op == SATURATION:
            im = ImageEnhance.Color(im).enhance(float(f32(factors[2])))
        elif op == HUE:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.uint8(shift & 255)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
        elif op != SKIP:
            raise ValueError(f"unknown op code {op}")
    return np.asarray(im, dtype=np.uint8).copy()


def pil_jitter_records(x, records):
    return np.stack([pil_jitter(x[n], *unpack_record(records[n])) for n in range(x.shape[0])])


def host_normalize(u8):
    """ToTensor + Normalize as the loader's transform computes them on the host (ibl/utils/data/__init__.py):
    u8 [N][H][W][3] uint8 (numpy or torch) -> torch float32 [N][3][H][W]."""
    import torch
    from ibl.utils.data import MEAN, STD
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    x = torch.as_tensor(u8).permute(0, 3, 1, 2).float() / 255.0
    return ((x - mean) / std).contiguous()
