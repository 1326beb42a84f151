"""Writes tests/golden/color_jitter.npz: inputs, records and the expected uint8 images of the device colour jitter,
the expected images computed by PIL (tests/helpers/color_jitter_ref.py: pil_jitter), never by the model or the kernel.

    python -m tests.helpers.make_color_jitter_golden

Per case NAME the file holds x_NAME [N][H][W][3] uint8, rec_NAME [N][8] int32 and y_NAME [N][H][W][3] uint8; `names`
lists the cases.  Every case is small: the shapes are the smallest at which the kernel takes another path."""
import itertools
from pathlib import Path

import numpy as np

from tests.helpers import color_jitter_ref as ref

OUT = Path(__file__).resolve().parent.parent / "golden" / "color_jitter.npz"
B, C, S, H, X = ref.BRIGHTNESS, ref.CONTRAST, ref.SATURATION, ref.HUE, ref.SKIP


def _rand_image(rng, n, h, w):
    """Noise over a smooth ramp: every channel order of max / min occurs, and so do saturated and dark pixels."""
    base = rng.integers(0, 256, (n, 1, 1, 3))
    ramp = np.linspace(-90, 90, h * w).reshape(1, h, w, 1) * rng.choice([-1.0, 1.0], (n, 1, 1, 3))
    return np.clip(base + ramp + rng.normal(0, 40, (n, h, w, 3)), 0, 255).astype(np.uint8)


def _draw(rng, n):
    return rng.uniform(0.3, 1.7, (n, 3)), [ref.hue_byte(h) for h in rng.uniform(-0.5, 0.5, n)]


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    # one image per permutation of the four ops
    perms = list(itertools.permutations((B, C, S, H)))
    f, hb = _draw(rng, 24)
    out["perm24"] = (_rand_image(rng, 24, 16, 16), ref.pack_records(perms, f, hb))
    # 105 bytes per image: the second and third image start misaligned; skipped ops, all four skipped
    f, hb = _draw(rng, 3)
    out["odd5x7"] = (_rand_image(rng, 3, 5, 7), ref.pack_records([(S, C, H, B), (X, C, X, H), (X, X, X, X)], f, hb))
    # no multiple of a wave or a vector width
    f, hb = _draw(rng, 3)
    out["odd37x53"] = (_rand_image(rng, 3, 37, 53), ref.pack_records([(H, B, C, S), (C, X, S, X), (B, S, X, C)], f, hb))
    # several workgroups' partial sums behind the contrast mean, with a prefix in front of it
    f, hb = _draw(rng, 1)
    out["parts96x128"] = (_rand_image(rng, 1, 96, 128), ref.pack_records([(H, B, C, S)], f, hb))
    # the ends and the middle of the factor ranges
    x = _rand_image(rng, 3, 37, 53)
    out["exact"] = (x, ref.pack_records([(B, C, S, H)] * 3, [(0.3,) * 3, (1.0,) * 3, (1.7,) * 3],
                                        [ref.hue_byte(-0.5), ref.hue_byte(0.0), ref.hue_byte(0.5)]))
    # max == min, max == 0, all white
    x = np.stack([np.full((16, 16, 3), 77, np.uint8), np.zeros((16, 16, 3), np.uint8),
                  np.full((16, 16, 3), 255, np.uint8), np.tile(np.uint8([200, 30, 90]), (16, 16, 1))])
    f, hb = _draw(rng, 4)
    out["flat"] = (x, ref.pack_records([(H, C, S, B), (C, H, B, S), (S, B, H, C), (C, S, H, B)], f, hb))
    # the rounding of the contrast mean: mean L exactly 100.5 (-> 101), just below it (-> 100), and the same two
    # behind a brightness op that is the identity (the prefix must not disturb the sum)
    grey = np.full((4, 256), 100, np.uint8)
    grey[0, :128] = 101
    grey[1, :127] = 101
    grey[2, :128] = 101
    grey[3, :127] = 101
    x = np.repeat(grey.reshape(4, 16, 16, 1), 3, -1)
    out["mean_half"] = (x, ref.pack_records([(C, X, X, X), (C, X, X, X), (B, C, X, X), (B, C, X, X)],
                                            [(1.0, 1.7, 1.0), (1.0, 1.7, 1.0), (1.0, 0.3, 1.0), (1.0, 0.3, 1.0)],
                                            [0] * 4))
    # a colour sweep through all six hue sectors
    from PIL import Image
    hh, yy = np.meshgrid(np.arange(64) * 4, np.arange(64), indexing="xy")
    hsv = np.stack([hh, 255 - 2 * yy, 129 + 2 * yy], -1).astype(np.uint8)
    sweep = np.asarray(Image.fromarray(hsv, mode="HSV").convert("RGB"))
    f, hb = _draw(rng, 3)
    out["sweep64"] = (np.stack([sweep] * 3), ref.pack_records([(H, X, X, X), (X, X, H, X), (S, H, C, B)], f,
                                                              [0, 43, hb[2]]))
    return out


def main():
    arrays = {"names": np.array(sorted(cases()))}
    for name, (x, rec) in cases().items():
        arrays["x_" + name], arrays["rec_" + name] = x, rec
        arrays["y_" + name] = ref.pil_jitter_records(x, rec)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
