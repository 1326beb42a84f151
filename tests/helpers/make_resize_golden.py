"""Writes tests/golden/resize_u8.npz: inputs and the expected uint8 images of the device resize, the expected images
computed by PIL itself (`Image.resize((nw, nh), Image.BILINEAR)`), never by the model or the kernel.

    python -m tests.helpers.make_resize_golden

Per case NAME the file holds x_NAME [N][H][W][3] uint8 and y_NAME [N][nh][nw][3] uint8; `names` lists the cases and
`pil_version` the PIL that judged.  jr_NAME [N][nh][nw][3] is PIL's resize of the JITTERED bytes y_NAME of
tests/golden/color_jitter.npz — the reference's order, ColorJitter before Resize — for the cases in JITTERED.
Every case is small: the largest image is 97 x 131."""
from pathlib import Path

import numpy as np

from tests.helpers import resize_u8_ref as ref

GOLDEN = Path(__file__).resolve().parent.parent / "golden"
OUT = GOLDEN / "resize_u8.npz"

# name: (images, source height x width, target height x width)
CASES = {
    "half": (1, (96, 128), (48, 64)),        # exact 2x
    "down": (3, (61, 83), (48, 64)),         # three distinct images: the batch tests use them
    "up": (1, (30, 40), (48, 64)),
    "one_axis": (1, (48, 83), (48, 64)),
    "same": (2, (48, 64), (48, 64)),         # must equal the input
    "far": (1, (97, 131), (16, 16)),         # 6.1x and 8.2x: rows of 15 and 19 coefficients, one tile
    "to_one": (2, (7, 5), (1, 1)),
    "from_one": (2, (1, 1), (5, 7)),
}
# colour-jitter case: target size of the resize behind it
JITTERED = {"odd37x53": (24, 32), "parts96x128": (48, 64), "perm24": (12, 20)}


def cases():
    out = {}
    for k, (name, (n, (h, w), size)) in enumerate(sorted(CASES.items())):
        out[name] = (np.stack([ref.make_image(100 * k + i, h, w) for i in range(n)]), size)
    return out


def main():
    import PIL
    arrays = {"names": np.array(sorted(CASES)), "pil_version": np.array(PIL.__version__)}
    for name, (x, (nh, nw)) in cases().items():
        arrays["x_" + name] = x
        arrays["y_" + name] = np.stack([ref.pil_resize(img, nh, nw) for img in x])
    jitter = np.load(GOLDEN / "color_jitter.npz", allow_pickle=False)
    for name, (nh, nw) in JITTERED.items():
        arrays["jr_" + name] = np.stack([ref.pil_resize(img, nh, nw) for img in jitter["y_" + name]])
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
