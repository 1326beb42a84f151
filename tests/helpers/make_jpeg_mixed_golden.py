"""Writes tests/golden/jpeg_mixed.npz: nine image files of nine stored sizes written by the installed Pillow — the
batch of mixed sizes the tests of the mixed device decoder and resize use — with what the same Pillow makes of them,
never the model's or the kernel's:

    python -m tests.helpers.make_jpeg_mixed_golden

    names               the cases, in batch order; per NAME
        s_NAME          the file (uint8)
        y_NAME          `Image.open(f).convert('RGB')`, [H][W][3] uint8
        rK_NAME         `.resize((W2, H2), Image.BILINEAR)` of that for target K of `targets`, [H2][W2][3] uint8 (absent
                        where the stored size is more than 16 times the target on an axis: the resize's limit)
    targets             int [3][2] = (H2, W2)
    pil_version         the Pillow that wrote and judged
The file stays under 512 kB."""
import io
from pathlib import Path

import numpy as np

from tests.helpers import jpeg_ref as ref

OUT = Path(__file__).resolve().parent.parent / "golden" / "jpeg_mixed.npz"

S444, S422, S420 = 0, 1, 2
TARGETS = ((40, 72), (48, 64), (16, 16))    # partial tiles on both axes; the identity for 48x64_grey; a small one
MAX_SHRINK = 16
# name: (H, W, content, how it is written)
CASES = {
    "37x53_420": (37, 53, "photo", dict(subsampling=S420)),                  # nothing a multiple of 16
    "48x64_grey": (48, 64, "photo", dict(mode="L")),
    "64x48_422": (64, 48, "smooth", dict(subsampling=S422)),                 # portrait next to landscape
    "9x8_444": (9, 8, "smooth", dict(subsampling=S444)),                     # the minimum width
    "120x160_420": (120, 160, "photo", dict(subsampling=S420, quality=90)),  # several kB of scan: many chunks
    "120x160_420_rstrow": (120, 160, "photo", dict(subsampling=S420, quality=90, restart_marker_rows=1)),
    "640x16_420": (640, 16, "photo", dict(subsampling=S420)),                # a factor of exactly 16 to a height of 40
    "40x56_progressive": (40, 56, "photo", dict(subsampling=S420, progressive=True)),   # the host route
    "24x30_png": (24, 30, "smooth", "PNG"),                                              # the host route
}


def encode(img, how):
    if how == "PNG":
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(img, "RGB").save(buf, "PNG")
        return np.frombuffer(buf.getvalue(), np.uint8).copy()
    return ref.pil_encode(img, **how)


def pil_rgb(data):
    from PIL import Image
    return Image.open(io.BytesIO(bytes(data))).convert("RGB")


def main():
    import PIL
    from PIL import Image
    arrays = {"names": np.array(list(CASES)), "pil_version": np.array(PIL.__version__),
              "targets": np.array(TARGETS, np.int32)}
    for k, (name, (h, w, kind, how)) in enumerate(CASES.items()):
        data = encode(ref.make_image(900 + 7 * k, h, w, kind), how)
        rgb = pil_rgb(data)
        arrays["s_" + name], arrays["y_" + name] = data, np.asarray(rgb)
        assert arrays["y_" + name].shape == (h, w, 3)
        for t, (h2, w2) in enumerate(TARGETS):
            if h <= MAX_SHRINK * h2 and w <= MAX_SHRINK * w2:
                arrays[f"r{t}_{name}"] = np.asarray(rgb.resize((w2, h2), Image.BILINEAR))
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
