"""Writes tests/golden/jpeg_chunked.npz: five JPEG files of 120 x 160 written by the installed Pillow, long enough for
the chunked route of the device decoder to have many lanes per segment, and the RGB bytes the same Pillow decodes them
to (`Image.open(f).convert('RGB')`), never the model's or the kernel's.

    python -m tests.helpers.make_jpeg_chunked_golden

    names               the cases; per NAME s_NAME (the file, uint8) and y_NAME ([120][160][3] uint8, Pillow's)
    pil_version         the Pillow that wrote and judged
The file stays under 512 kB; tests/golden/jpeg_decode.npz is read as it is."""
from pathlib import Path

import numpy as np

from tests.helpers import jpeg_ref as ref

OUT = Path(__file__).resolve().parent.parent / "golden" / "jpeg_chunked.npz"

S444, S422, S420 = 0, 1, 2
H, W = 120, 160
# name: (content, Pillow's save arguments)
CASES = {
    "420_q75_smooth": ("smooth", dict(subsampling=S420, quality=75)),
    "444_q95_noise": ("noise", dict(subsampling=S444, quality=95)),          # a long scan with many stuffed FFs
    "422_opt": ("photo", dict(subsampling=S422, optimize=True)),             # custom tables
    "grey": ("photo", dict(mode="L")),
    "420_rst2rows": ("photo", dict(subsampling=S420, restart_marker_rows=2)),   # four long segments
}


def main():
    import PIL
    arrays = {"names": np.array(list(CASES)), "pil_version": np.array(PIL.__version__)}
    for k, (name, (kind, kw)) in enumerate(CASES.items()):
        data = ref.pil_encode(ref.make_image(500 + 11 * k, H, W, kind), **kw)
        arrays["s_" + name], arrays["y_" + name] = data, ref.pil_decode(data)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
