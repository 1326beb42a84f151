"""Writes tests/golden/jpeg_decode.npz: JPEG streams written by the installed Pillow and the RGB bytes the same
Pillow decodes them to (`Image.open(f).convert('RGB')`), never the model's or the kernel's.

    python -m tests.helpers.make_jpeg_golden

    names               the single-image cases the device decodes; per NAME s_NAME (the file, uint8) and y_NAME
                        ([H][W][3] uint8, Pillow's)
    mixed4              four of those names, all 48 x 64, differing in sampling, quality, tables and restarts
    many_bytes / many_offsets / many_y      70 files of 16 x 16 back to back, file i = bytes[offsets[i]:offsets[i+1]]
    damaged             names of the damaged streams (s_NAME only): the 48 x 64 q75 4:2:0 file cut at half its scan,
                        and the same file with one scan byte XOR-ed (the first byte behind the middle of the scan
                        whose damage the numpy model notices; the model chooses the byte, it judges nothing)
    fallbacks           names of the files the host decodes; per NAME f_NAME and fy_NAME
    pil_version         the Pillow that wrote and judged
Sizes are height x width.  The file stays under 1 MB."""
import io
from pathlib import Path

import numpy as np

from tests.helpers import jpeg_ref as ref

OUT = Path(__file__).resolve().parent.parent / "golden" / "jpeg_decode.npz"

S444, S422, S420 = 0, 1, 2
# name: (height, width, content, Pillow's save arguments)
CASES = {
    "8x8_444": (8, 8, "smooth", dict(subsampling=S444)),
    "16x16_420": (16, 16, "smooth", dict(subsampling=S420)),                 # one MCU
    "9x17_422": (9, 17, "smooth", dict(subsampling=S422)),
    "17x31_420": (17, 31, "smooth", dict(subsampling=S420)),                 # partial MCUs on both axes
    "37x53_444": (37, 53, "smooth", dict(subsampling=S444)),
    "37x53_422": (37, 53, "smooth", dict(subsampling=S422)),
    "37x53_420": (37, 53, "smooth", dict(subsampling=S420)),
    "48x64_420_q30": (48, 64, "photo", dict(subsampling=S420, quality=30)),
    "48x64_420_q75": (48, 64, "photo", dict(subsampling=S420, quality=75)),
    "48x64_420_q95": (48, 64, "photo", dict(subsampling=S420, quality=95)),
    "48x64_420_rst1": (48, 64, "photo", dict(subsampling=S420, restart_marker_blocks=1)),   # 12 intervals: index wraps
    "48x64_420_rst3": (48, 64, "photo", dict(subsampling=S420, restart_marker_blocks=3)),   # not a divisor of the row
    "48x64_420_rstrow": (48, 64, "photo", dict(subsampling=S420, restart_marker_rows=1)),
    "48x64_422_opt": (48, 64, "photo", dict(subsampling=S422, optimize=True)),               # custom tables
    "37x53_grey": (37, 53, "smooth", dict(mode="L")),
    "48x64_444_flat": (48, 64, "flat", dict(subsampling=S444)),                              # EOB-only blocks
    "48x64_444_noise": (48, 64, "noise", dict(subsampling=S444, quality=95)),   # ZRL runs, long codes, stuffed FFs
    "40x104_444_rst65": (40, 104, "smooth", dict(subsampling=S444, restart_marker_blocks=1)),   # 65 segments
}
MIXED4 = ("48x64_420_q30", "48x64_422_opt", "48x64_420_rst3", "48x64_444_noise")
MANY = 70


def _scan_range(data):
    from openibl_amd import jpeg
    p = jpeg.parse(data)
    return p.scan_begin, p.scan_end


def main():
    import PIL
    from PIL import Image
    arrays = {"names": np.array(list(CASES)), "mixed4": np.array(MIXED4), "pil_version": np.array(PIL.__version__)}
    for k, (name, (h, w, kind, kw)) in enumerate(CASES.items()):
        data = ref.pil_encode(ref.make_image(7 * k + 1, h, w, kind), **kw)
        arrays["s_" + name], arrays["y_" + name] = data, ref.pil_decode(data)
    assert any(b"\xff\x00" in arrays["s_" + n].tobytes() for n in CASES)

    many = [ref.pil_encode(ref.make_image(200 + i, 16, 16, ("smooth", "noise", "photo")[i % 3]),
                           subsampling=i % 3, quality=(30, 75, 95, 60)[i % 4], optimize=bool(i % 5 == 0))
            for i in range(MANY)]
    arrays["many_bytes"] = np.concatenate(many)
    arrays["many_offsets"] = np.cumsum([0] + [m.size for m in many]).astype(np.int64)
    arrays["many_y"] = np.stack([ref.pil_decode(m) for m in many])

    base = arrays["s_48x64_420_q75"]
    b0, b1 = _scan_range(base)
    arrays["s_truncated"] = base[:b0 + (b1 - b0) // 2].copy()
    for at in range(b0 + (b1 - b0) // 2, b1):
        hurt = base.copy()
        hurt[at] ^= 0x55
        if hurt[at] not in (0x00, 0xFF) and hurt[at - 1] != 0xFF and ref.decode(hurt).status:
            arrays["s_xor"] = hurt
            break
    arrays["damaged"] = np.array(["truncated", "xor"])

    img = ref.make_image(5, 37, 53)
    files = {}
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", progressive=True)
    files["progressive"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    files["cmyk"] = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG")
    files["png"] = buf.getvalue()
    files["9x4_420"] = ref.pil_encode(ref.make_image(6, 9, 4), subsampling=S420).tobytes()   # 4 pixels wide
    arrays["fallbacks"] = np.array(list(files))
    for name, data in files.items():
        arrays["f_" + name] = np.frombuffer(data, np.uint8)
        arrays["fy_" + name] = ref.pil_decode(data)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
