"""Writes tests/golden/train_input.npz: what the reference's training transform makes of the nine files of
tests/golden/jpeg_mixed.npz with one fixed jitter record each — computed by the installed Pillow alone, never by the
numpy models or the kernels:

    python -m tests.helpers.make_train_input_golden

    names               the files, in the batch order of jpeg_mixed.npz
    records             int32 [9][8], one record per file (tests/helpers/color_jitter_ref.py states the layout):
                        contrast at each of the four places, one record without contrast, one with every op skipped,
                        and three more (a skipped place in the middle, the two files of the host route among them)
    t_NAME              [32][48][3] uint8: `Image.open(f).convert('RGB')` -> the record's ops in the record's order
                        (`color_jitter_ref.pil_jitter`, as make_color_jitter_golden does it) ->
                        `.resize((48, 32), Image.BILINEAR)`
    u_NAME              [48][32][3] uint8: the same with `.resize((32, 48), Image.BILINEAR)`.  640x16_420 is 640 rows
                        high: a height of 32 is beyond the device resize's shrink limit of 16 per axis, a height of 48
                        is not, so this target is the one the device chain takes all nine files to
    pil_version         the Pillow that judged
The file stays under 100 kB."""
import io
from pathlib import Path

import numpy as np

from tests.helpers import color_jitter_ref as ref

GOLDEN = Path(__file__).resolve().parent.parent / "golden"
OUT = GOLDEN / "train_input.npz"
B, C, S, H, X = ref.BRIGHTNESS, ref.CONTRAST, ref.SATURATION, ref.HUE, ref.SKIP
ORDERS = ((C, B, S, H), (B, C, H, S), (H, S, C, B), (S, H, B, C),       # contrast at each of the four places
          (B, S, H, X),                                                  # no contrast: the first launch leaves at once
          (X, X, X, X),                                                  # nothing: the decoded bytes, resized
          (H, C, X, B), (S, X, C, X), (C, H, S, B))
TARGETS = {"t": (32, 48), "u": (48, 32)}     # (height, width)


def records():
    rng = np.random.default_rng(20240917)
    factors = rng.uniform(0.3, 1.7, (len(ORDERS), 3))
    hues = [ref.hue_byte(h) for h in rng.uniform(-0.5, 0.5, len(ORDERS))]
    return ref.pack_records(ORDERS, factors, hues)


def main():
    import PIL
    from PIL import Image
    src = dict(np.load(GOLDEN / "jpeg_mixed.npz", allow_pickle=False))
    names = [str(n) for n in src["names"]]
    rec = records()
    assert len(names) == len(ORDERS) == rec.shape[0]
    arrays = {"names": np.array(names), "records": rec, "pil_version": np.array(PIL.__version__)}
    for n, name in enumerate(names):
        rgb = np.asarray(Image.open(io.BytesIO(bytes(src["s_" + name]))).convert("RGB"))
        assert np.array_equal(rgb, src["y_" + name]), f"{name}: this Pillow decodes other bytes than the fixture's"
        jittered = Image.fromarray(ref.pil_jitter(rgb, *ref.unpack_record(rec[n])), mode="RGB")
        for key, (h2, w2) in TARGETS.items():
            arrays[f"{key}_{name}"] = np.asarray(jittered.resize((w2, h2), Image.BILINEAR))
            assert arrays[f"{key}_{name}"].shape == (h2, w2, 3)
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
