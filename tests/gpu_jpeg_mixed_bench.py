"""JPEG batches of mixed stored sizes: one mixed decode + resize call against the existing uniform calls (diagnostic,
not a pytest), with the files and the method of tests/gpu_jpeg_decode_bench.py: q75, 4:2:0, the benchmark's synthetic
content; HIP events over the whole call, warm, the median of 7 with the spread.  The files are stored at 480 x 640,
640 x 480, 960 x 1280 and 1280 x 960 in equal parts, shuffled (seeded), without restart markers and with one restart
per MCU row; batches of 32; the target is 480 x 640.  One step per process, so that each can run under a time limit of
its own; every step appends to the output file.
  calls     one `ops.decode_resize_jpeg` on the mixed batch against the sum of the existing uniform calls on the same
            files grouped by size (four `decode_jpeg` + `resize_u8` pairs), with the two stages of each timed alone and
            the bit check of both against each other;
  uniform   the mixed entry on a uniform batch of 32 files of 480 x 640 against the existing uniform calls;
  e2e       extract_features over a directory of 1024 such files with 8 loader workers, f16mx and bf16:
            `jpeg.collate_mixed` at batch 32, the Pillow uint8 loader with the host resize at batch 32, and the device
            path (`jpeg.collate`) at batch size 1; second pass of each; the descriptors compared.
    python tests/gpu_jpeg_mixed_bench.py STEP [output file]"""
import functools
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from openibl_amd import jpeg, ops  # noqa: E402
from gpu_jpeg_decode_bench import encode, events, spread  # noqa: E402

dev = torch.device("cuda", 0)
SIZES = ((480, 640), (640, 480), (960, 1280), (1280, 960))
TARGET = (480, 640)
BATCH, PER_SIZE = 32, 8
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def photos_at(n, h, w, seed):
    """The benchmark's synthetic images (openibl_amd.synth.images) at h x w, uint8 [n][h][w][3]."""
    from ibl.utils.data import MEAN, STD
    from openibl_amd import synth
    base = synth.images(n, h, w, seed=seed)
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    return ((base * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def mixed_files(**kw):
    """32 files, eight of every size, in a seeded shuffle -> (files, sizes)."""
    files, sizes = [], []
    for k, (h, w) in enumerate(SIZES):
        for img in photos_at(PER_SIZE, h, w, 900 + k):
            files.append(encode(img, **kw))
            sizes.append((h, w))
    order = np.random.RandomState(0).permutation(len(files))
    return [files[i] for i in order], [sizes[i] for i in order]


def med(fn):
    runs = events(fn)
    return statistics.median(runs), runs


def calls(label, files, sizes):
    mixed = jpeg.MixedJpegBatch.from_files(files, target=TARGET).to(dev)
    groups = {}
    for i, s in enumerate(sizes):
        groups.setdefault(s, []).append(i)
    uniform = {s: jpeg.JpegBatch.from_files([files[i] for i in idx]).to(dev) for s, idx in groups.items()}
    say(f"{label}: {len(files)} files, {len(groups)} sizes, {mixed.scan.numel() / 1e3:.0f} kB of scan, longest segment "
        f"{mixed.max_segment_bytes} bytes, packed pixels {mixed.totals[2] / 1e6:.1f} MB")

    def grouped():
        return {s: ops.resize_u8(ops.decode_jpeg(b, check=False)[0], TARGET) for s, b in uniform.items()}

    got, status = ops.decode_resize_jpeg(mixed, TARGET, check=False)
    assert int(status.abs().sum()) == 0
    route = ops.last_jpeg_route
    want = grouped()
    equal = all(torch.equal(got[idx], want[s]) for s, idx in groups.items())
    one, runs = med(lambda: ops.decode_resize_jpeg(mixed, TARGET, check=False))
    say(f"    one mixed decode_resize_jpeg call ({route}): {spread(runs, 'ms')}; {one / len(files):.4f} ms per image")
    four, runs = med(grouped)
    say(f"    four uniform decode_jpeg + resize_u8 pairs : {spread(runs, 'ms')}; {four / len(files):.4f} ms per image")
    say(f"    mixed / grouped = {one / four:.3f}; bit-equal: {equal}")
    # the stages alone
    dec, runs = med(lambda: ops._decode_jpeg_mixed_packed(mixed, "auto", None))
    say(f"    mixed, decode alone    : {spread(runs, 'ms')}")
    packed, _ = ops._decode_jpeg_mixed_packed(mixed, "auto", None)
    host_sizes = mixed.sizes.numpy()
    rs, runs = med(lambda: ops._resize_u8_mixed(packed, mixed.geom, host_sizes, *TARGET, "uint8", ops.REF_MEAN,
                                                ops.REF_STD, dev))
    say(f"    mixed, resize alone    : {spread(runs, 'ms')}")
    dec4, runs = med(lambda: [ops.decode_jpeg(b, check=False) for b in uniform.values()])
    say(f"    grouped, four decodes  : {spread(runs, 'ms')}")
    px = {s: ops.decode_jpeg(b, check=False)[0] for s, b in uniform.items()}
    rs4, runs = med(lambda: [ops.resize_u8(p, TARGET) for p in px.values()])
    say(f"    grouped, four resizes  : {spread(runs, 'ms')}")


def uniform_step(label, **kw):
    files = [encode(img, **kw) for img in photos_at(BATCH, 480, 640, 900)]
    mixed = jpeg.MixedJpegBatch.from_files(files).to(dev)
    plain = jpeg.JpegBatch.from_files(files).to(dev)
    got = ops.decode_resize_jpeg(mixed, TARGET)
    want = ops.resize_u8(ops.decode_jpeg(plain), TARGET)
    a, runs = med(lambda: ops.decode_resize_jpeg(mixed, TARGET, check=False))
    say(f"{label}: 32 files of 480 x 640, the mixed entry      : {spread(runs, 'ms')}")
    b, runs = med(lambda: ops.resize_u8(ops.decode_jpeg(plain, check=False)[0], TARGET))
    say(f"{label}: 32 files of 480 x 640, the uniform calls    : {spread(runs, 'ms')}")
    say(f"    mixed / uniform = {a / b:.3f}; bit-equal: {bool(torch.equal(got, want))}")


def e2e(label, **kw):
    import hubconf
    from ibl.evaluators import extract_features
    from ibl.utils.data import get_transformer_test
    from ibl.utils.data.preprocessor import Preprocessor
    from openibl_amd import synth
    n = 1024
    files, _ = mixed_files(**kw)
    with tempfile.TemporaryDirectory() as td:
        records = []
        for i in range(n):
            (Path(td) / f"{i:05d}.jpg").write_bytes(files[i % len(files)].tobytes())
            records.append((f"{i:05d}.jpg", i, 0.0, 0.0))
        common = dict(num_workers=8, shuffle=False, pin_memory=True, persistent_workers=True)
        raw = Preprocessor(records, root=td, raw=True)
        loaders = (
            ("collate_mixed, batch 32, decode + resize on the device",
             torch.utils.data.DataLoader(raw, batch_size=BATCH, collate_fn=functools.partial(
                 jpeg.collate_mixed, target=TARGET), **common), {"input_decode": True, "input_resize": TARGET}),
            ("Pillow uint8 loader with the host resize, batch 32",
             torch.utils.data.DataLoader(Preprocessor(records, root=td, transform=get_transformer_test(
                 *TARGET, as_uint8=True)), batch_size=BATCH, **common), {}),
            ("device path at batch size 1 (collate, decode_jpeg + resize_u8)",
             torch.utils.data.DataLoader(raw, batch_size=1, collate_fn=jpeg.collate, **common),
             {"input_decode": True, "input_resize": TARGET}))
        model = hubconf.vgg16_netvlad()
        model.load_state_dict(synth.embednetpca_state(0))
        model = model.to(dev).eval()
        for precision in ("f16mx", "bf16"):
            model.set_precision(precision)
            res = {}
            for name, loader, args in loaders:
                for rep in range(2):      # the second pass: graphs captured, workspaces sized
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    feats = extract_features(model, loader, records, gpu=dev.index, print_freq=10 ** 9, **args)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                res[name] = feats
                say(f"{label}, extract_features, {precision}, {n} files of 4 sizes, 8 workers, {name}: {dt:.3f} s = "
                    f"{n / dt:7.0f} images/s")
            first = next(iter(res.values()))
            for name, r in list(res.items())[1:]:
                say(f"    descriptors bit-equal, collate_mixed against {name}: "
                    f"{all(torch.equal(first[k], r[k]) for k in first)}")


if __name__ == "__main__":
    step = sys.argv[1] if len(sys.argv) > 1 else ""
    if step not in ("calls", "uniform", "e2e"):
        sys.exit(__doc__)
    torch.cuda.set_device(dev)
    import PIL
    say(f"---- {step}: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, Pillow {PIL.__version__}; "
        f"CHUNK_BYTES {jpeg.CHUNK_BYTES}, CHUNKED_MIN_BYTES {jpeg.CHUNKED_MIN_BYTES}")
    for label, kw in (("no restarts", {}), ("restart per MCU row", {"restart_marker_rows": 1})):
        if step == "calls":
            calls(label, *mixed_files(**kw))
        elif step == "uniform":
            uniform_step(label, **kw)
        else:
            e2e(label, **kw)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write("\n".join(LINES) + "\n")
