"""Training tuples from the files' bytes: the colour jitter on the packed buffer, the whole input chain and a Trainer
step under three inputs (diagnostic, not a pytest), with the files and the method of tests/gpu_jpeg_mixed_bench.py:
q75, 4:2:0, the benchmark's synthetic content; HIP events over the whole call (wall clock with the device drained for
the trainer), warm, the median of 7 with the spread.  One step per process, so that each can run under a time limit
of its own; every step appends to the output file.
  jitter    `ops.color_jitter_mixed` in place on 12 and 48 images of 480 x 640 against `ops.color_jitter(out='uint8')`
            on the same images with the same records (the cost of the table indirection), the bit check of one
            against the other, and a batch of four sizes (480 x 640 .. 1280 x 960);
  chain     `ops.decode_jitter_resize_jpeg` to 480 x 640 float for one tuple of 12 files and for 4 tuples, without
            restart markers and with one restart per MCU row, with its three stages timed alone;
  trainer   `Trainer.train` (one tuple of 12 images per step, train_layers='conv5', the model's default precision),
            per step over 20 iterations from batches held in memory: uint8 tuples + `augment` (the flow before this
            one), the files' bytes with prefetch=False, and with prefetch=True.
    python tests/gpu_train_input_bench.py STEP [output file]"""
import contextlib
import io
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from openibl_amd import jpeg, ops  # noqa: E402
from openibl_amd.augment import ColorJitter, Compose, DecodeJpeg, Resize  # noqa: E402
from gpu_jpeg_decode_bench import encode, events, spread  # noqa: E402
from gpu_jpeg_mixed_bench import SIZES, photos_at  # noqa: E402

dev = torch.device("cuda", 0)
TARGET = (480, 640)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def med(fn):
    runs = events(fn)
    return statistics.median(runs), runs


def draw(n, seed=5):
    return ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(seed)).draw(n)


def pack(images):
    """uint8 images [H_i][W_i][3] -> (packed buffer on the device, sizes)."""
    sizes = np.asarray([im.shape[:2] for im in images], np.int32)
    geom, totals = jpeg.mixed_layout(sizes)
    packed = torch.zeros(totals[2], dtype=torch.uint8)
    for im, o in zip(images, jpeg.geom_pixel_offsets(geom).tolist()):
        packed[o:o + im.size] = torch.from_numpy(im.reshape(-1))
    return packed.to(dev), sizes


def jitter_step():
    for n in (12, 48):
        imgs = photos_at(n, 480, 640, 900)
        rec = draw(n).to(dev)
        dense = torch.from_numpy(imgs).to(dev)
        packed, sizes = pack(list(imgs))
        geom = torch.from_numpy(jpeg.mixed_layout(sizes)[0]).to(dev)
        want = ops.color_jitter(dense, rec, out="uint8")
        got = ops.color_jitter_mixed(packed, sizes, rec)
        equal = torch.equal(got.view(n, 480, 640, 3), want)         # 480 x 640 x 3 is a multiple of 64: no padding
        a, runs = med(lambda: ops._color_jitter_mixed(packed, geom, sizes, rec, packed, dev))
        say(f"{n} images of 480 x 640, color_jitter_mixed in place : {spread(runs, 'ms')}")
        b, runs = med(lambda: ops.color_jitter(dense, rec, out="uint8"))
        say(f"{n} images of 480 x 640, color_jitter(out='uint8')   : {spread(runs, 'ms')}")
        say(f"    mixed / uniform = {a / b:.3f}; bit-equal: {bool(equal)}")
    imgs = [photos_at(1, h, w, 910 + k)[0] for k, (h, w) in enumerate(SIZES) for _ in range(3)]
    rec = draw(len(imgs)).to(dev)
    packed, sizes = pack(imgs)
    geom = torch.from_numpy(jpeg.mixed_layout(sizes)[0]).to(dev)
    a, runs = med(lambda: ops._color_jitter_mixed(packed, geom, sizes, rec, packed, dev))
    mpx = sum(im.shape[0] * im.shape[1] for im in imgs) / 1e6
    say(f"12 images of four sizes (480 x 640 .. 1280 x 960, {mpx:.1f} Mpixel), color_jitter_mixed in place: "
        f"{spread(runs, 'ms')}; {a / mpx:.4f} ms per Mpixel")


def tuple_files(n, **kw):
    """n files cycling through the four sizes."""
    return [encode(photos_at(1, *SIZES[k % 4], 920 + k)[0], **kw) for k in range(n)]


def chain_step():
    for label, kw in (("no restarts", {}), ("restart per MCU row", {"restart_marker_rows": 1})):
        for n in (12, 48):
            batch = jpeg.MixedJpegBatch.from_files(tuple_files(n, **kw), target=TARGET).to(dev)
            rec = draw(n).to(dev)
            sizes = batch.sizes.numpy()
            out, status = ops.decode_jitter_resize_jpeg(batch, rec, TARGET, check=False)
            assert int(status.abs().sum()) == 0
            a, runs = med(lambda: ops.decode_jitter_resize_jpeg(batch, rec, TARGET, check=False))
            say(f"{label}, {n} files of four sizes -> 480 x 640 float, decode_jitter_resize_jpeg "
                f"({ops.last_jpeg_route}): {spread(runs, 'ms')}; {a / n:.4f} ms per image")
            _, runs = med(lambda: ops._decode_jpeg_mixed_packed(batch, "auto", None))
            say(f"    decode alone : {spread(runs, 'ms')}")
            packed, _ = ops._decode_jpeg_mixed_packed(batch, "auto", None)
            _, runs = med(lambda: ops._color_jitter_mixed(packed, batch.geom, sizes, rec, packed, dev))
            say(f"    jitter alone : {spread(runs, 'ms')}")
            _, runs = med(lambda: ops._resize_u8_mixed(packed, batch.geom, sizes, *TARGET, "float", ops.REF_MEAN,
                                                       ops.REF_STD, dev))
            say(f"    resize alone : {spread(runs, 'ms')}")


def trainer_step(iters=20, reps=7):
    from ibl import models
    from ibl.trainers import Trainer
    from ibl.utils.data import IterLoader
    from openibl_amd import synth
    B, N = 1, 12
    base = models.create("vgg16", pretrained=False, train_layers="conv5")
    model = models.create("embednet", base, models.create("netvlad", dim=base.feature_dim))
    model.load_state_dict({k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")})
    for layer in list(base.base.children())[:type(base)._fix_layers["conv5"]]:
        for p in layer.parameters():
            p.requires_grad_(False)
    model = model.to(dev).train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-6, momentum=0.9)
    say(f"Trainer.train, {B} tuple of {N} images per step, target 480 x 640, precision "
        f"{getattr(model.base_model, 'precision', '?')}, {iters} iterations per run, ms per step")
    # the flow before this one: uint8 tuples of one size (the workers decoded and resized), jitter on the device
    raw = torch.from_numpy(photos_at(B * N, 480, 640, 99)).view(B, N, 480, 640, 3)
    u8_batches = [[(raw[:, j].contiguous().pin_memory(), ["name"] * B) for j in range(N)]] * iters
    # the files' bytes: 480 x 640 files (what the row above decodes in its workers), and files of four sizes
    same = [[(torch.from_numpy(encode(im)), f"f{k}", k, 0.0, 0.0) for k, im in enumerate(photos_at(N, 480, 640, 99))]]
    four = [[(torch.from_numpy(f), f"f{k}", k, 0.0, 0.0) for k, f in enumerate(tuple_files(N))]]

    def pinned(items):
        b = jpeg.collate_tuples(items, target=TARGET)
        return [[b[0].pin_memory()] + b[1:]] * iters

    def jit(**kw):
        return ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(5), **kw)

    def chain():
        return Compose(DecodeJpeg(), jit(out="uint8"), Resize(*TARGET))
    rows = (("uint8 tuples of 480 x 640 + augment (decode and resize in the workers)", jit(), False, u8_batches),
            ("the files' bytes, 480 x 640 files, prefetch=False", chain(), False, pinned(same)),
            ("the files' bytes, 480 x 640 files, prefetch=True", chain(), True, pinned(same)),
            ("the files' bytes, files of four sizes, prefetch=False", chain(), False, pinned(four)),
            ("the files' bytes, files of four sizes, prefetch=True", chain(), True, pinned(four)))
    results = {label: [] for label, *_ in rows}
    for rep in range(reps + 1):                     # the first round warms every flow; the flows alternate
        for label, augment, prefetch, batches in rows:
            trainer = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index, augment=augment, prefetch=prefetch)
            loader = IterLoader(batches, length=iters)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                trainer.train(0, 0, loader, opt, iters, print_freq=10 ** 9)
            torch.cuda.synchronize()
            if rep:
                results[label].append((time.perf_counter() - t0) * 1e3 / iters)
    base_ms = statistics.median(results[rows[0][0]])
    for label, runs in results.items():
        say(f"    {label:72s}: {spread(runs, 'ms')}; {statistics.median(runs) / base_ms:.3f} of the first row")


if __name__ == "__main__":
    step = sys.argv[1] if len(sys.argv) > 1 else ""
    if step not in ("jitter", "chain", "trainer"):
        sys.exit(__doc__)
    torch.cuda.set_device(dev)
    import PIL
    say(f"---- {step}: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, Pillow {PIL.__version__}")
    {"jitter": jitter_step, "chain": chain_step, "trainer": trainer_step}[step]()
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write("\n".join(LINES) + "\n")
