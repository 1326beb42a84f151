"""The chunked route of the device JPEG decoder against the serial one (diagnostic, not a pytest), with the files and
the method of tests/gpu_jpeg_decode_bench.py: 480 x 640, q75, 4:2:0, photo-like synthetic content, 32 distinct images
repeated; HIP events over the whole `ops.decode_jpeg(check=False)` call, warm, the median of 7 with the spread.  One
step per process, so that each can run under a time limit of its own; every step appends to the output file.
  routes   serial and chunked (the default chunk size) on 32, 256 and 1024 files without restart markers, the bit
           check of both against Pillow;
  chunks   chunk sizes 64, 128, 256 and 512 on 32 and on 1024 such files, with the settle rounds the kernel counted;
  sweep    the segment size at 32 files: one restart per MCU row, per 4 rows, per 10 rows, and the whole scan — the
           serial route against the chunked one at 64, 128 and 256 bytes (what CHUNKED_MIN_BYTES and CHUNK_BYTES of
           openibl_amd/jpeg.py are set from);
  pillow   Pillow on one host thread on the same files;
  e2e      extract_features over a directory of 1024 files without restart markers, 8 loader workers, batches of 32,
           f16mx and bf16: input_decode="serial", then "chunked", then the decoding uint8 loader; second pass of each.
    python tests/gpu_jpeg_chunked_bench.py STEP [output file]"""
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
from gpu_jpeg_decode_bench import DISTINCT, H, W, REPS, encode, events, photos, spread  # noqa: E402

dev = torch.device("cuda", 0)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def timed(batch, **kw):
    got, status = ops.decode_jpeg(batch, check=False, **kw)
    assert int(status.abs().sum()) == 0
    runs = events(lambda: ops.decode_jpeg(batch, check=False, **kw))
    rounds = ops.last_jpeg_rounds.cpu() if ops.last_jpeg_route == "chunked" else None
    return got, runs, rounds


def line(label, n, runs, rounds=None):
    med = statistics.median(runs)
    extra = "" if rounds is None else f"; settle rounds max {int(rounds.max())}, mean {float(rounds.float().mean()):.1f}"
    say(f"{label}: {spread(runs, 'ms')}; {1e3 * n / med:9.0f} images/s{extra}")
    return med


def batch_of(files, n):
    return jpeg.JpegBatch.from_files([files[i % DISTINCT] for i in range(n)])


def routes(plain):
    pil_rgb = torch.from_numpy(np.stack([jpeg.decode_on_host(f) for f in plain]))
    for n in (32, 256, 1024):
        host = batch_of(plain, n)
        batch = host.to(dev)
        say(f"no restarts, {n} files ({batch.scan.numel() / n / 1e3:.1f} kB of scan each, longest segment "
            f"{host.max_segment_bytes} bytes)")
        a, runs, _ = timed(batch, scan="serial")
        serial = line(f"    serial              ", n, runs)
        b, runs, rounds = timed(batch, scan="chunked")
        chunked = line(f"    chunked, {jpeg.CHUNK_BYTES:3d}-byte chunks", n, runs, rounds)
        say(f"    chunked / serial = {chunked / serial:.3f}; the two routes bit-equal: {bool(torch.equal(a, b))}"
            + (f"; bit-equal to Pillow on all {DISTINCT} distinct images: {bool(torch.equal(b.cpu(), pil_rgb))}"
               if n == 32 else ""))
        _, runs, _ = timed(batch, scan="auto")
        line(f"    auto ({ops.last_jpeg_route})", n, runs)


def chunks(plain):
    for n in (32, 1024):
        batch = batch_of(plain, n).to(dev)
        _, runs, _ = timed(batch, scan="serial")
        line(f"no restarts, {n:4d} files, serial             ", n, runs)
        for cb in (64, 128, 256, 512):
            _, runs, rounds = timed(batch, scan="chunked", chunk_bytes=cb)
            line(f"no restarts, {n:4d} files, chunked {cb:3d} bytes", n, runs, rounds)


def sweep(imgs, plain):
    for label, files in (("restart per MCU row", [encode(im, restart_marker_rows=1) for im in imgs]),
                         ("restart per 4 MCU rows", [encode(im, restart_marker_rows=4) for im in imgs]),
                         ("restart per 10 MCU rows", [encode(im, restart_marker_rows=10) for im in imgs]),
                         ("no restarts", plain)):
        host = batch_of(files, 32)
        batch = host.to(dev)
        seg = (host.segments[:, 1] - host.segments[:, 0]).float()
        say(f"{label}, 32 files: {host.segments.shape[0] // 32} segment(s) per image, mean {float(seg.mean()):.0f} "
            f"bytes, longest {host.max_segment_bytes}")
        a, runs, _ = timed(batch, scan="serial")
        serial = line("    serial           ", 32, runs)
        for cb in (64, 128, 256):
            b, runs, rounds = timed(batch, scan="chunked", chunk_bytes=cb)
            med = line(f"    chunked {cb:3d} bytes", 32, runs, rounds)
            say(f"        chunked / serial = {med / serial:.3f}; bit-equal: {bool(torch.equal(a, b))}")


def pillow(plain):
    runs = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for f in plain:
            jpeg.decode_on_host(f)
        runs.append((time.perf_counter() - t0) * 1e3 / len(plain))
    say(f"Pillow on one host thread, Image.open(...).convert('RGB'), per image: {spread(runs, 'ms')}; "
        f"{1e3 / statistics.median(runs):.0f} images/s per thread")


def e2e(plain):
    import hubconf
    from ibl.evaluators import extract_features
    from ibl.utils.data import get_transformer_test
    from ibl.utils.data.preprocessor import Preprocessor
    from openibl_amd import synth
    n = 1024
    with tempfile.TemporaryDirectory() as td:
        records = []
        for i in range(n):
            (Path(td) / f"{i:05d}.jpg").write_bytes(plain[i % DISTINCT].tobytes())
            records.append((f"{i:05d}.jpg", i, 0.0, 0.0))
        raw = torch.utils.data.DataLoader(Preprocessor(records, root=td, raw=True), batch_size=32, num_workers=8,
                                          shuffle=False, collate_fn=jpeg.collate, pin_memory=True,
                                          persistent_workers=True)
        host = torch.utils.data.DataLoader(
            Preprocessor(records, root=td, transform=get_transformer_test(H, W, as_uint8=True, resize=False)),
            batch_size=32, num_workers=8, shuffle=False, pin_memory=True, persistent_workers=True)
        model = hubconf.vgg16_netvlad()
        model.load_state_dict(synth.embednetpca_state(0))
        model = model.to(dev).eval()
        for precision in ("f16mx", "bf16"):
            model.set_precision(precision)
            res = {}
            for name, loader, kw in (("raw-bytes loader + input_decode='serial'", raw, {"input_decode": "serial"}),
                                     ("raw-bytes loader + input_decode='chunked'", raw, {"input_decode": "chunked"}),
                                     ("raw-bytes loader + input_decode=True", raw, {"input_decode": True}),
                                     ("host-decoding uint8 loader (Pillow)", host, {})):
                for rep in range(2):      # the second pass: graphs captured, workspaces sized
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    feats = extract_features(model, loader, records, gpu=dev.index, print_freq=10 ** 9, **kw)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                res[name] = feats
                say(f"no restarts, extract_features, {precision}, {n} files, 8 workers, {name}: {dt:.3f} s = "
                    f"{n / dt:7.0f} images/s")
            first = next(iter(res.values()))
            say(f"    descriptors bit-equal between all loaders: "
                f"{all(torch.equal(first[k], r[k]) for r in res.values() for k in first)}")


if __name__ == "__main__":
    step = sys.argv[1] if len(sys.argv) > 1 else ""
    if step not in ("routes", "chunks", "sweep", "pillow", "e2e"):
        sys.exit(__doc__)
    torch.cuda.set_device(dev)
    import PIL
    say(f"---- {step}: {torch.cuda.get_device_name(dev)}, torch {torch.__version__}, Pillow {PIL.__version__}; "
        f"CHUNK_BYTES {jpeg.CHUNK_BYTES}, CHUNKED_MIN_BYTES {jpeg.CHUNKED_MIN_BYTES}")
    imgs = photos(DISTINCT)
    plain = [encode(im) for im in imgs]
    {"routes": routes, "chunks": chunks, "pillow": pillow, "e2e": e2e}.get(step, lambda p: sweep(imgs, p))(plain)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "a") as f:
            f.write("\n".join(LINES) + "\n")
