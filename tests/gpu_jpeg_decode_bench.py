"""The device JPEG decoder at the extraction shape (diagnostic, not a pytest).  In one process, warm, the median of 7
with the spread, by HIP events:
  (a) ops.decode_jpeg(check=False) on 32, 256 and 1024 files of 480 x 640 (q75, 4:2:0, photo-like synthetic content,
      32 distinct images repeated), written without restart markers and with one restart per MCU row; the time of the
      memset and of each of the three kernels from the profiler's kernel records of one call, when they are available;
  (b) the host side per image: jpeg.parse + packing (JpegBatch.from_files) on one thread;
  (c) Pillow on one host thread on the same files, Image.open(...).convert('RGB') (if Pillow can be imported), and the
      bit check of the first batch against it;
  (d) end to end: extract_features over a directory of 1024 such files, 8 loader workers, batches of 32, f16mx and
      bf16 — the raw-bytes loader with input_decode=True against the decoding uint8 loader, second pass of each
      (persistent workers: the second pass does not pay their start).
    python tests/gpu_jpeg_decode_bench.py [output file]"""
import io
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from openibl_amd import jpeg, ops  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W, REPS, DISTINCT = 480, 640, 7, 32
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def spread(runs, unit):
    return f"median {statistics.median(runs):9.4f} {unit} (min {min(runs):.4f}, max {max(runs):.4f})"


def events(fn, reps=REPS):
    fn()
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        runs.append(s.elapsed_time(e))
    return runs


def photos(n):
    """The benchmark's own synthetic images (openibl_amd.synth.images: low-frequency sinusoids, soft blobs and noise, as
    bench.py feeds the model) as uint8 [n][H][W][3]."""
    from ibl.utils.data import MEAN, STD
    from openibl_amd import synth
    base = synth.images(n, H, W, seed=900)
    mean, std = torch.tensor(MEAN).view(1, 3, 1, 1), torch.tensor(STD).view(1, 3, 1, 1)
    return ((base * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()


def encode(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=75, subsampling=2, **kw)
    return np.frombuffer(buf.getvalue(), np.uint8).copy()


def stage_times(batch):
    """{kernel or memset: microseconds} of one call, from the profiler's device records."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ops.decode_jpeg(batch, check=False)
            torch.cuda.synchronize()
        out = {}
        for ev in prof.events():
            name = ev.name
            if "jpeg_" in name or "emset" in name or "fill" in name.lower():
                key = name.split("jpeg_")[1].split("_kernel")[0] if "jpeg_" in name else "memset"
                out[key] = out.get(key, 0.0) + float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
        return out
    except Exception as e:      # the profiler is a convenience here, not a requirement
        return {"unavailable": repr(e)[:80]}


def device_bench(files, label, pil_rgb):
    for n in (32, 256, 1024):
        batch_host = jpeg.JpegBatch.from_files([files[i % DISTINCT] for i in range(n)])
        batch = batch_host.to(dev)
        got, status = ops.decode_jpeg(batch, check=False)
        assert int(status.abs().sum()) == 0
        if pil_rgb is not None and n == 32:
            say(f"{label}: bit-equal to Pillow on all {DISTINCT} distinct images: "
                f"{bool(torch.equal(got.cpu(), torch.from_numpy(pil_rgb)))}")
        runs = events(lambda: ops.decode_jpeg(batch, check=False))
        med = statistics.median(runs)
        say(f"{label}, {n:4d} files ({batch.scan.numel() / n / 1e3:.1f} kB of scan each, {batch.segments.shape[0] // n} "
            f"segment(s) per image): {spread(runs, 'ms')}; {n / med:8.1f} images/ms = {1e3 * n / med:9.0f} images/s")
        st = stage_times(batch)
        say("    one call by stage (us): " + ", ".join(f"{k} {v:.0f}" if isinstance(v, float) else f"{k} {v}"
                                                      for k, v in sorted(st.items())))


def host_bench(files, label):
    runs = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        jpeg.JpegBatch.from_files([files[i % DISTINCT] for i in range(256)])
        runs.append((time.perf_counter() - t0) * 1e3 / 256)
    say(f"{label}: jpeg.parse + packing on one host thread, per image: {spread(runs, 'ms')}")


def pil_bench(files):
    runs = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for f in files:
            jpeg.decode_on_host(f)
        runs.append((time.perf_counter() - t0) * 1e3 / len(files))
    say(f"Pillow on one host thread, Image.open(...).convert('RGB'), per image: {spread(runs, 'ms')}; "
        f"{1e3 / statistics.median(runs):.0f} images/s per thread")


def end_to_end(files, label):
    import hubconf
    from ibl.evaluators import extract_features
    from ibl.utils.data import get_transformer_test
    from ibl.utils.data.preprocessor import Preprocessor
    from openibl_amd import synth
    n = 1024
    with tempfile.TemporaryDirectory() as td:
        records = []
        for i in range(n):
            (Path(td) / f"{i:05d}.jpg").write_bytes(files[i % DISTINCT].tobytes())
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
            for name, loader, kw in (("host-decoding uint8 loader", host, {}),
                                     ("raw-bytes loader + input_decode", raw, {"input_decode": True})):
                for rep in range(2):      # the second pass: graphs captured, workspaces sized
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    feats = extract_features(model, loader, records, gpu=dev.index, print_freq=10 ** 9, **kw)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                res[name] = feats
                say(f"{label}, extract_features, {precision}, {n} files, 8 workers, {name}: {dt:.3f} s = "
                    f"{n / dt:7.0f} images/s")
            a, b = res.values()
            say(f"    descriptors bit-equal between the two loaders: {all(torch.equal(a[k], b[k]) for k in a)}; "
                f"f16mx range fallbacks of the model so far: {model.base_model.range_fallbacks}")


if __name__ == "__main__":
    say(f"{torch.cuda.get_device_name(dev)}, torch {torch.__version__}")
    try:
        import PIL
        say(f"Pillow {PIL.__version__}")
    except ImportError:
        sys.exit("the files of this benchmark are written by Pillow, which cannot be imported here")
    imgs = photos(DISTINCT)
    plain = [encode(im) for im in imgs]
    rows = [encode(im, restart_marker_rows=1) for im in imgs]
    pil_rgb = np.stack([jpeg.decode_on_host(f) for f in plain])
    device_bench(plain, "no restarts", pil_rgb)
    device_bench(rows, "restart per MCU row", np.stack([jpeg.decode_on_host(f) for f in rows]))
    host_bench(plain, "no restarts")
    host_bench(rows, "restart per MCU row")
    pil_bench(plain)
    end_to_end(plain, "no restarts")
    end_to_end(rows, "restart per MCU row")
    if len(sys.argv) > 1:
        Path(sys.argv[1]).write_text("\n".join(LINES) + "\n")
