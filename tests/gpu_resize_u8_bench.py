"""The device resize at the extraction and training shapes (diagnostic, not a pytest).  In one process, warm, the
median of 7 with the spread, by HIP events:
  (a) ops.resize_u8 — the two table launches and the fused resampling launch — at 960 x 1280 -> 480 x 640 with 12
      and 32 images in both output kinds, 480 x 640 -> 480 x 640 (both passes are the identity) and one phone photo
      of 2448 x 3264 -> 480 x 640; the bytes the call must move (input + output) and the TB/s that makes;
  (b) in the same run ops.color_jitter(result, None) on the 480 x 640 result: a pass that writes the same output
      from an input of the target size — the yardstick;
  (c) PIL on the host, one thread, the same resize of one image (if PIL can be imported).
    python tests/gpu_resize_u8_bench.py"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from helpers import resize_u8_ref as ref  # noqa: E402
from openibl_amd import ops  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H2, W2 = 480, 640
REPS = 7


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


def images(n, h, w, seed):
    """Smooth structure plus noise, as a photograph has."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(xx / 37.0 + c) * np.cos(yy / 53.0 - c) for c in range(3)], -1)
    out = np.empty((n, h, w, 3), dtype=np.uint8)
    for i in range(n):
        out[i] = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    return out


def shape_bench(n, h, w, check_pil):
    x_host = images(n, h, w, n + h)
    x = torch.from_numpy(x_host).to(dev)
    print(f"---- {n} images of {h} x {w} -> {H2} x {W2} ----", flush=True)
    small = ops.resize_u8(x, (H2, W2), out="uint8")
    for out, out_bytes in (("float", 12), ("uint8", 3)):
        runs = events(lambda: ops.resize_u8(x, (H2, W2), out=out))
        ref_runs = events(lambda: ops.color_jitter(small, None, out=out))
        moved = n * (h * w * 3 + H2 * W2 * out_bytes)
        med = statistics.median(runs)
        print(f"ops.resize_u8 out={out:5s}: {spread(runs, 'ms')}; {moved / 1e6:7.1f} MB moved, "
              f"{moved / med / 1e9:6.3f} TB/s; {n * H2 * W2 / med / 1e3:7.1f} output Mpixel/s", flush=True)
        print(f"  ops.color_jitter(result, None) out={out:5s}: {spread(ref_runs, 'ms')}", flush=True)
    if check_pil:
        try:
            want = ref.pil_resize(x_host[0], H2, W2)
        except ImportError:
            print("PIL is not importable here: no host figure, no bit check", flush=True)
            return
        print(f"bit-equal to PIL on the first image: {np.array_equal(small[0].cpu().numpy(), want)}", flush=True)
        runs = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            ref.pil_resize(x_host[0], H2, W2)
            runs.append((time.perf_counter() - t0) * 1e3)
        print(f"PIL on the host, one thread, one image (array -> Image -> resize -> array): {spread(runs, 'ms')}; "
              f"{1e3 / statistics.median(runs):.1f} images/s per thread", flush=True)


if __name__ == "__main__":
    print(f"{torch.cuda.get_device_name(dev)}, torch {torch.__version__}", flush=True)
    shape_bench(12, 960, 1280, True)
    shape_bench(32, 960, 1280, False)
    shape_bench(12, 480, 640, True)
    shape_bench(1, 2448, 3264, True)
