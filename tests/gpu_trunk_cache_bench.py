"""Re-extraction with the trunk frozen: `TrunkCache.descriptors` against `_extract_local` in the same run (diagnostic,
not a pytest).  512 synthetic 480 x 640 images in batches of 32, EmbedNet with the synthetic weights, f16mx and bf16;
per arithmetic, warm, the median of 7 with the spread, by HIP events and by the wall clock with the device drained:
  (a) the full pass on inputs resident on the device (normalised fp32 batches): what the trunk costs, nothing else;
  (b) the full pass through a loader of pinned host uint8 batches (the cheapest way an image reaches the device);
  (c) the cached pass (conv5 + head per recorded batch), and its two parts alone: the 16 conv5 calls, the 16 heads;
  (d) the fill, once, and the bytes it keeps.
The descriptors of (c) are compared with (a)'s for equality (and a cache filled from the uint8 loader with (b)'s).
The cached pass has to be at least 3x faster than (a): the script exits with status 1 otherwise.
    python tests/gpu_trunk_cache_bench.py [output file, default profiles/trunk_cache_bench.txt]"""
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from openibl_amd import models, ops, synth  # noqa: E402
from openibl_amd.evaluators import _extract_local  # noqa: E402
from openibl_amd.extract import _head_fn  # noqa: E402
from openibl_amd.trunk_cache import TrunkCache  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
N, B, H, W = 512, 32, 480, 640
REPS = 7
FLOOR = 3.0
OUT = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "trunk_cache_bench.txt"
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def spread(runs, unit="ms"):
    return f"median {statistics.median(runs):9.3f} {unit} (min {min(runs):.3f}, max {max(runs):.3f})"


def timed(fn, reps=REPS):
    """One warm-up, then `reps` runs: (HIP-event ms, wall-clock ms with the device drained before and after)."""
    fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(s.elapsed_time(e))
    return ev, wall


def images():
    """uint8 [N][H][W][3] on the device: smooth structure plus noise, as a photograph has; and the loader's
    normalised fp32 NCHW tensor of the same pixels."""
    g = torch.Generator(device=dev).manual_seed(11)
    low = torch.rand((N, 3, H // 32, W // 32), generator=g, device=dev)
    img = torch.nn.functional.interpolate(low, size=(H, W), mode="bilinear", align_corners=False) * 255.0
    img = (img + torch.randn((N, 3, H, W), generator=g, device=dev) * 6.0).round_().clamp_(0, 255)
    u8 = img.permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    mean = torch.tensor(ops.REF_MEAN, device=dev).view(1, 3, 1, 1)
    std = torch.tensor(ops.REF_STD, device=dev).view(1, 3, 1, 1)
    f32 = ((img / 255.0 - mean) / std).contiguous()
    return u8, f32


def main():
    say(f"trunk cache bench: {N} images of {H} x {W}, batches of {B}, EmbedNet (synthetic weights), vlad descriptors; "
        f"{torch.cuda.get_device_name(dev)}; warm, median of {REPS}")
    u8, f32 = images()
    resident = [(f32[i:i + B], None) for i in range(0, N, B)]
    host_u8 = [(u8[i:i + B].cpu().pin_memory(), None) for i in range(0, N, B)]
    dataset = [(i,) for i in range(N)]
    model = models.EmbedNet(models.vgg16(pretrained=False), models.NetVLAD())
    model.load_state_dict(synth.embednet_state(0))
    for l in list(model.base_model.base.children())[:24]:
        for p in l.parameters():
            p.requires_grad_(False)
    model = model.to(dev).eval()
    ok = True
    for prec in ("f16mx", "bf16"):
        model.set_precision(prec)
        say()
        say(f"---- {prec} ----")
        cache = TrunkCache.fill(model, resident, dataset, gpu=dev.index)         # warm-up of the fill
        fills = []
        for _ in range(3):
            del cache
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cache = TrunkCache.fill(model, resident, dataset, gpu=dev.index)
            torch.cuda.synchronize()
            fills.append((time.perf_counter() - t0) * 1e3)
        nbytes = cache.lines.numel() * cache.lines.element_size()
        assert nbytes == TrunkCache.nbytes(N, H, W, prec)
        say(f"(d) fill from resident batches, wall: {spread(fills)}; {nbytes} bytes kept ({nbytes / N} per image), "
            f"batches stored as {sorted(set(t for _, _, t, _ in cache.batches))}, range fallbacks "
            f"{cache.fill_range_fallbacks}")
        full = lambda: _extract_local(model, resident, True, None, dev.index, 1 << 30, 0)       # noqa: E731
        full_u8 = lambda: _extract_local(model, host_u8, True, None, dev.index, 1 << 30, 0)     # noqa: E731
        cached = lambda: cache.descriptors(model, True)                                        # noqa: E731
        want = full()
        got = cached()
        torch.cuda.synchronize()
        say(f"descriptors [{got.shape[0]}][{got.shape[1]}] equal to the full pass on the same batches: "
            f"{torch.equal(got, want)}; conv5 range fallbacks {cache.range_fallbacks}")
        ok = ok and torch.equal(got, want)
        cache8 = TrunkCache.fill(model, host_u8, dataset, gpu=dev.index)
        same8 = torch.equal(cache8.descriptors(model, True), full_u8())
        say(f"cache filled from the uint8 loader equal to the full pass through that loader: {same8}")
        ok = ok and same8
        del cache8, want, got
        ev_a, wall_a = timed(full)
        say(f"(a) full pass, resident fp32 batches:   events {spread(ev_a)}; wall {spread(wall_a)}; "
            f"{N / statistics.median(wall_a) * 1e3:.0f} images/s")
        ev_b, wall_b = timed(full_u8)
        say(f"(b) full pass, host uint8 loader:       events {spread(ev_b)}; wall {spread(wall_b)}; "
            f"{N / statistics.median(wall_b) * 1e3:.0f} images/s")
        ev_c, wall_c = timed(cached)
        say(f"(c) cached pass (conv5 + head):         events {spread(ev_c)}; wall {spread(wall_c)}; "
            f"{N / statistics.median(wall_c) * 1e3:.0f} images/s")
        base = model.base_model
        head = _head_fn(model, True, None, None)

        def conv5_only():
            for row, n, p, _ in cache.batches:
                ws, bs = cache._conv5_packed(base, p)
                ops.vgg16_conv5_from_pool4(cache.lines[row:row + n], ws, bs, p)

        row, n, p, _ = cache.batches[0]
        feat = ops.vgg16_conv5_from_pool4(cache.lines[row:row + n], *cache._conv5_packed(base, p), p)

        def head_only():
            with torch.no_grad():
                for _ in cache.batches:
                    head(feat)

        ev_5, _ = timed(conv5_only)
        ev_h, _ = timed(head_only)
        say(f"    its parts alone, events: {len(cache.batches)} conv5 calls {spread(ev_5)}; {len(cache.batches)} heads "
            f"{spread(ev_h)}")
        r_wall = statistics.median(wall_a) / statistics.median(wall_c)
        r_ev = statistics.median(ev_a) / statistics.median(ev_c)
        r_u8 = statistics.median(wall_b) / statistics.median(wall_c)
        verdict = "met" if r_wall >= FLOOR else "MISSED"
        say(f"ratio (a) / (c): {r_wall:.2f}x by the wall clock, {r_ev:.2f}x by events; (b) / (c): {r_u8:.2f}x by the "
            f"wall clock; floor {FLOOR:.0f}x against (a): {verdict}")
        ok = ok and r_wall >= FLOOR
        del cache, feat
        ops.release_workspaces()
        torch.cuda.empty_cache()
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text("\n".join(LINES) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
