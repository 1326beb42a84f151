"""The two kernels of the NetVLAD initialisation at the reference's sizes (diagnostic, not a pytest):
  (a) oibl_local_descriptors: 100 sampled positions of each of 500 conv5 maps of 30 x 40 x 512 (the 50 000
      descriptors of examples/cluster.py), fp32 and bf16 maps;
  (b) oibl_assign_gap at n = 50 000, K = 64, C = 512 (NetVLAD._init_params), against numpy's evaluation of the same
      step on this machine's CPU (ibl/models/netvlad.py:35-40: normalise, [K][n] dot products, sort, mean top-2 gap).
Both in one process, warm, HIP events around a batch of calls sized far above the timer's resolution, the median of
several such batches with their spread; numpy by the wall clock, median of 3.
    python tests/gpu_netvlad_init_bench.py"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import cluster, lib, ops  # noqa: E402

dev = torch.device("cuda", 0)


def blas_threads():
    """the thread count of the BLAS numpy's dot runs on, as threadpoolctl reports it"""
    from threadpoolctl import threadpool_info
    n = [int(p["num_threads"]) for p in threadpool_info() if p.get("user_api") == "blas"]
    return max(n) if n else "?"


def timed(fn, iters, batches=7):
    """median, min, max over `batches` of the mean microseconds per call of `iters` back-to-back calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(batches):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        runs.append(s.elapsed_time(e) / iters * 1e3)
    return statistics.median(runs), min(runs), max(runs)


# ---- (a) the sampling kernel: the C entry itself, positions already on the device --------------------------------
N, h, w, C, S = 500, 30, 40, 512, 100
P = h * w
handle = lib.load()
pos = torch.from_numpy(cluster.sample_positions(N, P, S, np.random.RandomState(43))).to(torch.int32).to(dev)
out = torch.empty((N * S, C), dtype=torch.float32, device=dev)
for dtype, code in ((torch.float32, ops.F32), (torch.bfloat16, ops.BF16)):
    feat = (torch.randn((N, h, w, C), device=dev) * 3.0).to(dtype)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        lib.check(handle.oibl_local_descriptors(feat.data_ptr(), N, P, C, code, pos.data_ptr(), S, out.data_ptr(), st))

    med, lo, hi = timed(call, iters=50)
    moved = N * S * C * (feat.element_size() + 4)
    print(f"oibl_local_descriptors, {N} maps of {h} x {w} x {C} {str(dtype).split('.')[-1]}, {S} positions each "
          f"({N * S} rows of the {feat.numel() * feat.element_size() / 1e6:.0f} MB map): median {med:7.1f} us "
          f"(min {lo:7.1f}, max {hi:7.1f}) = {moved / med / 1e6:.2f} TB/s of rows read + written", flush=True)
    t0 = time.perf_counter()
    rows = ops.local_descriptors(feat, pos)
    torch.cuda.synchronize()
    print(f"    ops.local_descriptors with its host-side range check of the positions: "
          f"{(time.perf_counter() - t0) * 1e3:.2f} ms per call", flush=True)
    del feat
descs = rows                      # 50 000 unit-norm rows (of the bf16 map)

# ---- (b) assign_gap against numpy --------------------------------------------------------------------------------
n, K = N * S, 64
clsts = descs[torch.from_numpy(np.random.RandomState(1).choice(n, K, replace=False)).to(dev)] * 0.7 \
    + 0.05 * torch.randn((K, C), device=dev)
clsts = clsts.contiguous()
ws = ops.workspace(handle.oibl_assign_gap_workspace_bytes(n, K, C), dev, "assign_gap")
ca = torch.empty((K, C), dtype=torch.float32, device=dev)
gap = torch.empty((n,), dtype=torch.float32, device=dev)
gsum = torch.empty((1,), dtype=torch.float64, device=dev)
st = torch.cuda.current_stream(dev).cuda_stream


def call_gap():
    lib.check(handle.oibl_assign_gap(descs.data_ptr(), n, clsts.data_ptr(), K, C, ca.data_ptr(), gap.data_ptr(),
                                     gsum.data_ptr(), ws.data_ptr(), ws.numel(), st))


med, lo, hi = timed(call_gap, iters=20)
mean_gap = float(gsum.item()) / n
t_end = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.assign_gap(descs, clsts)                 # launches + the 8-byte read of the sum
    t_end.append((time.perf_counter() - t0) * 1e6)

clsts_h, descs_h = clsts.cpu().numpy(), descs.cpu().numpy()


def numpy_step():
    a = clsts_h / np.linalg.norm(clsts_h, axis=1, keepdims=True)
    dots = np.dot(a, descs_h.T)
    dots.sort(0)
    dots = dots[::-1, :]
    return float(-np.log(0.01) / np.mean(dots[0, :] - dots[1, :]))


t_np = []
for _ in range(3):
    t0 = time.perf_counter()
    alpha_np = numpy_step()
    t_np.append((time.perf_counter() - t0) * 1e6)
alpha = -np.log(0.01) / mean_gap
print(f"oibl_assign_gap, n = {n}, K = {K}, C = {C} (3 launches, {2 * n * K * C / 1e9:.1f} GFLOP): median {med:7.1f} us "
      f"(min {lo:7.1f}, max {hi:7.1f}); ops.assign_gap with the read of the mean, wall clock: median "
      f"{statistics.median(t_end):7.1f} us", flush=True)
print(f"numpy, the same step on this machine's CPU ({blas_threads()} BLAS threads): median "
      f"{statistics.median(t_np) / 1e3:7.2f} ms (min {min(t_np) / 1e3:.2f}, max {max(t_np) / 1e3:.2f}) = "
      f"{statistics.median(t_np) / med:.0f}x the kernel time; alpha {alpha:.6f} against numpy's {alpha_np:.6f} "
      f"(relative {abs(alpha - alpha_np) / alpha_np:.1e})", flush=True)
