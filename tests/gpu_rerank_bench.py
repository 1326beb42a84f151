"""k-reciprocal re-ranking from descriptors on the device, stage by stage (diagnostic, not a pytest):
  (a) openibl_amd.rerank.re_ranking_features at Pitts30k-test size (6816 x 10000) and Pitts250k-test size
      (8280 x 83952), 4096-d, k1 = 25, k2 = 1, lambda = 0 (the Evaluator's setting): device time of every stage and
      of the whole call — HIP events, one warm-up call, the median of the following calls — and the peak device
      memory the call adds;
  (b) the host flow it replaces (three dense matrices on the device, their download, openibl_amd.rerank.re_ranking
      in numpy) at 2048 x 8192, the largest size at which it finishes in a few minutes: wall time, once.
Descriptors: unit vectors around "places" of four gallery views each, queries near a view, generated on the device.
    python tests/gpu_rerank_bench.py [--out FILE] [--sizes 6816x10000,8280x83952] [--host 2048x8192 | --host none]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import ops  # noqa: E402
from openibl_amd import rerank as rr  # noqa: E402
from openibl_amd.models import default_precision  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--sizes", default="6816x10000,8280x83952")
ap.add_argument("--host", default="2048x8192")
ap.add_argument("--precision", default="f16mx")
ap.add_argument("--iters", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
K1, K2, LAM, D = 25, 1, 0.0, 4096
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def problem(nq, ng, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    places = torch.nn.functional.normalize(torch.randn(((ng + 3) // 4, D), generator=g, device=dev), dim=1)
    amp = 0.6 / D ** 0.5
    gal = torch.nn.functional.normalize(places.repeat_interleave(4, 0)[:ng] +
                                        amp * torch.randn((ng, D), generator=g, device=dev), dim=1)
    pick = torch.randint(0, ng, (nq,), generator=g, device=dev)
    qry = torch.nn.functional.normalize(gal[pick] + 2 * amp * torch.randn((nq, D), generator=g, device=dev), dim=1)
    return qry.contiguous(), gal.contiguous()


class Stages:
    """re_ranking_features with an event pair around every stage (the same calls in the same order)."""

    def __init__(self):
        self.ev = []

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append((name, e))

    def run(self, q, g, precision):
        self.ev = []
        nq, n = q.shape[0], q.shape[0] + g.shape[0]
        half = ops.rerank_half(K1)
        k = max(K1 + 1, half + 1, K2)
        self.mark("start")
        x = torch.cat([q, g]).contiguous()
        route = ops.topk_precision(precision, x.dtype, k)
        prepared = ops.PreparedRows(x, route)
        self.mark("concatenate + prepare rows")
        block = max(256, min(n, (1 << 26) // n // 256 * 256))
        rank = torch.cat([ops.sqdist_topk_prepared(prepared.rows(lo, min(lo + block, n)), prepared, k)[1]
                          for lo in range(0, n, block)])
        del prepared
        name = {ops.BF16: "bf16", ops.F32: "fp32", ops.BF16X3: "bf16x3", ops.F16MX: "f16mx", ops.F16R: "f16r"}[route]
        self.mark(f"neighbour search ({k} nearest of n, {name})")
        norms, rowmax = ops.rerank_row_extremes(x)
        self.mark("row extremes (fp32 n x n x d, no output matrix)")
        idx, cnt = ops.rerank_sets(rank, K1, half)
        self.mark("reciprocal + expanded sets")
        val = ops.rerank_weights(x, norms, rowmax, idx, cnt)
        self.mark("gathered distances -> V")
        if K2 != 1:
            idx, val, cnt = ops.rerank_expand(rank, K2, idx, val, cnt)
            self.mark("k2 expansion")
        inv = ops.rerank_invert(idx, val, cnt)
        self.mark("inverted index")
        dist = ops.pairwise_sqdist(x[:nq], x[nq:], precision=ops.F32)
        self.mark("q x g squared distances (fp32)")
        out = ops.rerank_jaccard(idx, val, cnt, *inv, rowmax, dist, LAM)
        self.mark("Jaccard pass + blend")
        torch.cuda.synchronize()
        ms = [(b[0], a[1].elapsed_time(b[1])) for a, b in zip(self.ev, self.ev[1:])]
        return out, ms, float(cnt.float().mean()), int(cnt.max())


say(f"k-reciprocal re-ranking from descriptors, d = {D}, k1 = {K1}, k2 = {K2}, lambda = {LAM}, neighbour search "
    f"asked as '{args.precision}' (package default: '{default_precision()}'); {torch.cuda.get_device_name(0)}")
for size in [s for s in args.sizes.split(",") if s]:
    nq, ng = map(int, size.split("x"))
    q, g = problem(nq, ng, 11)
    st = Stages()
    out, _, mean_set, max_set = st.run(q, g, args.precision)                  # warm-up (workspaces, code objects)
    ref = rr.re_ranking_features(q, g, k1=K1, k2=K2, lambda_value=LAM, precision=args.precision)
    same = torch.equal(out, ref)
    del out, ref
    runs = [st.run(q, g, args.precision)[1] for _ in range(args.iters)]
    say()
    say(f"{nq} x {ng} (n = {nq + ng}): members per item mean {mean_set:.1f}, max {max_set}; staged run equals "
        f"re_ranking_features bit for bit: {same}")
    total = 0.0
    for i, (name, _) in enumerate(runs[0]):
        med = statistics.median(r[i][1] for r in runs)
        lo, hi = min(r[i][1] for r in runs), max(r[i][1] for r in runs)
        total += med
        say(f"  {name:<58s} {med:10.3f} ms   ({lo:.3f} .. {hi:.3f})")
    say(f"  {'sum of the stage medians':<58s} {total:10.3f} ms")
    ops.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    out = rr.re_ranking_features(q, g, k1=K1, k2=K2, lambda_value=LAM, precision=args.precision)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    added = torch.cuda.max_memory_allocated(dev) - before
    say(f"  re_ranking_features, one call from released workspaces: {wall * 1e3:.1f} ms wall; peak device memory added "
        f"{added / 1e9:.2f} GB (result {out.numel() * 4 / 1e9:.2f} GB; one n x n float32 array would be "
        f"{(nq + ng) ** 2 * 4 / 1e9:.2f} GB, the host flow builds two)")
    del out, q, g

if args.host != "none":
    nq, ng = map(int, args.host.split("x"))
    q, g = problem(nq, ng, 12)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prec = ops.topk_precision(args.precision, torch.float32, 10)
    prec = ops.F16MX if prec == ops.F16R else prec
    mats = [ops.pairwise_sqdist(a, b, prec).cpu().numpy() for a, b in ((q, g), (q, q), (g, g))]
    t1 = time.perf_counter()
    host = rr.re_ranking(*mats, k1=K1, k2=K2, lambda_value=LAM)
    t2 = time.perf_counter()
    devout = rr.re_ranking_features(q, g, k1=K1, k2=K2, lambda_value=LAM, precision=args.precision)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    diff = (devout.cpu() - torch.from_numpy(host)).abs()
    say()
    say(f"host flow at {nq} x {ng}: three matrices + download {t1 - t0:.2f} s, re_ranking (numpy) {t2 - t1:.1f} s; "
        f"the device call on the same descriptors {(t3 - t2) * 1e3:.1f} ms wall; entries differing by more than 1e-5: "
        f"{float((diff > 1e-5).float().mean()):.4%}")

if args.out:
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
