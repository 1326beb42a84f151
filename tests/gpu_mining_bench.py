"""A round of hard-negative mining, the host flow against the device flow (diagnostic, not a pytest), at the
Pitts30k-train shape: Q = 7416 queries, G = 10 000 gallery images (then G = 83 952), A = 1000 anchors per round
(cache_size), neg_pool 1000, neg_num 10, pos_pool 20, 30 positives and 150 excluded entries per query, the negative
cache filled.  In one process, warm, the median of 7 with the spread:
  (a) the round: `sort_gallery` (all Q rows ranked on the device, the int64 ranking copied to the host) against
      `sort_gallery_on_device` on the same host matrix and on a device matrix, and against `mine_from_features` +
      `load_mined` from descriptors on the device (d = 4096; the [Q][G] matrix never exists) — wall clock with the
      device drained, every copy to the host included;
  (b) the device work of ops.mine_rows alone (ranking + mining pass of the A rows), by HIP events;
  (c) the host time of `__iter__` per anchor, both paths from the same `random` state, by the wall clock.
    python tests/gpu_mining_bench.py [G ...]"""
import itertools
import random
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from ibl.utils.data.sampler import DistributedRandomDiffTupleSampler  # noqa: E402
from openibl_amd import mining, ops  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
Q, A, D = 7416, 1000, 4096
REPS = 7


def spread(runs, unit):
    return f"median {statistics.median(runs):9.3f} {unit} (min {min(runs):.3f}, max {max(runs):.3f})"


def wall(fn, reps=REPS):
    fn()
    runs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    return runs


def events(fn, reps=REPS):
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


def bench(G):
    rng = np.random.default_rng(G)
    print(f"---- Q = {Q}, G = {G}, A = {A}, d = {D}, neg_pool 1000, neg_num 10, pos_pool 20 ----", flush=True)
    centre = rng.integers(100, G - 100, size=Q)
    pos = [np.sort(c + rng.choice(np.arange(-20, 21), size=30, replace=False)).tolist() for c in centre]
    neg = [list(range(c - 75, c + 75)) for c in centre]
    g = torch.nn.functional.normalize(torch.randn((G, D), device=dev), dim=1)
    q = torch.nn.functional.normalize(g[torch.from_numpy(centre).to(dev)] + 0.5 * torch.nn.functional.normalize(
        torch.randn((Q, D), device=dev), dim=1), dim=1)
    dist_dev = ops.pairwise_sqdist(q, g, "fp32")
    dist_host = dist_dev.cpu()
    sub = random.Random(1).sample(range(Q), A)

    def make():
        return DistributedRandomDiffTupleSampler(list(range(Q)), list(range(G)), pos, neg, pos_num=10, pos_pool=20,
                                                 neg_num=10, neg_pool=1000, num_replicas=1, rank=0)
    old, new = make(), make()
    # fill the negative cache: one round on the new path, its cache handed to the old sampler
    new.sort_gallery_on_device(dist_dev, dist_dev, sub)
    random.seed(5)
    for _ in iter(new):
        pass
    old.neg_cache = [list(c) for c in new.neg_cache]

    # (a) the round
    t_old = wall(lambda: old.sort_gallery(dist_host, dist_host, sub))
    print(f"round, sort_gallery (host matrix, {Q} rows ranked, {Q * G * 8 / 1e6:.0f} MB int64 to the host): "
          f"{spread(t_old, 'ms')}", flush=True)
    t_new_h = wall(lambda: new.sort_gallery_on_device(dist_host, dist_host, sub))
    print(f"round, sort_gallery_on_device (host matrix, {A} rows gathered and mined, {A * G * 4 / 1e6:.0f} MB int32 "
          f"to the host): {spread(t_new_h, 'ms')}", flush=True)
    t_new_d = wall(lambda: new.sort_gallery_on_device(dist_dev, dist_dev, sub))
    print(f"round, sort_gallery_on_device (device matrix): {spread(t_new_d, 'ms')}", flush=True)
    t_feat = wall(lambda: new.load_mined(mining.mine_from_features(q, g, sub, new, precision="fp32"), sub))
    print(f"round, mine_from_features + load_mined (descriptors on the device, fp32 distances of the {A} rows): "
          f"{spread(t_feat, 'ms')}", flush=True)

    # (b) the device work alone
    lists = mining._sampler_lists(new, dev)
    rows_at = torch.as_tensor(sub, dtype=torch.int32, device=dev)
    rows = dist_dev[rows_at.long()].contiguous()
    cache = torch.from_numpy(np.asarray([new.neg_cache[a] for a in sub], dtype=np.int32)).to(dev)
    t_dev = events(lambda: ops.mine_rows(rows, *lists, cache=cache, pos_pool=20, jac=rows, csr_row=rows_at))
    print(f"ops.mine_rows, {A} x {G} (ranking + mining pass, with its one check of the lists), HIP events: "
          f"{spread(t_dev, 'ms')}", flush=True)

    # (c) __iter__ per anchor: the first `take` anchors of the round, both paths from one random state
    take = 200 if G <= 20000 else 50
    old.neg_cache = [list(c) for c in new.neg_cache]
    held = [list(c) for c in new.neg_cache]
    per = {"ranking": [], "mined": []}
    same = True
    for rep in range(REPS):
        out = {}
        for name, smp in (("ranking", old), ("mined", new)):
            smp.neg_cache = [list(c) for c in held]
            if name == "mined":
                new.sort_gallery_on_device(dist_dev, dist_dev, sub)   # places of the cache as held
            random.seed(100 + rep)
            t0 = time.perf_counter()
            out[name] = list(itertools.islice(iter(smp), take))
            per[name].append((time.perf_counter() - t0) * 1e3 / take)
        same = same and out["ranking"] == out["mined"]
    print(f"__iter__ per anchor over the ranking ({take} anchors a run): {spread(per['ranking'], 'ms')}", flush=True)
    print(f"__iter__ per anchor over mined rows: {spread(per['mined'], 'ms')}; equal tuples: {same}", flush=True)
    del old, new, dist_host, dist_dev, q, g
    ops.release_workspaces()
    torch.cuda.empty_cache()


for G in ([int(a) for a in sys.argv[1:]] or [10000, 83952]):
    bench(G)
