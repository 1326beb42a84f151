"""Generate tests/golden/netvlad_init.npz by running THE REFERENCE's NetVLAD._init_params.

Run in the build container only (`python tests/helpers/make_netvlad_init_golden.py`): the reference tree is imported
through oracle.refshim, exactly as make_region_golden.py does, and does not exist on the GPU box.

What is exercised, through the reference's own code object:
  pool = models.create('netvlad', num_clusters=K, dim=C); pool.clsts, pool.traindescs = ...; pool._init_params()
                                                                                  (ibl/models/netvlad.py:34-42)
Each case draws n seeded unit-norm descriptors and takes perturbed descriptors as the K centres (so every centre
has descriptors near it and the top-2 gap is an O(0.1) quantity, as after a k-means), and stores the inputs `clsts`,
`traindescs` and the reference's results `alpha`, `centroids`, `conv_weight` under `<case>_<name>`; `cases` lists
the case names.  The n = 1 case uses well-separated centres (centre 0 the descriptor, centre 1 its negative): a
near-tie of the top pair of a single descriptor is ill-conditioned (alpha = 4.6 / gap).  The inputs are drawn on
a grid of 14 significant bits (the descriptors are unit-norm to 2e-5), which keeps the compressed file under 500 KB;
the reference's outputs are stored as it computed them.

Every stored case is checked here: the reference's fp32 alpha and conv_weight lie within 1e-5 (relative) of a float64
evaluation of the same formula on the same inputs — the 1e-4 bar of the GPU tests is then a bar on the kernel, not on
the conditioning of the case.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from oracle import refshim  # noqa: E402

refshim.install()  # puts the reference FIRST on sys.path: `import ibl` below is the reference

OUT = ROOT / "tests" / "golden" / "netvlad_init.npz"
CASES = (("k64", 64, 128, 257, 101), ("k20", 20, 128, 257, 102), ("k2_n1", 2, 64, 1, 103), ("k256", 256, 64, 300, 104))


def grid(a):
    """float32 values rounded to 14 significant bits (the low 10 mantissa bits are zero: 3e-5 relative)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x200)) & np.uint32(0xFFFFFC00)).view(np.float32)


def inputs(K, C, n, seed):
    rng = np.random.RandomState(seed)
    d = rng.randn(n, C)
    d = grid(d / np.linalg.norm(d, axis=1, keepdims=True))
    if n == 1:
        clsts = np.concatenate([d, -d]).astype(np.float32)          # well separated: gap = 2
    else:
        pick = rng.choice(n, K, replace=K > n)
        clsts = grid(d[pick] * rng.uniform(0.5, 1.5, (K, 1)) + 0.05 * rng.randn(K, C))
    return np.ascontiguousarray(clsts), np.ascontiguousarray(d)


def float64_formula(clsts, descs):
    c, d = clsts.astype(np.float64), descs.astype(np.float64)
    ca = c / np.linalg.norm(c, axis=1, keepdims=True)
    dots = np.sort(ca @ d.T, axis=0)[::-1]
    alpha = -np.log(0.01) / np.mean(dots[0] - dots[1])
    return alpha, alpha * ca


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import models

    store = {"cases": np.array([c[0] for c in CASES])}
    for name, K, C, n, seed in CASES:
        clsts, descs = inputs(K, C, n, seed)
        torch.manual_seed(0)
        pool = models.create("netvlad", num_clusters=K, dim=C)
        pool.clsts, pool.traindescs = clsts.copy(), descs.copy()
        pool._init_params()
        alpha = float(pool.alpha)
        cent = pool.centroids.detach().numpy().copy()
        w = pool.conv.weight.detach().numpy().copy()
        assert w.shape == (K, C, 1, 1) and np.array_equal(cent, clsts)
        a64, w64 = float64_formula(clsts, descs)
        da = abs(alpha - a64) / a64
        dw = float(np.linalg.norm(w.reshape(K, C) - w64) / np.linalg.norm(w64))
        print(f"{name}: K {K} C {C} n {n}  alpha {alpha:.6f}  fp32 reference against float64: alpha {da:.1e}, "
              f"conv_weight rel-L2 {dw:.1e}")
        assert da <= 1e-5 and dw <= 1e-5, (name, da, dw)
        store.update({f"{name}_clsts": clsts, f"{name}_traindescs": descs, f"{name}_alpha": np.float64(alpha),
                      f"{name}_centroids": cent, f"{name}_conv_weight": w})
    np.savez_compressed(OUT, **store)
    print(OUT, OUT.stat().st_size, "bytes")
    assert OUT.stat().st_size < 500 * 1024


if __name__ == "__main__":
    main()
