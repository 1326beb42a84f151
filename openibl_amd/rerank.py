"""k-reciprocal re-ranking of a distance matrix (f4: a host-side caller of the matching path).

Mirror of `ibl.utils.rerank.re_ranking` (ibl/utils/rerank.py:32-100; Zhong et al., CVPR 2017), the
optional post-processing `Evaluator.evaluate(rerank=True)` applies to the query x gallery matrix
(ibl/evaluators.py:190-200).  The reference runs it in numpy on the host over the dense
(Q+G) x (Q+G) matrix; so does this module — the three distance matrices it consumes come from the
HIP distance kernel.  Same parameters, same return value ([Q][G] float32).

The algorithm, in the order the reference applies it:
  1. D = [[qq, qg], [qgT, gg]] ** 2, every column divided by its maximum, then transposed.
  2. R(i) = the k1+1 nearest items of i;  i and j are k-reciprocal iff j in R(i) and i in R(j).
     The reciprocal set of i is expanded by the (k1/2-sized) reciprocal set of each member whose
     overlap with it exceeds 2/3 of its own size.
  3. V[i, j] = exp(-D[i, j]) over that set, normalised to sum 1 (a sparse soft encoding of i).
  4. k2 > 1: every V[i] is replaced by the mean encoding of i's k2 nearest items.
  5. Jaccard distance of the encodings, J[i, j] = 1 - s / (2 - s), s = sum_c min(V[i, c], V[j, c]);
     result = (1 - lambda) * J + lambda * D for query rows / gallery columns.

`re_ranking_features(q, g, ...)` computes the same matrix on the device from the descriptor rows: the k1 + 1
nearest items come from the fused distance + top-k kernels, the column maxima from a contraction that keeps only
row extremes, a few dozen distances per item are recomputed from its rows, and everything after that is sparse
(csrc/rerank.hip) — no (Q+G) x (Q+G) array exists at any point, so it serves any gallery the top-k path serves.
`re_ranking` stays the host mirror of the reference and is what the device path is tested against.
"""
from __future__ import annotations

import numpy as np

__all__ = ["re_ranking", "re_ranking_features"]


def _nearest(D: np.ndarray, k: int) -> np.ndarray:
    """Indices of the k smallest entries of every row in ascending order (ties: lowest index)."""
    n = D.shape[1]
    k = min(k, n)
    part = np.argpartition(D, k - 1, axis=1)[:, :k] if k < n else np.tile(np.arange(n), (D.shape[0], 1))
    vals = np.take_along_axis(D, part, axis=1)
    order = np.lexsort((part, vals), axis=1)
    return np.take_along_axis(part, order, axis=1).astype(np.int32)


def _reciprocal(rank: np.ndarray, i: int, k: int) -> np.ndarray:
    """Members j of the k+1 nearest of i that have i among their own k+1 nearest."""
    fwd = rank[i, : k + 1]
    back = rank[fwd, : k + 1]
    return fwd[(back == i).any(axis=1)]


def re_ranking(q_g_dist, q_q_dist, g_g_dist, k1=20, k2=6, lambda_value=0.3):
    q_g = np.asarray(q_g_dist, dtype=np.float32)
    q_q = np.asarray(q_q_dist, dtype=np.float32)
    g_g = np.asarray(g_g_dist, dtype=np.float32)
    nq, ng = q_g.shape
    n = nq + ng
    D = np.empty((n, n), dtype=np.float32)
    D[:nq, :nq], D[:nq, nq:], D[nq:, :nq], D[nq:, nq:] = q_q, q_g, q_g.T, g_g
    D = np.power(D, 2).astype(np.float32)
    D = np.ascontiguousarray((D / D.max(axis=0)).T)

    half = int(np.around(k1 / 2.0))
    rank = _nearest(D, max(k1 + 1, half + 1, k2))
    V = np.zeros((n, n), dtype=np.float32)
    for i in range(n):
        base = _reciprocal(rank, i, k1)
        members = [base]
        for cand in base:
            sub = _reciprocal(rank, int(cand), half)
            if len(np.intersect1d(sub, base)) > 2.0 / 3.0 * len(sub):
                members.append(sub)
        idx = np.unique(np.concatenate(members))
        w = np.exp(-D[i, idx])
        V[i, idx] = w / w.sum()
    if k2 != 1:
        V = np.stack([V[rank[i, :k2]].mean(axis=0) for i in range(n)]).astype(np.float32)

    # s[i, j] = sum_c min(V[i, c], V[j, c]) for the query rows, walking only the non-zero columns
    cols = [np.nonzero(V[:, c])[0] for c in range(n)]
    jac = np.zeros((nq, n), dtype=np.float32)
    for i in range(nq):
        s = np.zeros(n, dtype=np.float32)
        for c in np.nonzero(V[i])[0]:
            rows = cols[c]
            s[rows] += np.minimum(V[i, c], V[rows, c])
        jac[i] = 1.0 - s / (2.0 - s)
    final = jac * (1.0 - lambda_value) + D[:nq] * lambda_value
    return final[:, nq:]


def re_ranking_features(q, g, k1=20, k2=6, lambda_value=0.3, precision=None):
    """k-reciprocal re-ranking from descriptors on the device: q [Q][d], g [G][d] (float32, or the float16 /
    bfloat16 stored forms the matching path accepts) -> [Q][G] float32 device tensor, the matrix
    re_ranking(q_g_dist, q_q_dist, g_g_dist, k1, k2, lambda_value) returns for their squared-L2 distances.

    `precision` (default: the package's default precision) selects the route of the neighbour search only
    (ops.topk_precision, ops.sqdist_topk of [q; g] against itself; ties: lowest index first).  The column maxima,
    the gathered distances and the q x g distances of the lambda term always run in fp32, so the values do not
    depend on it.  Memory: the fp32 rows of [q; g], O(n (k1 + 1)(round(k1 / 2) + 2)) sparse entries (times k2 when
    k2 > 1) and the [Q][G] result.  Limits: k1 <= 31, k2 <= 8 (ValueError beyond)."""
    import torch

    from . import ops
    from .lib import OpenIBLAmdError
    from .models import default_precision

    ops.rerank_check_limits(k1, k2)
    k1, k2 = int(k1), int(k2)
    if not (torch.is_tensor(q) and torch.is_tensor(g)) or q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError("re_ranking_features expects tensors q [Q][d] and g [G][d]")
    if q.dtype != g.dtype or q.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError("re_ranking_features: q and g must share one of float32, float16, bfloat16")
    if not (q.is_cuda and g.is_cuda):
        raise OpenIBLAmdError("openibl_amd: re_ranking_features runs only on an AMD GPU through the HIP extension; "
                              "openibl_amd.rerank.re_ranking is the host implementation")
    nq, ng = int(q.shape[0]), int(g.shape[0])
    n = nq + ng
    if nq == 0 or ng == 0:
        return torch.empty((nq, ng), dtype=torch.float32, device=q.device)
    half = ops.rerank_half(k1)
    k = max(k1 + 1, half + 1, k2)
    stored = torch.cat([q, g]).contiguous()                     # X = [q; g] in its storage type
    route = ops.topk_precision(precision or default_precision(), stored.dtype, k)
    # the neighbour search: X prepared once, matched against itself in blocks of rows so that the top-k
    # workspace (distance tiles / candidate lists per query row) stays a fraction of the rows themselves
    prepared = ops.PreparedRows(stored, route)
    block = max(256, min(n, (1 << 26) // n // 256 * 256))
    rank = torch.cat([ops.sqdist_topk_prepared(prepared.rows(lo, min(lo + block, n)), prepared, k)[1]
                      for lo in range(0, n, block)])
    x = ops._pad_dim(stored.float() if stored.dtype != torch.float32 else stored)   # 16-bit rows widen exactly
    del stored, prepared
    norms, rowmax = ops.rerank_row_extremes(x)
    idx, cnt = ops.rerank_sets(rank, k1, half)
    val = ops.rerank_weights(x, norms, rowmax, idx, cnt)
    if k2 != 1:
        idx, val, cnt = ops.rerank_expand(rank, k2, idx, val, cnt)
    col_off, inv_row, inv_val = ops.rerank_invert(idx, val, cnt)
    dist = ops.pairwise_sqdist(x[:nq], x[nq:], precision=ops.F32)
    return ops.rerank_jaccard(idx, val, cnt, col_off, inv_row, inv_val, rowmax, dist, lambda_value)
