"""numpy mirror of oibl_mine_rows (include/openibl_amd.h): the yardstick for every integer output of the
mining entry, and a host stand-in for it where a test has no GPU.  Plain restatement of the contract:
np.argsort(kind="stable") for the rank order, np.isin for membership, positions by search."""
import numpy as np


def mine_rows(dist, pos_lists, excl_lists, cache=None, pos_pool=1, jac=None):
    """dist [A][G]; pos_lists / excl_lists: one sequence per anchor (any order, repeats and foreign indices
    allowed, as np.isin takes them); cache [A][C] int (-1: none) or None; jac [A][G] or None.
    -> dict(cand [A][G], cand_len [A], cache_pos [A][C], pos_ranked [A][pos_pool], pos_jac [A][pos_pool] or None)"""
    dist = np.asarray(dist, dtype=np.float32)
    A, G = dist.shape
    C = 0 if cache is None else np.asarray(cache).shape[1]
    cand = np.full((A, G), -1, dtype=np.int32)
    cand_len = np.zeros(A, dtype=np.int32)
    cache_pos = np.full((A, C), -1, dtype=np.int32)
    pos_ranked = np.full((A, pos_pool), -1, dtype=np.int32)
    pos_jac = None if jac is None else np.full((A, pos_pool), np.nan, dtype=np.float32)
    for a in range(A):
        ranked = np.argsort(dist[a], kind="stable").astype(np.int32)
        kept = ranked[~np.isin(ranked, np.asarray(excl_lists[a], dtype=np.int64))]
        cand[a, :len(kept)] = kept
        cand_len[a] = len(kept)
        for c in range(C):
            hit = np.nonzero(kept == cache[a][c])[0] if cache[a][c] >= 0 else []
            if len(hit):
                cache_pos[a, c] = hit[0]
        pr = ranked[np.isin(ranked, np.asarray(pos_lists[a], dtype=np.int64))][:pos_pool]
        pos_ranked[a, :len(pr)] = pr
        if jac is not None:
            pos_jac[a, :len(pr)] = np.asarray(jac, dtype=np.float32)[a][pr]
    return dict(cand=cand, cand_len=cand_len, cache_pos=cache_pos, pos_ranked=pos_ranked, pos_jac=pos_jac)


def mine_for_sampler(sampler, dist, anchors, jac=None):
    """openibl_amd.mining.mine on the host: MinedRows for `anchors` from the full [Q][G] matrices."""
    from openibl_amd.mining import MinedRows
    dist = np.asarray(dist, dtype=np.float32)
    C = sampler.neg_num
    cache = np.full((len(anchors), C), -1, dtype=np.int32)
    for i, a in enumerate(anchors):
        held = sampler.neg_cache[a][:C]
        cache[i, :len(held)] = held
    out = mine_rows(dist[anchors], [sampler.pos_list[a] for a in anchors], [sampler.neg_list[a] for a in anchors],
                    cache, int(getattr(sampler, "pos_pool", 1)),
                    None if jac is None else np.asarray(jac, dtype=np.float32)[anchors])
    return MinedRows(np.asarray(anchors, dtype=np.int64), out["cand"], out["cand_len"], out["cache_pos"],
                     out["pos_ranked"], out["pos_jac"])
