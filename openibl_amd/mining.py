"""Hard-negative mining for the tuple samplers on the device, only for the anchors of the round.

The reference's `update_sampler` (examples/netvlad_img.py:73-83, netvlad_img_sfrs.py:74-94) builds the
whole query x gallery matrix on the host and `sort_gallery` ranks every row of it, although a round visits
`cache_size` anchors; `__iter__` then tests the ranked row of every anchor for membership in its lists.
Here only the anchors' rows are computed, ranked and mined (csrc/mining.hip, `ops.mine_rows`), and what
reaches the host is what `__iter__` looks up: per anchor the candidates in rank order, the places of last
round's negatives among them, and the ranked positives (`MinedRows`).  The samplers of
`ibl.utils.data.sampler` take it with `load_mined` and yield the tuples they yield from `sort_gallery` on
the same distances and the same `random` state.

    from openibl_amd.mining import update_sampler       # in place of the training scripts' own
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .lib import OpenIBLAmdError

from .trunk_cache import TrunkCache

__all__ = ["MinedRows", "mine", "mine_from_features", "update_sampler", "TrunkCache"]


class MinedRows:
    """What one round of mining leaves on the host, one row per anchor (numpy arrays):
    anchors [A] the query indices, cand [A][G] int32 the gallery in rank order without the anchor's
    exclusion zone (-1 behind cand_len [A]), cache_pos [A][neg_num] the places in cand of the negatives the
    sampler cached last round (-1: none), pos_ranked [A][pos_pool] the positives in rank order (-1 behind
    the last), pos_jac [A][pos_pool] the k-reciprocal distance of each (None without such a matrix)."""

    __slots__ = ("anchors", "cand", "cand_len", "cache_pos", "pos_ranked", "pos_jac")

    def __init__(self, anchors, cand, cand_len, cache_pos, pos_ranked, pos_jac=None):
        self.anchors, self.cand, self.cand_len = anchors, cand, cand_len
        self.cache_pos, self.pos_ranked, self.pos_jac = cache_pos, pos_ranked, pos_jac


def csr_lists(lists, G):
    """(offsets [len + 1], values) int32: row i = np.unique(lists[i]) restricted to [0, G) — what
    np.isin(row, lists[i]) tests, where repeats and foreign indices do not matter."""
    rows = []
    for entry in lists:
        v = np.unique(np.asarray(entry, dtype=np.int64).reshape(-1))
        rows.append(v[(v >= 0) & (v < G)].astype(np.int32))
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError("mining: the lists hold 2^31 entries or more")
    val = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int32)
    return off.astype(np.int32), val.astype(np.int32)


def _sampler_lists(sampler, dev):
    """The sampler's two lists in CSR form on `dev`; built once per sampler (its lists are fixed)."""
    held = getattr(sampler, "_mining_lists", None)
    if held is None or held[0] != dev:
        G = len(sampler.gallery_source)
        parts = csr_lists(sampler.pos_list, G) + csr_lists(sampler.neg_list, G)
        held = (dev, tuple(torch.from_numpy(p).to(dev) for p in parts))
        sampler._mining_lists = held
    return held[1]


def _to_host(*tensors):
    """Device tensors -> numpy arrays, each copied once through pinned memory, one synchronisation."""
    out = []
    for t in tensors:
        if t is None:
            out.append(None)
            continue
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        out.append(h)
    torch.cuda.current_stream(next(t for t in tensors if t is not None).device).synchronize()
    return [None if h is None else h.numpy() for h in out]


def mine(dist_rows, anchors, sampler, jac_rows=None, max_ws_bytes=1 << 31):
    """Mine the rows dist_rows [A][G] (float32, device) of the query indices `anchors` for `sampler`
    (its pos_list, neg_list, neg_cache, neg_num and, on the SFRS sampler, pos_pool) -> MinedRows.
    jac_rows [A][G] (float32, device): the k-reciprocal distances of the same rows, for pos_jac."""
    if not (torch.is_tensor(dist_rows) and dist_rows.is_cuda):
        raise OpenIBLAmdError("openibl_amd: mining runs only on an AMD GPU through the HIP extension; "
                              "sampler.sort_gallery is the flow with the bookkeeping on the host")
    anchors = [int(a) for a in anchors]
    A, G = len(anchors), len(sampler.gallery_source)
    if tuple(dist_rows.shape) != (A, G):
        raise ValueError(f"mine: dist_rows is {tuple(dist_rows.shape)}, expected ({A}, {G})")
    if anchors and not 0 <= min(anchors) <= max(anchors) < len(sampler.query_source):
        raise ValueError("mine: anchors must index sampler.query_source")
    C = int(sampler.neg_num)
    if C > ops.MINE_MAX_CACHE:
        raise ValueError(f"mine: neg_num = {C} exceeds the kernel's {ops.MINE_MAX_CACHE} cached negatives")
    dev = dist_rows.device
    pos_off, pos_val, excl_off, excl_val = _sampler_lists(sampler, dev)
    cache = np.full((A, C), -1, dtype=np.int32)
    for i, a in enumerate(anchors):
        held = sampler.neg_cache[a][:C]
        cache[i, :len(held)] = held
    out = ops.mine_rows(dist_rows, pos_off, pos_val, excl_off, excl_val, cache=torch.from_numpy(cache).to(dev),
                        pos_pool=int(getattr(sampler, "pos_pool", 1)), jac=jac_rows,
                        csr_row=torch.as_tensor(anchors, dtype=torch.int32, device=dev),
                        max_ws_bytes=max_ws_bytes)
    if A == 0:
        return MinedRows(np.zeros(0, dtype=np.int64), *(None if t is None else t.cpu().numpy() for t in out))
    return MinedRows(np.asarray(anchors, dtype=np.int64), *_to_host(*out))


def mine_from_features(q_desc, g_desc, sub_set, sampler, rerank=False, lambda_value=0.1, precision=None):
    """Mine a round from descriptors on the device: q_desc [Q][d], g_desc [G][d] -> MinedRows for the anchors
    `sampler` visits on this replica when `sub_set` is the round's subset (sampler.mining_anchors).

    Only the anchors' rows of the distance matrix are computed: the `ops.pairwise_sqdist(x, y, precision)`
    call of `pairwise_distance`, on q_desc[anchors].  For the SFRS sampler the k-reciprocal distances are the
    same rows (rerank=False, as in the training script) or the anchors' rows of
    re_ranking_features(q_desc, g_desc, k1=20, k2=1, lambda_value), which stays on the device."""
    from .models import default_precision
    if not (torch.is_tensor(q_desc) and torch.is_tensor(g_desc) and q_desc.is_cuda and g_desc.is_cuda):
        raise OpenIBLAmdError("openibl_amd: mine_from_features runs only on an AMD GPU through the HIP extension "
                              "(descriptors on the device); there is no CPU fallback")
    if int(q_desc.shape[0]) != len(sampler.query_source) or int(g_desc.shape[0]) != len(sampler.gallery_source):
        raise ValueError("mine_from_features: descriptors and the sampler's sources differ in length")
    prec = precision or default_precision()
    anchors = sampler.mining_anchors(sub_set)
    at = torch.as_tensor(anchors, dtype=torch.long, device=q_desc.device)
    rows = ops.pairwise_sqdist(q_desc[at].float().contiguous(), g_desc.float().contiguous(), prec)
    jac_rows = None
    if hasattr(sampler, "pos_pool"):
        jac_rows = rows
        if rerank:
            from .rerank import re_ranking_features
            jac_rows = re_ranking_features(q_desc.contiguous(), g_desc.contiguous(), k1=20, k2=1,
                                           lambda_value=lambda_value, precision=prec)[at].contiguous()
    return mine(rows, anchors, sampler, jac_rows=jac_rows)


def update_sampler(sampler, model, loader, query, gallery, sub_set, rerank=False, vlad=True, gpu=None,
                   sync_gather=False, lambda_value=0.1, trunk_cache=None, input_resize=None, input_decode=None):
    """The `update_sampler` of examples/netvlad_img.py and netvlad_img_sfrs.py with the descriptors, the
    distances and the mining on the device: extract over sorted(set(query) | set(gallery)) (`loader`'s
    dataset, as in the scripts), look the rows up by file name, mine this round's anchors, load the sampler.
    `rerank` only matters to the SFRS sampler.  Single rank (`sync_gather` has nothing to gather).
    trunk_cache: a `TrunkCache` filled from `loader` over that dataset while conv4 and below are frozen: the
    descriptors then come from its stored pool4 maps (conv5 and the head with the live parameters, the same bits),
    `loader` is not iterated and no image is decoded; everything behind the extraction is unchanged.
    input_resize: as in `extract_features` — `loader` delivers raw uint8 batches at their stored size, resized on the
    device (a trunk cache was filled behind the same resize: `TrunkCache.fill(..., input_resize=...)`).
    input_decode: as in `extract_features` — `loader` delivers the files' bytes as JpegBatch batches, decoded on the
    device in front of the resize; MixedJpegBatch batches (files of mixed stored sizes, `jpeg.collate_mixed`) need
    input_resize=(height, width) and are decoded and resized in one step."""
    from .evaluators import _extract_local, _rank_world
    rank, world = _rank_world()
    if world != 1:
        raise RuntimeError(
            f"mining.update_sampler: mining on the device runs on a single rank (world size {world}): the "
            "descriptors are not gathered between devices yet; use the host flow (extract_features + "
            "pairwise_distance + sampler.sort_gallery)")
    if not torch.cuda.is_available():
        raise OpenIBLAmdError("openibl_amd: mining.update_sampler runs only on an AMD GPU through the HIP "
                              "extension (there is no CPU fallback)")
    if rank == 0:
        print("===> Start extracting features for sorting gallery")
    dataset = sorted(list(set(query) | set(gallery)))
    if trunk_cache is not None:
        trunk_cache.check(model, len(dataset))
        feats = trunk_cache.descriptors(model, vlad)
    else:
        feats = _extract_local(model, loader, vlad, None, gpu, 10, rank, input_resize=input_resize,
                               input_decode=input_decode)[:len(dataset)]
    where = {f: i for i, (f, *_) in enumerate(dataset)}
    q_feat = feats[torch.as_tensor([where[f] for f, *_ in query], device=feats.device)]
    g_feat = feats[torch.as_tensor([where[f] for f, *_ in gallery], device=feats.device)]
    del feats
    if rank == 0:
        print("===> Start sorting gallery")
    sampler.load_mined(mine_from_features(q_feat, g_feat, sub_set, sampler, rerank=rerank,
                                          lambda_value=lambda_value), sub_set)
