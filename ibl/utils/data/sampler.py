from __future__ import absolute_import

import torch.distributed as dist
# examples/cluster.py imports SubsetRandomSampler from this module (the reference's sampler.py:9-11
# pulls torch's samplers into its namespace)
from torch.utils.data import BatchSampler  # noqa: F401
from torch.utils.data.sampler import (  # noqa: F401
    RandomSampler, Sampler, SequentialSampler, SubsetRandomSampler, WeightedRandomSampler)

from openibl_amd.sharded import slice_bounds


class DistributedSliceSampler(Sampler):
    """Rank r iterates the contiguous index range [r * per, (r + 1) * per), per = ceil(L / W);
    indices past the end wrap to the start (padding that extract_features drops after the
    gather).  Same dealing as the reference's sampler, which is what makes the gallery shard of
    rank r a contiguous block of gallery positions."""

    def __init__(self, dataset, num_replicas=None, rank=None):
        if num_replicas is None:
            num_replicas = dist.get_world_size()
        if rank is None:
            rank = dist.get_rank()
        self.dataset = dataset
        self.num_replicas = num_replicas
        self.rank = rank
        start, per, _ = slice_bounds(len(dataset), rank, num_replicas)
        self.num_samples = per
        self.total_size = per * num_replicas
        n = len(dataset)
        self._indices = [(start + i) % n for i in range(per)] if n else []

    def __iter__(self):
        return iter(self._indices)

    def __len__(self):
        return self.num_samples


class DistributedRandomTupleSampler(Sampler):
    """Tuples for hard-negative mining — `[anchor, easiest positive, neg_num hardest negatives]`, the
    gallery entries offset by len(query_source) — with the contract of the reference's sampler
    (ibl/utils/data/sampler.py:15-86; examples/netvlad_img.py:42-46).

    What is accelerated is `sort_gallery`: the reference calls `torch.argsort(distmat, dim=1)` over
    the whole query x gallery matrix on the host (sampler.py:49); here the full-row ranking runs on
    the GPU (`oibl_row_argsort`, stable: ties go to the lowest gallery index).  The tuple bookkeeping
    below is host logic restated with numpy; it draws from `random` exactly like the reference
    (one `random.sample(range(#candidates), min(neg_pool, #candidates))` per anchor), so a seeded
    run yields the same tuples (tests/golden/tuple_sampler.npz).

    `sort_gallery_on_device` / `load_mined` (an extension; openibl_amd/mining.py) handle only the anchors
    this replica visits in the round: the membership tests run on the GPU too (`oibl_mine_rows`) and
    `__iter__` makes the same draw over the mined rows — the same tuples from the same `random` state."""

    def __init__(self, query_source, gallery_source, pos_list, neg_list, neg_num=10, neg_pool=1000,
                 sub_length=None, num_replicas=None, rank=None):
        self.num_replicas = dist.get_world_size() if num_replicas is None else num_replicas
        self.rank = dist.get_rank() if rank is None else rank
        self.epoch = 0
        self.query_source, self.gallery_source = query_source, gallery_source
        self.pos_list, self.neg_list = pos_list, neg_list
        self.neg_num, self.neg_pool = neg_num, neg_pool
        self.sort_idx = None
        self._drop_mined()
        self.neg_cache = [[] for _ in range(len(query_source))]
        self._set_subset(list(range(len(query_source))))
        if sub_length is not None:
            self.sub_length = sub_length      # (the reference leaves the derived sizes to sort_gallery)

    def _set_subset(self, sub_set):
        self.sub_set = list(sub_set)
        self.sub_length = len(self.sub_set)
        self.sub_length_dist = -(-self.sub_length // self.num_replicas)
        self.total_size = self.sub_length_dist * self.num_replicas

    def sort_gallery(self, distmat, sub_set):
        """Rank the whole gallery for every query (ascending distance) and select this epoch's anchors."""
        assert distmat.shape[0] == len(self.query_source) and distmat.shape[1] == len(self.gallery_source)
        import torch
        from openibl_amd import ops
        d = torch.as_tensor(distmat, dtype=torch.float32)
        if not d.is_cuda:
            d = d.to(torch.device("cuda", torch.cuda.current_device()))
        self.sort_idx = ops.row_argsort(d.contiguous()).cpu().long()
        self._drop_mined()
        self._set_subset(sub_set)

    # -- mining on the device: only the rows this replica visits, no ranking on the host -------------
    def _drop_mined(self):
        self._mined = self._mined_row = self._mined_cpos = None

    def mining_anchors(self, sub_set):
        """The anchors this replica's slots visit when `sub_set` is the epoch's subset: first visit
        first, every anchor once (what `_my_slots` walks after `_set_subset(sub_set)`)."""
        sub_set = list(sub_set)
        total = -(-len(sub_set) // self.num_replicas) * self.num_replicas
        slots = list(range(len(sub_set)))
        slots += slots[: total - len(slots)]
        return list(dict.fromkeys(sub_set[s] for s in slots[self.rank: total: self.num_replicas]))

    def load_mined(self, mined, sub_set):
        """Take the rows `openibl_amd.mining` mined for this replica's anchors (MinedRows: candidates in
        rank order, the places of last round's negatives among them, the ranked positives) in place
        of a ranking, and select this epoch's anchors.  `__iter__` then yields the tuples it yields from
        `sort_gallery` on the same distances and the same `random` state."""
        row = {int(a): i for i, a in enumerate(mined.anchors)}
        missing = [a for a in self.mining_anchors(sub_set) if a not in row]
        if missing:
            raise KeyError("load_mined: no mined row for anchor(s) {}".format(missing[:8]))
        self._set_subset(sub_set)
        self.sort_idx = None
        self._mined, self._mined_row = mined, row
        self._mined_cpos = [[int(p) for p in r if p >= 0] for r in mined.cache_pos]

    def _anchor_rows(self, mat, anchors):
        """Rows `anchors` of a [Q][G] host or device matrix -> float32 on the current device."""
        import torch
        assert mat.shape[0] == len(self.query_source) and mat.shape[1] == len(self.gallery_source)
        dev = torch.device("cuda", torch.cuda.current_device())
        m = torch.as_tensor(mat)
        rows = m[torch.as_tensor(anchors, dtype=torch.long, device=m.device)]
        return rows.to(dev).float().contiguous()

    def sort_gallery_on_device(self, distmat, sub_set):
        """`sort_gallery` for the anchors of this epoch only: the rows this replica's slots visit are
        gathered from `distmat` ([Q][G], host or device), ranked and mined on the GPU
        (oibl_mine_rows) and loaded; no [Q][G] ranking exists on the host."""
        from openibl_amd import mining
        anchors = self.mining_anchors(sub_set)
        self.load_mined(mining.mine(self._anchor_rows(distmat, anchors), anchors, self), sub_set)

    def __len__(self):
        return self.sub_length_dist

    def set_epoch(self, epoch):
        self.epoch = epoch

    def _my_slots(self):
        slots = list(range(self.sub_length))
        slots += slots[: self.total_size - len(slots)]        # wrap-around padding
        return slots[self.rank: self.total_size: self.num_replicas]

    def _iter_mined(self):
        """`__iter__` over mined rows: the same draw, lookups instead of membership tests."""
        import heapq
        import random
        offset = len(self.query_source)
        m = self._mined
        for slot in self._my_slots():
            anchor = self.sub_set[slot]
            row = self._mined_row[anchor]
            positive = int(m.pos_ranked[row][0])
            if positive < 0:
                raise IndexError("anchor {} has no positive in the gallery".format(anchor))
            cand, n = m.cand[row], int(m.cand_len[row])
            pool = set(random.sample(range(n), min(self.neg_pool, n)))
            pool.update(self._mined_cpos[row])
            at = heapq.nsmallest(self.neg_num, pool)
            picked = [int(cand[i]) for i in at]
            assert len(picked) == self.neg_num
            # (the places go with the cache: an anchor that occurs twice in sub_set finds them here)
            self.neg_cache[anchor], self._mined_cpos[row] = picked, at
            yield [anchor, positive + offset] + [g + offset for g in picked]

    def __iter__(self):
        if self._mined is not None:
            yield from self._iter_mined()
            return
        import random
        import numpy as np
        offset = len(self.query_source)
        for slot in self._my_slots():
            anchor = self.sub_set[slot]
            ranked = np.asarray(self.sort_idx[anchor])
            # easiest positive: the best-ranked gallery entry among the anchor's positives
            positive = int(ranked[np.isin(ranked, self.pos_list[anchor])][0])
            # hardest negatives: best-ranked entries outside the anchor's exclusion zone, restricted
            # to a random pool plus the negatives used last time
            cand = ranked[~np.isin(ranked, self.neg_list[anchor])]
            pool = set(random.sample(range(len(cand)), min(self.neg_pool, len(cand))))
            if self.neg_cache[anchor]:
                where = {int(g): i for i, g in enumerate(cand.tolist())}
                pool |= {where[g] for g in self.neg_cache[anchor]}
            picked = [int(cand[i]) for i in sorted(pool)[: self.neg_num]]
            assert len(picked) == self.neg_num
            self.neg_cache[anchor] = picked
            yield [anchor, positive + offset] + [g + offset for g in picked]


class DistributedRandomDiffTupleSampler(DistributedRandomTupleSampler):
    """The SFRS mining sampler (ibl/utils/data/sampler.py:92-190 of the reference;
    examples/netvlad_img_sfrs.py): tuples `[anchor, easiest positive, neg_num hardest negatives,
    up to pos_num "difficult" positives]`.  As above, what runs on the GPU is the full-row ranking of
    `sort_gallery` (sampler.py:130: `torch.argsort(distmat, dim=1)`); the k-reciprocal matrix
    `distmat_jac` is only indexed.

    Difficult positives (sampler.py:158-178): of the anchor's best-ranked `pos_pool` positives, those
    that the Jaccard distance ranks HIGHER than the descriptor distance does, largest promotion first,
    then the ones both rankings agree on.  The two small sorts are `torch.argsort` calls on the same
    values as in the reference (its tie behaviour on equal promotions is torch's, so torch is asked);
    a seeded run yields the same tuples (tests/golden/diff_tuple_sampler.npz)."""

    def __init__(self, query_source, gallery_source, pos_list, neg_list, pos_num=10, pos_pool=20,
                 neg_num=10, neg_pool=1000, sub_length=None, num_replicas=None, rank=None):
        super().__init__(query_source, gallery_source, pos_list, neg_list, neg_num=neg_num, neg_pool=neg_pool,
                         sub_length=sub_length, num_replicas=num_replicas, rank=rank)
        self.pos_num, self.pos_pool = pos_num, pos_pool
        self.distmat_jac = None

    def sort_gallery(self, distmat, distmat_jac, sub_set):
        super().sort_gallery(distmat, sub_set)
        self.distmat_jac = distmat_jac

    def _difficult_positives(self, anchor, ranked_pos):
        import torch
        pool = torch.as_tensor(ranked_pos[: self.pos_pool], dtype=torch.long)
        jac = torch.as_tensor(self.distmat_jac[anchor])[pool]
        return self._promoted(pool, jac)

    def _promoted(self, pool, jac):
        import torch
        by_jac = torch.argsort(jac, dim=0)                  # by_jac[i]: descriptor rank of the i-th by Jaccard
        gap = torch.arange(by_jac.size(0)) - by_jac         # < 0: promoted by the Jaccard distance
        slots = torch.arange(by_jac.size(0))
        promoted = slots[gap < 0][torch.argsort(gap[gap < 0], dim=0)]
        chosen = torch.cat((promoted, slots[gap == 0]), dim=0)[: self.pos_num]
        return pool[by_jac[chosen]].tolist()

    def sort_gallery_on_device(self, distmat, distmat_jac, sub_set):
        """`sort_gallery` for the anchors of this epoch only (see the tuple sampler).  A float32 device
        `distmat_jac` is gathered by the mining kernel; of any other matrix the few entries the difficult
        positives need are read where it lies, in its own type."""
        import numpy as np
        import torch
        from openibl_amd import mining
        anchors = self.mining_anchors(sub_set)
        rows = self._anchor_rows(distmat, anchors)
        on_device = torch.is_tensor(distmat_jac) and distmat_jac.is_cuda and distmat_jac.dtype == torch.float32
        if distmat_jac is distmat:
            mined = mining.mine(rows, anchors, self, jac_rows=rows)
        elif on_device:
            mined = mining.mine(rows, anchors, self, jac_rows=self._anchor_rows(distmat_jac, anchors))
        else:
            assert distmat_jac.shape[0] == len(self.query_source) and distmat_jac.shape[1] == len(self.gallery_source)
            mined = mining.mine(rows, anchors, self)
            jac = torch.as_tensor(distmat_jac).cpu().numpy()
            at = np.maximum(mined.pos_ranked, 0)
            mined.pos_jac = np.where(mined.pos_ranked >= 0, jac[np.asarray(anchors)[:, None], at], np.nan)
        self.load_mined(mined, sub_set)
        self.distmat_jac = None

    def __iter__(self):
        import numpy as np
        offset = len(self.query_source)
        base = super().__iter__()
        if self._mined is not None:
            import torch
            m = self._mined
            for slot in self._my_slots():
                row = self._mined_row[self.sub_set[slot]]
                n = int((m.pos_ranked[row] >= 0).sum())
                extra = self._promoted(torch.as_tensor(m.pos_ranked[row][:n], dtype=torch.long),
                                       torch.as_tensor(m.pos_jac[row][:n]))
                yield next(base) + [p + offset for p in extra]
            return
        for slot in self._my_slots():
            anchor = self.sub_set[slot]
            ranked = np.asarray(self.sort_idx[anchor])
            ranked_pos = ranked[np.isin(ranked, self.pos_list[anchor])].tolist()
            extra = self._difficult_positives(anchor, ranked_pos)   # (no RNG: before or after `base` alike)
            yield next(base) + [p + offset for p in extra]
