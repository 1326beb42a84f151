"""Mining on the device (GPU): oibl_mine_rows against its numpy mirror at the edges of the pass, the samplers'
`sort_gallery_on_device` against the reference's tuples, and the flows from descriptors and from a model against
the host flow they replace.  Every integer output is compared for equality."""
import random

import numpy as np
import pytest
import torch

from helpers import mining_ref
from openibl_amd import mining, ops, synth
from ibl.utils.data.sampler import DistributedRandomDiffTupleSampler, DistributedRandomTupleSampler

pytestmark = pytest.mark.gpu

LDS_EXCL = 4096      # exclusion entries per anchor the kernel stages in LDS (csrc/mining.hip: MINE_LDS_EXCL)
CHUNK = 256          # ranks per step of the pass (MINE_THREADS)


def _run(dev, dist, pos, excl, cache=None, pos_pool=1, jac=None, csr_row=None, **kw):
    """ops.mine_rows on host inputs -> dict of numpy arrays (the mirror's keys)."""
    G = dist.shape[1]
    lists = [torch.from_numpy(p).to(dev) for p in mining.csr_lists(pos, G) + mining.csr_lists(excl, G)]
    out = ops.mine_rows(dist.to(dev) if not dist.is_cuda else dist, *lists,
                        cache=None if cache is None else torch.from_numpy(np.asarray(cache, dtype=np.int32)).to(dev),
                        pos_pool=pos_pool, jac=None if jac is None else (jac if jac.is_cuda else jac.to(dev)),
                        csr_row=None if csr_row is None else torch.as_tensor(csr_row, dtype=torch.int32, device=dev),
                        **kw)
    keys = ("cand", "cand_len", "cache_pos", "pos_ranked", "pos_jac")
    return {k: None if t is None else t.cpu().numpy() for k, t in zip(keys, out)}


def _same(got, want):
    for k in ("cand", "cand_len", "cache_pos", "pos_ranked"):
        assert got[k].dtype == np.int32
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got["pos_jac"] is None) == (want["pos_jac"] is None)
    if want["pos_jac"] is not None:      # copied floats: the same bits, NaN behind the last positive
        assert np.array_equal(np.isnan(got["pos_jac"]), np.isnan(want["pos_jac"]))
        np.testing.assert_array_equal(np.nan_to_num(got["pos_jac"]).view(np.int32),
                                      np.nan_to_num(want["pos_jac"]).view(np.int32))


def _random_problem(rng, A, G, ties):
    if ties:
        d = rng.integers(0, 5, size=(A, G)).astype(np.float32) * 0.25
    else:
        d = rng.standard_normal((A, G)).astype(np.float32)
    jac = rng.uniform(0, 1, size=(A, G)).astype(np.float32)
    pos = [rng.choice(G, size=min(G, 7), replace=False) for _ in range(A)]
    excl = [np.union1d(p[:3], rng.choice(G, size=min(G, max(1, G // 5)), replace=False)) for p in pos]
    kept = [np.setdiff1d(np.arange(G), e) for e in excl]
    # a cache with an absent entry, an excluded index, and whatever candidates there are
    cache = np.full((A, 5), -1, dtype=np.int32)
    for a in range(A):
        cache[a, 1] = excl[a][0]
        some = rng.choice(kept[a], size=min(3, len(kept[a])), replace=False) if len(kept[a]) else []
        cache[a, 2:2 + len(some)] = some
    return torch.from_numpy(d), torch.from_numpy(jac), pos, excl, cache


@pytest.mark.parametrize("G", [1, 63, 64, 65, 255, 256, 257, 2500, 4097])
def test_mine_rows_at_row_lengths_around_the_chunk(dev, G):
    """Rows shorter than a wave, a chunk, one past, many chunks; A = 1 and 3; with and without ties, a row
    stride beyond G, jac absent and present; cache entries absent (-1), excluded and kept."""
    rng = np.random.default_rng([G, 3])
    for A, ties, wide, with_jac in ((1, False, False, True), (3, True, True, False), (3, False, True, True)):
        d, jac, pos, excl, cache = _random_problem(rng, A, G, ties)
        dd = d.to(dev)
        if wide:                      # ld > G: a view of a wider matrix, the columns beyond hold smaller values
            full = torch.full((A, G + 37), -9.0, device=dev)
            full[:, :G] = dd
            dd = full[:, :G]
            assert dd.stride(0) == G + 37
        got = _run(dev, dd, pos, excl, cache, pos_pool=4 if A == 1 else 9, jac=jac if with_jac else None)
        want = mining_ref.mine_rows(d.numpy(), pos, excl, cache, 4 if A == 1 else 9, jac.numpy() if with_jac else None)
        _same(got, want)
        assert (got["cache_pos"][:, 0] == -1).all() and (got["cache_pos"][:, 1] == -1).all()


def test_mine_rows_in_groups_under_a_workspace_bound(dev):
    """7 rows under a bound that holds 2: four groups, with one CSR row per anchor and with csr_row."""
    rng = np.random.default_rng(11)
    A, G = 7, 300
    d, jac, pos, excl, cache = _random_problem(rng, A, G, ties=True)
    want = mining_ref.mine_rows(d.numpy(), pos, excl, cache, 6, jac.numpy())
    bound = 2 * (20 * G + 2048)
    assert ops._lib.load().oibl_mine_rows_workspace_bytes(2, G) <= bound < 3 * 20 * G
    _same(_run(dev, d, pos, excl, cache, pos_pool=6, jac=jac, max_ws_bytes=bound), want)
    # the lists of 12 "queries", the anchors' rows among them in any order, one twice
    rows = [9, 2, 11, 2, 0, 5, 7]
    many_pos, many_excl = [[0]] * 12, [[1]] * 12
    for a, r in enumerate(rows):
        many_pos[r], many_excl[r] = pos[a], excl[a]
    pos2, excl2 = [many_pos[r] for r in rows], [many_excl[r] for r in rows]
    want2 = mining_ref.mine_rows(d.numpy(), pos2, excl2, cache, 6, jac.numpy())
    _same(_run(dev, d, many_pos, many_excl, cache, pos_pool=6, jac=jac, csr_row=rows, max_ws_bytes=bound), want2)
    _same(_run(dev, d, many_pos, many_excl, cache, pos_pool=6, jac=jac, csr_row=rows), want2)


def test_mine_rows_tie_rule_and_chunk_borders(dev):
    G = 3 * CHUNK + 40
    # all-equal rows: rank order is the gallery index
    d = torch.zeros((2, G))
    d[1] = 2.5
    pos = [[5, 700, 3], [G - 1]]
    excl = [[0, 1, 400], []]
    got = _run(dev, d, pos, excl, [[2, 400, -1], [G - 1, 0, 7]], pos_pool=4)
    _same(got, mining_ref.mine_rows(d.numpy(), pos, excl, np.array([[2, 400, -1], [G - 1, 0, 7]]), 4))
    assert got["pos_ranked"].tolist() == [[3, 5, 700, -1], [G - 1, -1, -1, -1]]
    assert got["cache_pos"].tolist() == [[0, -1, -1], [G - 1, 0, 7]] and got["cand_len"].tolist() == [G - 3, G]
    # duplicated values straddling excluded and kept entries: equal distances keep the index order among
    # the kept ones whatever lies between them
    d = torch.from_numpy(np.repeat(np.arange(G // 4 + 1), 4)[:G].astype(np.float32))[None].flip(1).contiguous()
    excl = [list(range(1, G, 2))]
    got = _run(dev, d, [[8, 9, 10, 11]], excl, [[10, 9, 8]], pos_pool=8)
    _same(got, mining_ref.mine_rows(d.numpy(), [[8, 9, 10, 11]], excl, np.array([[10, 9, 8]]), 8))
    # rank = index; excluded entries at the first and the last place of a chunk (and of the row)
    d = torch.arange(G, dtype=torch.float32)[None].contiguous()
    excl = [[0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, 3 * CHUNK - 1, 3 * CHUNK, G - 1]]
    cache = [[1, CHUNK - 2, CHUNK + 1, 3 * CHUNK + 1, G - 2, CHUNK]]
    got = _run(dev, d, [[CHUNK - 1, CHUNK, 0]], excl, cache, pos_pool=3)
    _same(got, mining_ref.mine_rows(d.numpy(), [[CHUNK - 1, CHUNK, 0]], excl, np.array(cache), 3))
    assert got["cache_pos"].tolist() == [[0, CHUNK - 3, CHUNK - 2, 3 * CHUNK - 6, G - 9, -1]]
    assert got["pos_ranked"].tolist() == [[0, CHUNK - 1, CHUNK]]      # positives are ranked, excluded or not


def test_mine_rows_long_exclusion_lists(dev):
    """Exclusion lists at and beyond the LDS staging limit (4096 entries): the rows of one launch take the
    LDS search and the global-memory search side by side."""
    rng = np.random.default_rng(13)
    G = 6000
    d = torch.from_numpy(rng.standard_normal((4, G)).astype(np.float32))
    excl = [rng.choice(G, size=n, replace=False) for n in (LDS_EXCL, LDS_EXCL + 1, 5500, 17)]
    pos = [rng.choice(G, size=12, replace=False) for _ in range(4)]
    cache = np.stack([np.concatenate([e[:2], np.setdiff1d(np.arange(G), e)[-3:]]) for e in excl]).astype(np.int32)
    got = _run(dev, d, pos, excl, cache, pos_pool=20, jac=d)
    _same(got, mining_ref.mine_rows(d.numpy(), pos, excl, cache, 20, d.numpy()))
    assert got["cand_len"].tolist() == [G - LDS_EXCL, G - LDS_EXCL - 1, 500, G - 17]


def test_exactly_neg_num_candidates_and_untidy_lists_through_the_python_layer(dev):
    """An exclusion zone that leaves exactly neg_num candidates still yields tuples; one entry more raises the
    AssertionError of the ranking path.  The sampler's lists come unsorted, with repeats and foreign indices."""
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(17)
    Q, G, neg_num = 4, 300, 10
    d = torch.from_numpy(rng.standard_normal((Q, G)).astype(np.float32))
    keep = [rng.choice(G, size=neg_num, replace=False) for _ in range(Q)]
    neg = [np.setdiff1d(np.arange(G), k)[::-1].tolist() + [G + 3, -1, 0, 0] for k in keep]
    neg = [[v for v in n if v not in set(k.tolist())] for n, k in zip(neg, keep)]
    pos = [[int(n[7]), int(n[3]), int(n[7]), G + 9, int(n[5])] for n in neg]
    smp = DistributedRandomTupleSampler(list(range(Q)), list(range(G)), pos, neg, neg_num=neg_num, neg_pool=40,
                                        num_replicas=1, rank=0)
    mined = mining.mine(d.to(dev), list(range(Q)), smp)
    want = mining_ref.mine_for_sampler(smp, d.numpy(), list(range(Q)))
    for k in ("cand", "cand_len", "cache_pos", "pos_ranked"):
        np.testing.assert_array_equal(getattr(mined, k), getattr(want, k), err_msg=k)
    assert mined.cand_len.tolist() == [neg_num] * Q and mined.pos_jac is None
    smp.load_mined(mined, list(range(Q)))
    tuples = list(iter(smp))
    for q, t in enumerate(tuples):
        assert sorted(g - Q for g in t[2:]) == sorted(keep[q].tolist())
    tight = DistributedRandomTupleSampler(list(range(Q)), list(range(G)), pos, [n + [int(keep[0][0])] for n in neg],
                                          neg_num=neg_num, neg_pool=40, num_replicas=1, rank=0)
    tight.sort_gallery_on_device(d, list(range(Q)))
    with pytest.raises(AssertionError):
        list(iter(tight))


def test_two_runs_give_identical_bytes(dev):
    rng = np.random.default_rng(19)
    d, jac, pos, excl, cache = _random_problem(rng, 5, 2500, ties=True)
    runs = [_run(dev, d, pos, excl, cache, pos_pool=7, jac=jac) for _ in range(2)]
    for k, v in runs[0].items():
        assert v.tobytes() == runs[1][k].tobytes(), k


def test_sort_gallery_on_device_yields_the_reference_tuples(dev):
    """Both goldens (the reference's own tuples: two replicas, two epochs, the second on the cache positions),
    the matrices once on the host and once on the device."""
    from test_host_logic import _run_diff_tuple_sampler, _run_tuple_sampler
    torch.cuda.set_device(dev)
    _run_tuple_sampler(lambda smp, d, sub: smp.sort_gallery_on_device(d, sub))
    _run_tuple_sampler(lambda smp, d, sub: smp.sort_gallery_on_device(d.to(dev), sub))
    _run_diff_tuple_sampler(lambda smp, d, jac, sub: smp.sort_gallery_on_device(d, jac, sub))
    _run_diff_tuple_sampler(lambda smp, d, jac, sub: smp.sort_gallery_on_device(d.to(dev), jac.to(dev), sub))
    _run_diff_tuple_sampler(lambda smp, d, jac, sub: smp.sort_gallery_on_device(d.numpy(), jac.double().numpy(), sub))

    def back_and_forth(smp, d, sub):          # sort_gallery drops the mined state, and the other way round
        smp.sort_gallery_on_device(d, sub)
        smp.sort_gallery(d, sub)
        assert smp._mined is None and smp.sort_idx is not None
    _run_tuple_sampler(back_and_forth)


def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True))


@pytest.mark.parametrize("Q,G,n_anchors", [(12, 300, 12), (64, 5000, 16)])
def test_mine_from_features_yields_the_host_paths_tuples(dev, Q, G, n_anchors):
    """From descriptors, two rounds, both samplers, rerank off and on: the tuples of `sort_gallery` fed a matrix
    whose anchor rows come from the same pairwise_sqdist call on the same rows (every other row +inf: a row of
    a sub-matrix is not assumed to equal the row of the full matrix)."""
    from openibl_amd.rerank import re_ranking_features
    torch.cuda.set_device(dev)
    rng = np.random.default_rng([Q, G])
    q, g = _unit_rows(rng, Q, 128).to(dev), _unit_rows(rng, G, 128).to(dev)
    pos, neg = synth.tuple_lists(Q, G, seed=23, positives=8)
    jac_full = re_ranking_features(q, g, k1=20, k2=1, lambda_value=0.1, precision="fp32").cpu()
    for diff in (False, True):
        for rerank in ((False, True) if diff else (False,)):
            def make():
                if diff:
                    return DistributedRandomDiffTupleSampler(list(range(Q)), list(range(G)), pos, neg, pos_num=4,
                                                             pos_pool=6, neg_num=5, neg_pool=40, num_replicas=2, rank=1)
                return DistributedRandomTupleSampler(list(range(Q)), list(range(G)), pos, neg, neg_num=5, neg_pool=40,
                                                     num_replicas=2, rank=1)
            old, new = make(), make()
            for rnd in range(2):
                sub = random.Random(rnd).sample(range(Q), n_anchors) + ([3] if rnd else [])
                anchors = new.mining_anchors(sub)
                at = torch.as_tensor(anchors, device=dev)
                full = torch.full((Q, G), float("inf"))
                full[anchors] = ops.pairwise_sqdist(q[at].float().contiguous(), g.float().contiguous(), "fp32").cpu()
                if diff:
                    old.sort_gallery(full, jac_full if rerank else full, sub)
                else:
                    old.sort_gallery(full, sub)
                random.seed(900 + rnd)
                want = list(iter(old))
                after = random.getstate()
                new.load_mined(mining.mine_from_features(q, g, sub, new, rerank=rerank, precision="fp32"), sub)
                random.seed(900 + rnd)
                assert list(iter(new)) == want and random.getstate() == after
                assert new.neg_cache == old.neg_cache


class _Slice(torch.utils.data.Sampler):
    def __init__(self, n):
        self.n = n

    def __iter__(self):
        return iter(range(self.n))

    def __len__(self):
        return self.n


def test_update_sampler_against_the_host_flow(dev, state_dict, tmp_path, monkeypatch):
    """mining.update_sampler on the synthetic dataset with the synthetic-weight model, against the training
    scripts' flow (extract_features + pairwise_distance + sort_gallery), fp32, both samplers, two rounds."""
    import hubconf
    from ibl.datasets.synthetic import Synthetic
    from ibl.evaluators import extract_features, pairwise_distance
    from ibl.utils.data import get_transformer_test
    from ibl.utils.data.preprocessor import Preprocessor
    monkeypatch.setenv("OPENIBL_AMD_PRECISION", "fp32")
    torch.cuda.set_device(dev)
    ds = Synthetic(str(tmp_path / "syn"), verbose=False, num_query=6, num_gallery=16, height=64, width=96)
    query, gallery = ds.q_train, ds.db_train
    Q, G = len(query), len(gallery)
    records = sorted(list(set(query) | set(gallery)))
    loader = torch.utils.data.DataLoader(Preprocessor(records, root=ds.images_dir,
                                                      transform=get_transformer_test(64, 96)),
                                         batch_size=4, num_workers=0, shuffle=False, sampler=_Slice(len(records)))
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    model = model.to(dev).eval()
    pos = [[i % G] for i in range(Q)]
    neg = [[(i + k) % G for k in (-1, 0, 1)] for i in range(Q)]
    sub = list(range(Q))
    for diff in (False, True):
        def make():
            if diff:
                return DistributedRandomDiffTupleSampler(query, gallery, pos, neg, pos_num=1, pos_pool=2, neg_num=3,
                                                         neg_pool=6, num_replicas=1, rank=0)
            return DistributedRandomTupleSampler(query, gallery, pos, neg, neg_num=3, neg_pool=6, num_replicas=1,
                                                 rank=0)
        old, new = make(), make()
        for rnd in range(2):
            features = extract_features(model, loader, records, vlad=True, gpu=dev.index)
            distmat, _, _ = pairwise_distance(features, query, gallery)
            if diff:
                old.sort_gallery(distmat, distmat, sub)
            else:
                old.sort_gallery(distmat, sub)
            random.seed(40 + rnd)
            want = list(iter(old))
            mining.update_sampler(new, model, loader, query, gallery, sub, vlad=True, gpu=dev.index)
            random.seed(40 + rnd)
            assert list(iter(new)) == want
            assert len(want) == Q and all(len(t) == (6 if diff else 5) for t in want)
