"""Mining on the device, the parts that need no GPU: the samplers' `load_mined` / mined `__iter__` fed by the
numpy mirror of the kernel's contract (tests/helpers/mining_ref.py), the argument validation of the C entry
and its place in the ABI."""
import ctypes
import random

import numpy as np
import pytest
import torch

from helpers import mining_ref
from ibl.utils.data.sampler import DistributedRandomDiffTupleSampler, DistributedRandomTupleSampler
from test_host_logic import _run_diff_tuple_sampler, _run_tuple_sampler


def _load_from_mirror(smp, d, sub, jac=None):
    anchors = smp.mining_anchors(sub)
    smp.load_mined(mining_ref.mine_for_sampler(smp, d.numpy(), anchors, None if jac is None else jac.numpy()), sub)


def test_load_mined_yields_the_reference_tuples():
    """load_mined on the mirror's rows reproduces the reference's own tuples (two replicas, two epochs: the
    second draws on the cache positions)."""
    _run_tuple_sampler(lambda smp, d, sub: _load_from_mirror(smp, d, sub))


def test_load_mined_yields_the_reference_diff_tuples():
    _run_diff_tuple_sampler(lambda smp, d, jac, sub: _load_from_mirror(smp, d, sub, jac))


def _case(name):
    """(Q, G, dist, jac, pos, neg, sub_set, sampler keywords) of a seeded random case."""
    rng = np.random.default_rng([77, sum(map(ord, name))])
    Q, G = 9, 120
    kw = dict(neg_num=4, neg_pool=30)
    d = rng.standard_normal((Q, G)).astype(np.float32)
    jac = rng.uniform(0, 1, size=(Q, G)).astype(np.float32)
    pos = [sorted(rng.choice(G, size=8, replace=False).tolist()) for _ in range(Q)]
    neg = [sorted(set(p) | set(rng.choice(G, size=30, replace=False).tolist())) for p in pos]
    sub = list(range(Q))
    if name == "ties":                       # few distinct values: the tie rule decides most places
        d = rng.integers(0, 4, size=(Q, G)).astype(np.float32)
        jac = rng.integers(0, 3, size=(Q, G)).astype(np.float32)
    elif name == "empty_exclusion":
        neg = [[] if q % 2 else n for q, n in enumerate(neg)]
    elif name == "few_positives":            # fewer than pos_pool = 6, one anchor with a single one
        pos = [p[: 1 + q % 3] for q, p in enumerate(pos)]
    elif name == "anchor_twice":
        sub = [3, 5, 3, 1, 5, 3, 0]
    elif name == "pool_covers_all":          # neg_pool >= cand_len: every candidate is drawn
        kw = dict(neg_num=4, neg_pool=G)
    elif name == "unsorted_lists":           # repeats, any order, indices outside the gallery
        pos = [list(reversed(p)) + p[:2] + [G + 5, -3] for p in pos]
        neg = [list(reversed(n)) + n[:3] + [G, 10 * G] for n in neg]
    return Q, G, torch.from_numpy(d), torch.from_numpy(jac), pos, neg, sub, kw


CASES = ["plain", "ties", "empty_exclusion", "few_positives", "anchor_twice", "pool_covers_all", "unsorted_lists"]


@pytest.mark.parametrize("diff", [False, True], ids=["tuple", "diff"])
@pytest.mark.parametrize("name", CASES)
def test_mined_iter_equals_the_ranking_iter(name, diff):
    """Same tuples and the same `random` state afterwards, over three rounds (cache filled from the second),
    on both replicas."""
    Q, G, d, jac, pos, neg, sub, kw = _case(name)
    stable = torch.from_numpy(np.argsort(d.numpy(), axis=1, kind="stable"))
    for rank in range(2):
        def make():
            if diff:
                return DistributedRandomDiffTupleSampler(list(range(Q)), list(range(G)), pos, neg, pos_num=4,
                                                         pos_pool=6, num_replicas=2, rank=rank, **kw)
            return DistributedRandomTupleSampler(list(range(Q)), list(range(G)), pos, neg, num_replicas=2,
                                                 rank=rank, **kw)
        old, new = make(), make()
        state = None
        for rnd in range(3):
            sub_r = sub if rnd != 1 else sub[1:]
            old.sort_idx, old.distmat_jac = stable, jac
            old._set_subset(sub_r)
            random.seed(500 + rnd) if state is None else random.setstate(state)
            start = random.getstate()
            want = list(iter(old))
            after_old = random.getstate()
            random.setstate(start)
            _load_from_mirror(new, d, sub_r, jac if diff else None)
            got = list(iter(new))
            assert got == want
            assert random.getstate() == after_old
            assert new.neg_cache == old.neg_cache and len(new) == len(old)
            state = after_old


def test_sort_gallery_state_and_failure_modes():
    Q, G, d, jac, pos, neg, sub, kw = _case("plain")
    smp = DistributedRandomTupleSampler(list(range(Q)), list(range(G)), pos, neg, num_replicas=1, rank=0, **kw)
    assert smp._mined is None
    _load_from_mirror(smp, d, sub)
    assert smp._mined is not None and smp.sort_idx is None and len(smp) == Q
    with pytest.raises(KeyError):            # rows mined for another subset
        smp.load_mined(mining_ref.mine_for_sampler(smp, d.numpy(), [0, 1]), [0, 1, 2])
    # a missing positive: IndexError, like the [0] of the ranking path
    nopos = DistributedRandomTupleSampler(list(range(Q)), list(range(G)), [[] for _ in pos], neg, num_replicas=1,
                                          rank=0, **kw)
    _load_from_mirror(nopos, d, sub)
    with pytest.raises(IndexError):
        list(iter(nopos))
    # fewer than neg_num candidates: the AssertionError stays
    few = DistributedRandomTupleSampler(list(range(Q)), list(range(G)), pos, [list(range(3, G)) for _ in neg],
                                        num_replicas=1, rank=0, **kw)
    _load_from_mirror(few, d, sub)
    with pytest.raises(AssertionError):
        list(iter(few))


def test_csr_lists_follow_isin():
    from openibl_amd.mining import csr_lists
    off, val = csr_lists([[5, 1, 5, 99, -2], [], [0, 9]], 10)
    assert off.tolist() == [0, 2, 2, 4] and val.tolist() == [1, 5, 0, 9]
    assert off.dtype == np.int32 and val.dtype == np.int32


def test_cpu_tensors_are_refused():
    from openibl_amd import lib, mining, ops
    z = torch.zeros((2, 4))
    i = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(lib.OpenIBLAmdError):
        ops.mine_rows(z, i, i, i, i)
    smp = DistributedRandomTupleSampler([0, 1], [0, 1, 2, 3], [[0], [1]], [[0], [1]], neg_num=1, num_replicas=1,
                                        rank=0)
    with pytest.raises(lib.OpenIBLAmdError):
        mining.mine(z, [0, 1], smp)
    with pytest.raises(lib.OpenIBLAmdError):
        mining.mine_from_features(z, torch.zeros((4, 4)), [0, 1], smp)


def test_update_sampler_refuses_several_ranks(monkeypatch):
    """World size above 1: RuntimeError that names the host flow, before anything is extracted."""
    from openibl_amd import evaluators, mining
    monkeypatch.setattr(evaluators, "_rank_world", lambda: (1, 2))
    with pytest.raises(RuntimeError, match="sort_gallery"):
        mining.update_sampler(None, None, None, [], [], [])


def test_mine_rows_argument_validation():
    """Every bad argument returns OIBL_E_INVALID (-1) with its message before any HIP call (there is no
    device here to call)."""
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf) // 256 * 256 + 256          # some non-null, 256-byte aligned address
    good = dict(dist=p, A=2, G=8, ld=8, csr_row=None, pos_off=p, pos_val=p, excl_off=p, excl_val=p, cache=p, C=4,
                jac=None, jac_ld=0, pos_pool=2, cand=p, cand_ld=8, cand_len=p, cache_pos=p, pos_ranked=p,
                pos_jac=None, ws=p, ws_bytes=0, stream=None)

    def call(**change):
        return h.oibl_mine_rows(*{**good, **change}.values())

    for change, word in ((dict(dist=None), b"null"), (dict(pos_off=None), b"null"), (dict(excl_val=None), b"null"),
                         (dict(cand=None), b"null"), (dict(cand_len=None), b"null"), (dict(pos_ranked=None), b"null"),
                         (dict(ws=None), b"null"), (dict(A=0), b"bad shape"), (dict(G=0), b"bad shape"),
                         (dict(A=-1), b"bad shape"), (dict(ld=7), b"bad shape"), (dict(cand_ld=7), b"cand_ld"),
                         (dict(C=65), b"C=65"), (dict(C=-1), b"C=-1"), (dict(cache=None), b"cache"),
                         (dict(cache_pos=None), b"cache"), (dict(pos_pool=0), b"pos_pool"),
                         (dict(pos_pool=1025), b"pos_pool"), (dict(jac=p, jac_ld=8), b"jac"),
                         (dict(jac=p, pos_jac=p, jac_ld=7), b"jac"), (dict(ws=p + 4), b"aligned")):
        assert call(**change) == -1, change
        assert word in h.oibl_last_error(), (change, h.oibl_last_error())
    assert call() == -2 and b"workspace" in h.oibl_last_error()        # OIBL_E_WORKSPACE: still no HIP call
    assert h.oibl_mine_rows_workspace_bytes(0, 5) == 0 and h.oibl_mine_rows_workspace_bytes(5, 0) == 0
    # the ranking and the sort's four buffers, each rounded up to 256 bytes
    assert h.oibl_mine_rows_workspace_bytes(3, 1000) == 5 * 12032


def test_abi_stays_at_3_with_the_entries_added():
    import re
    from pathlib import Path
    from openibl_amd import lib
    assert lib.ABI_VERSION == 3 and lib.load().oibl_abi_version() == 3
    header = (Path(__file__).resolve().parent.parent / "include" / "openibl_amd.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ("oibl_mine_rows_workspace_bytes", "oibl_mine_rows"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in lib.SIGNATURES and hasattr(raw, name)
    decl = re.search(r"int oibl_mine_rows\((.*?)\);", code, flags=re.S).group(1)
    assert len(decl.split(",")) == len(lib.SIGNATURES["oibl_mine_rows"][1])
