"""k-reciprocal re-ranking on the device from descriptors (openibl_amd.rerank.re_ranking_features, csrc/rerank.hip)
against the host mirror of the reference (openibl_amd.rerank.re_ranking) and the reference's own outputs (GPU)."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from openibl_amd import ops, synth
from openibl_amd import rerank as rr
from oracle import matching as om

pytestmark = pytest.mark.gpu

PROBLEM = dict(views_per_place=4, hard_fraction=0.5, hard_noise_mult=35.0)


def _host_sets(rank, k1, half):
    """The member sets exactly as the host mirror builds them (rerank.py: _reciprocal + the expansion + unique)."""
    out = []
    for i in range(rank.shape[0]):
        base = rr._reciprocal(rank, i, k1)
        members = [base]
        for cand in base:
            sub = rr._reciprocal(rank, int(cand), half)
            if len(np.intersect1d(sub, base)) > 2.0 / 3.0 * len(sub):
                members.append(sub)
        out.append(np.unique(np.concatenate(members)))
    return out


def _sparse(V, stride):
    """Dense [n][n] -> (idx [n][stride] int32 ascending, val, cnt)."""
    n = V.shape[0]
    idx = np.zeros((n, stride), np.int32)
    val = np.zeros((n, stride), np.float32)
    cnt = np.zeros(n, np.int32)
    for i in range(n):
        c = np.nonzero(V[i])[0]
        cnt[i] = len(c)
        idx[i, :len(c)] = c
        val[i, :len(c)] = V[i, c]
    return idx, val, cnt


def _small(duplicates=False):
    """The 24 x 90 problem at d = 256; `duplicates`: eight query rows are gallery rows and four gallery rows are
    repeated (an image in both sets: distance-0 ties, fp32 self-distances that can come out slightly negative)."""
    q, g, _, _ = synth.retrieval_problem(24, 90, dim=256, seed=31, **PROBLEM)
    if duplicates:
        q, g = q.clone(), g.clone()
        q[:8] = g[10:18]
        g[40:44] = g[50:54]
    return q, g


def _stages(q, g, settings, dev):
    """Every stage on its own, fed from the host, for each (k1, k2, lambda) of `settings` (the checks are described
    at test_stages_against_the_host_mirror).  The rank lists are the host's, in the form the device search hands
    them on: K = max(k1 + 1, round(k1 / 2) + 1, k2) columns, -1 beyond the n items there are."""
    x = torch.cat([q, g])
    d64 = om.pairwise_distance(x.double(), x.double()).numpy()
    d32 = d64.astype(np.float32)
    d32 = ((d32 + d32.T) / 2).astype(np.float32)              # exactly symmetric: O[i][j] is D[j][i]^2 / m_i on the host
    nq, n = q.shape[0], x.shape[0]
    for k1, k2, lam in settings:
        half = ops.rerank_half(k1)
        K = max(k1 + 1, half + 1, k2)
        rank = om.topk(d64, K)[1].astype(np.int32)            # min(K, n) columns: what the mirror's _nearest returns
        want_sets = _host_sets(rank, k1, half)
        padded = np.full((n, K), -1, np.int32)
        padded[:, :rank.shape[1]] = rank
        rank_d = torch.from_numpy(padded).to(dev)
        idx, cnt = ops.rerank_sets(rank_d, k1)
        idx_h, cnt_h = idx.cpu().numpy(), cnt.cpu().numpy()
        assert idx.shape[1] == (k1 + 1) * (half + 2)
        for i in range(n):
            assert cnt_h[i] == len(want_sets[i]) and np.array_equal(idx_h[i, :cnt_h[i]], want_sets[i]), (k1, i)
        # ---- weights: host V from the symmetric fp32 matrix, as the mirror computes it
        sq = np.power(d32, 2).astype(np.float32)
        colmax = sq.max(axis=0)
        O = np.ascontiguousarray((sq / colmax).T)
        V = np.zeros((n, n), np.float32)
        for i in range(n):
            w = np.exp(-O[i, want_sets[i]])
            V[i, want_sets[i]] = w / w.sum()
        xd = x.to(dev)
        norms, rowmax = ops.rerank_row_extremes(xd)
        np.testing.assert_allclose(norms.cpu().numpy(), (x.double() ** 2).sum(1).numpy(), rtol=1e-6)
        np.testing.assert_allclose(rowmax.cpu().numpy(), colmax, rtol=4e-6)
        val = ops.rerank_weights(xd, norms, rowmax, idx, cnt).cpu().numpy()
        werr = max(np.abs(val[i, :cnt_h[i]] - V[i, want_sets[i]]).max() for i in range(n))
        print(f"{nq} x {n - nq} k1={k1}: weights max|dev - host| = {werr:.2e}")
        assert werr <= 2e-6
        # ---- from here on the device is fed the HOST's V: the remaining stages are compared exactly
        stride = idx.shape[1]
        hi, hv, hc = _sparse(V, stride)
        di, dv, dc = (torch.from_numpy(a).to(dev) for a in (hi, hv, hc))
        if k2 != 1:
            # the mirror's own arithmetic: rank[i, :k2] holds min(k2, n) items and the mean is taken over those
            V = np.stack([V[rank[i, :k2]].mean(axis=0) for i in range(n)]).astype(np.float32)
            di, dv, dc = ops.rerank_expand(rank_d, k2, di, dv, dc)
            ei, ev, ec = di.cpu().numpy(), dv.cpu().numpy(), dc.cpu().numpy()
            for i in range(n):
                cols = np.nonzero(V[i])[0]
                assert ec[i] == len(cols) and np.array_equal(ei[i, :ec[i]], cols), (k1, k2, i)
                np.testing.assert_allclose(ev[i, :ec[i]], V[i, cols], rtol=3 * 2.0 ** -23, atol=0,
                                           err_msg=f"k2 mean: n={n} k1={k1} k2={k2} item {i}")
            hi, hv, hc = _sparse(V, k2 * stride)                 # and again the host's values for what follows
            di, dv, dc = (torch.from_numpy(a).to(dev) for a in (hi, hv, hc))
        # ---- inverted index
        col_off, inv_row, inv_val = ops.rerank_invert(di, dv, dc)
        co, ir, iv = col_off.cpu().numpy(), inv_row.cpu().numpy(), inv_val.cpu().numpy()
        cols = [np.nonzero(V[:, c])[0] for c in range(n)]
        assert co[0] == 0 and np.array_equal(np.diff(co), [len(c) for c in cols])
        for c in range(n):
            assert np.array_equal(ir[co[c]:co[c + 1]], cols[c]), c
            assert np.array_equal(iv[co[c]:co[c + 1]], V[cols[c], c]), c
        # ---- Jaccard + blend: the host loop of the mirror, bit for bit
        jac = np.zeros((nq, n), np.float32)
        for i in range(nq):
            s = np.zeros(n, np.float32)
            for c in np.nonzero(V[i])[0]:
                s[cols[c]] += np.minimum(V[i, c], V[cols[c], c])
            jac[i] = 1.0 - s / (2.0 - s)
        want = (jac * (1.0 - lam) + O[:nq] * lam)[:, nq:]
        assert want.dtype == np.float32
        dist = torch.from_numpy(np.ascontiguousarray(d32[:nq, nq:])).to(dev)
        got = ops.rerank_jaccard(di, dv, dc, col_off, inv_row, inv_val, torch.from_numpy(colmax).to(dev), dist, lam)
        got = got.cpu().numpy()
        print(f"{nq} x {n - nq} k1={k1} k2={k2} lambda={lam}: Jaccard pass max|dev - host| = "
              f"{np.abs(got - want).max():.1e}")
        assert np.array_equal(got, want)


def test_stages_against_the_host_mirror(dev):
    """Every stage on its own, fed from the host.  Rank lists from fp64 distances (ties: lowest index).
    Exact: the member sets, the inverted index, the Jaccard pass + blend (same fp32 operations in the same order as the
    host loop, bit for bit).  The weights are compared at 2e-6: expf against numpy's exp (a few ulp of values <= 1)
    and one fp32 dot product per distance where the host holds a rounded fp64 one (d = 256: <= 1e-6 on D <= 4,
    2 D dD / m <= 1e-6 on O); the k2 mean at 3 ulp (numpy divides the fp32 sum in double and rounds once more)."""
    q, g = _small()
    _stages(q, g, ((20, 6, 0.3), (25, 1, 0.0), (10, 3, 0.5), (31, 8, 0.2)), dev)


def test_stages_with_duplicate_rows(dev):
    """The same checks with rows present twice (q[:8] = g[10:18], g[40:44] = g[50:54]): distance-0 ties inside the
    rank lists, members at O = 0 (weight exp(0)), self-distances of either sign in fp32.  This is where duplicates
    are checked by VALUE: every stage has the host's input, so no near-tie decides what is compared."""
    q, g = _small(duplicates=True)
    assert torch.equal(q[:8], g[10:18]) and torch.equal(g[40:44], g[50:54])
    _stages(q, g, ((20, 6, 0.3), (10, 3, 0.5)), dev)


def test_stages_with_more_query_rows_than_jaccard_workgroups(dev):
    """Q = 1100 > the 1024 workgroups of rerank_jaccard_kernel: 76 workgroups serve a second query row on the scratch
    row the first one left behind, which has to be zero again — the Jaccard pass + blend stay bit for bit.  n = 3400
    also gives every thread of the inverted index's scan four columns.  d = 64; the host side of the comparison
    (fp64 distances, a stable argsort, the mirror's loops) takes 5.8 s on the CPU."""
    q, g, _, _ = synth.retrieval_problem(1100, 2300, dim=64, seed=7, **PROBLEM)
    _stages(q, g, ((20, 6, 0.3),), dev)


@pytest.mark.parametrize("nq,ng", [(2, 4), (3, 9)])
def test_stages_with_fewer_items_than_neighbours(dev, nq, ng):
    """n = Q + G = 6 and 12 items, k1 + 1 = 21 / 32 and k2 = 6 / 8 neighbours asked for: every rank list ends in -1
    entries (n <= k1, and n < k2 at n = 6, k2 = 8).  The mirror — like the reference, np.mean over
    V[initial_rank[i, :k2]] — takes the k2 mean over the min(k2, n) rows that exist, and so must rerank_expand_kernel.
    (A kernel that divides by k2 whatever the list holds — as this one did — returns 6/8 of the mirror's values at
    n = 6, k2 = 8 and fails the k2-mean comparison there.)"""
    q, g, _, _ = synth.retrieval_problem(nq, ng, dim=64, seed=7, **PROBLEM)
    _stages(q, g, ((20, 6, 0.3), (31, 8, 0.3)), dev)


def test_matches_the_reference_outputs(dev):
    """tests/golden/rerank_small.npz: the REFERENCE's outputs for a 24 x 90 problem at three settings, every entry
    compared.  Tolerance: the reference's own rounding noise — max |host mirror on fp32 oracle distances - golden|
    over the three settings, measured here (~3e-7) — times 8, for expf against numpy's exp and one different
    summation order in the distances.  fp32 route."""
    g = load_golden("rerank_small")
    q, gal, _, _ = synth.retrieval_problem(int(g["Q"]), int(g["G"]), dim=int(g["dim"]), seed=int(g["seed"]), **PROBLEM)
    assert (q.shape[0], gal.shape[0], q.shape[1], int(g["seed"])) == (24, 90, 256, 31)
    settings = {"k20_6_3": (20, 6, 0.3), "k25_1_0": (25, 1, 0.0), "k10_3_5": (10, 3, 0.5)}
    qg, qq, gg = (om.pairwise_distance(a, b).numpy() for a, b in ((q, gal), (q, q), (gal, gal)))
    noise = max(np.abs(rr.re_ranking(qg.copy(), qq.copy(), gg.copy(), k1=k1, k2=k2, lambda_value=lam) - g[key]).max()
                for key, (k1, k2, lam) in settings.items())
    tol = 8 * float(noise)
    print(f"reference noise (host mirror, fp32 distances, vs golden) = {noise:.2e}; tolerance = {tol:.2e}")
    assert 0 < noise < 1e-6
    qd, gd = q.to(dev), gal.to(dev)
    for key, (k1, k2, lam) in settings.items():
        got = rr.re_ranking_features(qd, gd, k1=k1, k2=k2, lambda_value=lam, precision="fp32")
        assert got.shape == g[key].shape and got.dtype == torch.float32 and got.is_cuda
        err = np.abs(got.cpu().numpy() - g[key]).max()
        print(f"{key}: device max|got - reference| = {err:.2e}")
        assert err <= tol, (key, err, tol)


MID = {"96x800": (96, 800, 77), "256x4000": (256, 4000, 78)}
MID_CASES = [("96x800", 20, 6, 0.3, 0.002), ("96x800", 20, 1, 0.1, 0.002), ("256x4000", 25, 1, 0.0, 0.001)]


@functools.lru_cache(maxsize=None)
def _mid_problem(name):
    nq, ng, seed = MID[name]
    q, g, _, _ = synth.retrieval_problem(nq, ng, dim=4096, seed=seed, **PROBLEM)
    return q, g, tuple(om.pairwise_distance(a, b).numpy() for a, b in ((q, g), (q, q), (g, g)))


@functools.lru_cache(maxsize=None)
def _mid_want(name, k1, k2, lam):
    _, _, (qg, qq, gg) = _mid_problem(name)
    return rr.re_ranking(qg, qq, gg, k1=k1, k2=k2, lambda_value=lam)


@pytest.mark.parametrize("route", ["fp32", "f16mx", "bf16x3"])
@pytest.mark.parametrize("name,k1,k2,lam,cap", MID_CASES)
def test_mid_size_4096d_on_every_parity_route(dev, route, name, k1, k2, lam, cap):
    """4096-d descriptors, each neighbour-search route of the 1e-4 class (f16mx resolves to f16r), against the host
    mirror on the oracle's fp32 distance matrices.  Set membership is discontinuous: a near-tie in a neighbour list
    moves single entries by ~0.02, so the SHARE of entries off by more than 1e-5 is bounded (0.2 % / 0.1 %: what a
    +-2e-6 relative perturbation of the distances moves on the CPU is 0.15 % / 0.011 %), every other entry meets
    1e-5, and all entries lie in [0, 1]."""
    q, g, _ = _mid_problem(name)
    want = _mid_want(name, k1, k2, lam)
    if route == "f16mx":
        assert ops.topk_precision(route, torch.float32, k1 + 1) == ops.F16R
    got = rr.re_ranking_features(q.to(dev), g.to(dev), k1=k1, k2=k2, lambda_value=lam, precision=route).cpu().numpy()
    assert got.shape == want.shape
    diff = np.abs(got - want)
    off = diff > 1e-5
    share = float(off.mean())
    inside = float(diff[~off].max())
    print(f"{name} k1={k1} k2={k2} lambda={lam} {route}: share of entries off by > 1e-5 = {share:.5%} "
          f"(cap {cap:.1%}), largest error of the others = {inside:.2e}, largest of all = {diff.max():.2e}")
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0
    assert share <= cap


def test_two_calls_are_bit_identical(dev):
    q, g, _ = _mid_problem("96x800")
    qd, gd = q.to(dev), g.to(dev)
    for route in ("fp32", "f16mx"):
        a = rr.re_ranking_features(qd, gd, k1=20, k2=6, lambda_value=0.3, precision=route)
        b = rr.re_ranking_features(qd, gd, k1=20, k2=6, lambda_value=0.3, precision=route)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
    h = rr.re_ranking_features(qd.half(), gd.half(), k1=20, k2=1, lambda_value=0.0)
    w = rr.re_ranking_features(qd.half().float(), gd.half().float(), k1=20, k2=1, lambda_value=0.0)
    assert torch.equal(h, w)                                  # 16-bit stored rows are widened exactly


SEED = 7
# (Q, G, d, k1, k2, lambda, cap on the share of entries off by more than 1e-5, routes)
ALL_ROUTES = ("fp32", "f16mx", "bf16x3")
EDGE_CASES = [
    # n = 8464: the neighbour search runs in two blocks of rows (7680 + 784), the row extremes walk two column tiles
    # per workgroup.  CPU: a +-2e-6 relative and absolute perturbation of the distances moves 0.0000 % of the entries
    (64, 8400, 64, 20, 1, 0.3, 0.001, ("fp32", "f16mx")),
    # d = 100 is padded to 128; k1 = 31 and k2 = 8 are both limits; lambda = 1 is the pure distance term; one query.
    # CPU: the same perturbation moves no entry by more than 1.4e-6
    (40, 200, 100, 31, 8, 0.2, 0.0, ("fp32", "f16mx")),
    (40, 200, 100, 31, 8, 1.0, 0.0, ("fp32", "f16mx")),
    (1, 50, 100, 10, 3, 0.5, 0.0, ("fp32", "f16mx")),
    # n <= k1 (and n < k2): rank lists padded with -1 out of every route's top-k; mirror and reference agree exactly
    (2, 4, 64, 20, 6, 0.3, 0.0, ALL_ROUTES),
    (3, 9, 64, 20, 6, 0.3, 0.0, ALL_ROUTES),
    (5, 17, 64, 20, 6, 0.3, 0.0, ALL_ROUTES),
    (3, 9, 36, 20, 6, 0.3, 0.0, ALL_ROUTES),
    (2, 5, 64, 31, 8, 0.3, 0.0, ALL_ROUTES),
]


@functools.lru_cache(maxsize=None)
def _edge_problem(nq, ng, dim):
    q, g, _, _ = synth.retrieval_problem(nq, ng, dim=dim, seed=SEED, **PROBLEM)
    return q, g


@functools.lru_cache(maxsize=None)
def _edge_want(nq, ng, dim, k1, k2, lam):
    q, g = _edge_problem(nq, ng, dim)
    qg, qq, gg = (om.pairwise_distance(a, b).numpy() for a, b in ((q, g), (q, q), (g, g)))
    return rr.re_ranking(qg, qq, gg, k1=k1, k2=k2, lambda_value=lam)


@pytest.mark.parametrize("nq,ng,dim,k1,k2,lam,cap,route",
                         [c[:7] + (r,) for c in EDGE_CASES for r in c[7]],
                         ids=lambda v: str(v))
def test_edges_end_to_end_against_the_host_mirror(dev, nq, ng, dim, k1, k2, lam, cap, route):
    """re_ranking_features against the host mirror on the oracle's fp32 distance matrices, at the shapes listed at
    EDGE_CASES, with the convention of the mid-size test: the share of entries off by more than 1e-5 is capped (0.1 %
    at n = 8464, 0 everywhere else: what the CPU perturbation experiment noted there allows), every other entry
    meets 1e-5, all values are finite.  The mirror of the 64 x 8400 case takes 9.9 s on the CPU, once for both routes.
    The measured share and the largest errors are printed per case; device figures have not been recorded here yet:
    the expectations above come from the code and from the CPU experiments."""
    q, g = _edge_problem(nq, ng, dim)
    want = _edge_want(nq, ng, dim, k1, k2, lam)
    n = nq + ng
    if n > 8192:
        assert max(256, min(n, (1 << 26) // n // 256 * 256)) < n      # really more than one block of rows
    got = rr.re_ranking_features(q.to(dev), g.to(dev), k1=k1, k2=k2, lambda_value=lam, precision=route)
    assert got.shape == want.shape and got.dtype == torch.float32
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    diff = np.abs(got - want)
    off = diff > 1e-5
    share = float(off.mean())
    inside = float(diff[~off].max()) if (~off).any() else 0.0
    print(f"{nq} x {ng} d={dim} k1={k1} k2={k2} lambda={lam} {route}: share of entries off by > 1e-5 = {share:.5%} "
          f"(cap {cap:.1%}), largest error of the others = {inside:.2e}, largest of all = {diff.max():.2e}")
    assert share <= cap


def test_row_extremes_with_several_column_tiles_per_workgroup(dev):
    """rerank_row_extremes at n = 8464, d = 64 against fp64 values computed in blocks of rows on the host, at the
    bounds of the stage test (norms rtol 1e-6, maxima rtol 4e-6; a dot product of 64 terms can only do better than
    one of 256).  The rule of csrc/rerank.hip — 128-row tiles, about 4096 workgroups: chunks = min(ceil(4096 /
    tiles), tiles) ranges of ceil(tiles / chunks) column tiles — gives 67 tiles in ranges of 2, the last range one
    tile: the running maximum is carried across tiles and the last range is ragged.  The rule is restated here and
    checked against the workspace size the library asks for (one partial per row and range), so that a retuned rule
    fails this test instead of emptying it."""
    q, g = _edge_problem(64, 8400, 64)
    x = torch.cat([q, g])
    n, d = map(int, x.shape)
    tiles = -(-n // 128)
    chunks = min(-(-4096 // tiles), tiles)
    per = -(-tiles // chunks)
    ranges = -(-tiles // per)
    assert per > 1 and tiles % per != 0, (tiles, per)
    from openibl_amd import lib
    assert lib.load().oibl_rerank_row_extremes_workspace_bytes(n, d) == -(-ranges * n * 4 // 256) * 256
    xd = x.double()
    nn = (xd ** 2).sum(1)
    want = torch.zeros(n, dtype=torch.float64)
    for lo in range(0, n, 1024):
        D = nn[lo:lo + 1024, None] + nn[None, :] - 2.0 * xd[lo:lo + 1024] @ xd.T
        want = torch.maximum(want, (D ** 2).max(dim=0).values)
    norms, rowmax = ops.rerank_row_extremes(x.to(dev))
    norms, rowmax = norms.cpu().numpy(), rowmax.cpu().numpy()
    nerr, merr = np.abs(norms / nn.numpy() - 1).max(), np.abs(rowmax / want.numpy() - 1).max()
    print(f"n={n}: {tiles} tiles, {ranges} ranges of {per}; largest relative error: norms {nerr:.2e}, maxima {merr:.2e}")
    np.testing.assert_allclose(norms, nn.numpy(), rtol=1e-6)
    np.testing.assert_allclose(rowmax, want.numpy(), rtol=4e-6)


@pytest.mark.parametrize("route", ALL_ROUTES)
@pytest.mark.parametrize("storage", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_16_bit_stored_rows_equal_their_widened_copies(dev, storage, route):
    """Rows stored in fp16 / bf16 are widened exactly on every route: the result is the one of the same rows handed
    over as fp32, bit for bit (24 x 90, d = 256, k1 = 20, k2 = 6, lambda = 0.3)."""
    q, g = _small()
    qs, gs = q.to(dev).to(storage), g.to(dev).to(storage)
    got = rr.re_ranking_features(qs, gs, k1=20, k2=6, lambda_value=0.3, precision=route)
    wide = rr.re_ranking_features(qs.float(), gs.float(), k1=20, k2=6, lambda_value=0.3, precision=route)
    assert got.shape == (24, 90) and got.dtype == torch.float32 and wide.dtype == torch.float32
    assert torch.equal(got, wide)


def test_duplicate_rows_end_to_end(dev):
    """The duplicate problem of test_stages_with_duplicate_rows through re_ranking_features, every route: all values
    finite, <= 1 and >= -1e-6, two calls bit-identical.  No comparison of values here: on the CPU the mirror itself
    reaches -3.3e-7 on this input and an absolute 2e-6 perturbation of the distances moves up to 10 % of its entries
    (the ties at distance 0 decide the rank lists), so it would compare noise — the stage test is where duplicates
    are checked by value."""
    q, g = _small(duplicates=True)
    qd, gd = q.to(dev), g.to(dev)
    for route in ALL_ROUTES:
        a = rr.re_ranking_features(qd, gd, k1=20, k2=6, lambda_value=0.3, precision=route)
        b = rr.re_ranking_features(qd, gd, k1=20, k2=6, lambda_value=0.3, precision=route)
        lo, hi = float(a.min()), float(a.max())
        print(f"duplicates, {route}: values span {lo:.3e} .. {hi:.6f}")
        assert bool(torch.isfinite(a).all()) and hi <= 1.0 and lo >= -1e-6
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_no_dense_square_at_2048_x_30000(dev):
    """n = 32048: the (Q+G)^2 float32 array of the host flow would be 4.1 GB (the reference builds two).  The peak
    device memory the call adds — workspaces included, they are released first — stays below HALF of one such
    square; the planted positives of every query of this hard_fraction = 0 problem rank first; lambda = 0 outputs lie
    in [0, 1]."""
    nq, ng = 2048, 30000
    q, g, gt, _ = synth.retrieval_problem(nq, ng, dim=4096, seed=5, hard_fraction=0.0)
    qd, gd = q.to(dev), g.to(dev)
    ops.release_workspaces()
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = rr.re_ranking_features(qd, gd, k1=25, k2=1, lambda_value=0.0)
    torch.cuda.synchronize(dev)
    added = torch.cuda.max_memory_allocated(dev) - before
    square = (nq + ng) ** 2 * 4
    print(f"peak device memory added: {added / 1e9:.3f} GB; one (Q+G)^2 float32 array: {square / 1e9:.3f} GB")
    assert added < square // 2
    assert out.shape == (nq, ng)
    lo, hi = float(out.min()), float(out.max())
    print(f"values span {lo:.4f} .. {hi:.4f}")
    assert 0.0 <= lo and hi <= 1.0
    _, top = ops.row_topk(out, 2)
    top = top.cpu().numpy()
    assert all(sorted(top[i].tolist()) == gt[i] for i in range(nq))
    # the problem on which the host mirror was checked to do the same for all 128 queries (values 0.26 .. 1.0)
    q, g, gt, _ = synth.retrieval_problem(128, 2000, dim=4096, seed=5, hard_fraction=0.0)
    out = rr.re_ranking_features(q.to(dev), g.to(dev), k1=25, k2=1, lambda_value=0.0)
    print(f"128 x 2000: values span {float(out.min()):.4f} .. {float(out.max()):.4f}")
    assert 0.0 <= float(out.min()) and float(out.max()) <= 1.0
    top = ops.row_topk(out, 2)[1].cpu().numpy()
    assert all(sorted(top[i].tolist()) == gt[i] for i in range(128))


def test_evaluator_device_rerank_gives_the_host_flow_recalls(dev):
    """Evaluator(device_rerank=True).evaluate(rerank=True) against the host flow, through a stub model whose
    'images' are the 4096-d descriptors themselves.  160 queries (half of them hard) x 1500 gallery rows, rr_topk = 25,
    lambda = 0.1.  The problem was chosen so that the host flow's Recall@1/5/10 do not move under a +-2e-6 relative
    perturbation of every distance on the CPU (checked with five seeds when this test was written): the comparison
    does not hang on a near-tie."""
    from ibl.evaluators import Evaluator
    from ibl.utils.data.sampler import DistributedSliceSampler

    class Stub(torch.nn.Module):
        def forward(self, x):
            return x

    class Rows(torch.utils.data.Dataset):
        def __init__(self, rows, records):
            self.rows, self.records = rows, records

        def __len__(self):
            return len(self.records)

        def __getitem__(self, i):
            f, pid, x, y = self.records[i]
            return self.rows[i], f, pid, x, y

    nq, ng = 160, 1500
    q, g, gt, pids = synth.retrieval_problem(nq, ng, dim=4096, seed=91, **PROBLEM)
    query = [(f"q{i}.png", 100000 + i, 0.0, 0.0) for i in range(nq)]
    gallery = [(f"g{j}.png", pids[j], 0.0, 0.0) for j in range(ng)]
    qset, gset = Rows(q, query), Rows(g, gallery)

    def loader(ds):
        return torch.utils.data.DataLoader(ds, batch_size=64, num_workers=0, shuffle=False,
                                           sampler=DistributedSliceSampler(ds, num_replicas=1, rank=0))

    model = Stub().to(dev).eval()
    args = dict(rerank=True, rr_topk=25, lambda_value=0.1)
    r_host = Evaluator(model).evaluate(loader(qset), query + gallery, query, gallery, gt,
                                       gallery_loader=loader(gset), **args)
    r_dev = Evaluator(model, device_rerank=True).evaluate(loader(qset), query + gallery, query, gallery, gt,
                                                          gallery_loader=loader(gset), **args)
    r_one = Evaluator(model, device_rerank=True).evaluate(loader(Rows(torch.cat([q, g]), query + gallery)),
                                                          query + gallery, query, gallery, gt, **args)
    d = rr.re_ranking(*(om.pairwise_distance(a, b).numpy() for a, b in ((q, g), (q, q), (g, g))),
                      k1=25, k2=1, lambda_value=0.1)
    want = om.evaluate_all(d, gt, pids)
    print("re-ranked recalls: host flow", r_host, "device", r_dev, "device, one loader", r_one, "oracle", want)
    assert np.array_equal(r_host, want) and np.array_equal(r_dev, want) and np.array_equal(r_one, want)
    assert 0.3 < want[0] < 1.0
