"""The formulas csrc/loss.hip implements (tests/helpers/tuple_loss_ref.py, numpy float64, written from the maths) against
the reference's own float64 autograd (tests/golden/tuple_loss.npz, tests/helpers/make_tuple_loss_golden.py): losses and
gradients to 1e-12 relative, the hinge and coverage conditions of the stored cases, and the host side of the six entry
points — validation returns before any HIP call, so it runs without a GPU."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from helpers import tuple_loss_ref as ref

TOL = 1e-12
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("tuple_loss")
    return _cache["g"]


def formula(name, mode):
    """(loss, da, dp, dn) of a case and mode in float64, once per session."""
    if (name, mode) not in _cache:
        kind, score, margin, temp, _ = ref.MODES[mode]
        _cache[name, mode] = ref.tuple_loss(*ref.case_rows(name), kind, score, margin, temp)
    return _cache[name, mode]


@pytest.mark.parametrize("mode", list(ref.MODES))
@pytest.mark.parametrize("name", list(ref.CASES))
def test_formulas_reproduce_the_reference_in_float64(name, mode):
    g = golden()
    loss, da, dp, dn = formula(name, mode)
    want = float(g[f"{name}_{mode}_loss"])
    assert abs(loss - want) <= TOL * abs(want), (loss, want)
    for k, t in (("da", da), ("dp", dp), ("dn", dn)):
        e = ref.rel_max(ref.sample(t), g[f"{name}_{mode}_{k}"])
        assert e <= TOL, (name, mode, k, e)


@pytest.mark.parametrize("name", list(ref.SOFT_CASES))
def test_soft_label_formula_reproduces_the_reference_in_float64(name):
    g = golden()
    seed, B, J, ts, tt = ref.SOFT_CASES[name]
    assert (int(g[f"soft_{name}_seed"]), tuple(g[f"soft_{name}_shape"]), tuple(g[f"soft_{name}_temps"])) == \
        (seed, (B, J), (ts, tt))
    loss, ds = ref.soft_label_loss(*ref.draw_soft(seed, B, J), ts, tt)
    want = float(g[f"soft_{name}_loss"])
    assert abs(loss - want) <= TOL * max(abs(want), 1.0), (loss, want)
    assert ref.rel_max(ref.sample(ds), g[f"soft_{name}_ds"]) <= TOL
    # the gradient of a row sums to zero: both softmaxes sum to one
    assert np.abs(ds.sum(1)).max() <= 1e-13 * max(1.0, np.abs(ds).max() * J)


def test_stored_cases_cover_the_stated_conditions():
    g = golden()
    shapes = {tuple(int(v) for v in g[f"{n}_shape"]) for n in ref.CASES}
    assert shapes == {(1, 1, 4, 0), (2, 3, 1000, 0), (3, 10, 32768, 0), (2, 10, 4096, 1)}
    assert {(B, J) for _, B, J, _, _ in ref.SOFT_CASES.values()} == {(1, 1), (3, 90), (2, 4096)}
    assert {ts == tt for _, _, _, ts, tt in ref.SOFT_CASES.values()} == {True, False}
    assert {(k, s) for k, s, _, _, _ in ref.MODES.values() if k != "triplet"} == \
        {(k, s) for k in ("sare_joint", "sare_ind") for s in ("sqdist", "dot")}
    assert {m for k, _, m, _, _ in ref.MODES.values() if k == "triplet"} == {0.1 ** 0.5, 0.3}
    for name, (seed, B, M, L, strided) in ref.CASES.items():
        a, p, n = ref.case_rows(name)
        assert a.dtype == np.float32 and n.shape == (B, M, L)
        np.testing.assert_allclose(np.linalg.norm(n.astype(np.float64), axis=-1), 1.0, atol=1e-6)
        for tag, margin in (("m", 0.1 ** 0.5), ("m03", 0.3)):
            h = ref.hinge_arguments(a, p, n, margin)
            np.testing.assert_allclose(h, g[f"{name}_hinge_{tag}"], rtol=0, atol=1e-12)
            assert np.abs(h).min() >= 1e-3, (name, margin)            # fp32 and float64 agree on the active set
            if M >= 6:
                assert 0 < int((h > 0).sum()) < h.size, (name, margin)
    h = ref.hinge_arguments(*ref.case_rows("b3m10l32768"), 0.1 ** 0.5)
    assert int((h > 0).sum()) == 18 and h.size == 30
    h = ref.hinge_arguments(*ref.case_rows("b2m10l4096_regions"), 0.3)
    assert int((h > 0).sum()) == 12 and h.size == 20


def test_an_inactive_hinge_has_a_zero_row_and_the_regions_follow_the_argmax():
    _, _, _, dn = formula("b3m10l32768", "triplet")
    h = ref.hinge_arguments(*ref.case_rows("b3m10l32768"), 0.1 ** 0.5)
    assert np.array_equal(np.abs(dn).max(-1) > 0.0, h > 0.0)
    seed, B, M, L, _ = ref.CASES["b2m10l4096_regions"]
    vec, score = ref.draw_regions(seed, B, M, L)
    np.testing.assert_array_equal(score, golden()["b2m10l4096_regions_score"])
    _, _, neg, arg = ref.select_regions(vec, score)
    assert len(set(arg.ravel().tolist())) > 3                          # the negatives do use different regions
    for b in range(B):
        for j in range(M):
            assert arg[b, j] == int(np.argmax(score[b, j])) and np.array_equal(neg[b, j], vec[b, 2 + j, arg[b, j]])


def test_batch_mean_is_the_mean_of_the_tuples_own_losses():
    """What SFRSTrainer._get_hard_loss relies on: one call over the batch = (1 / B) sum of the per-tuple calls."""
    a, p, n = ref.case_rows("b2m10l4096_regions")
    for mode, (kind, score, margin, temp, _) in ref.MODES.items():
        whole = ref.tuple_loss(a, p, n, kind, score, margin, temp)
        parts = [ref.tuple_loss(a[b:b + 1], p[b:b + 1], n[b:b + 1], kind, score, margin, temp) for b in range(len(a))]
        assert abs(whole[0] - sum(t[0] for t in parts) / len(a)) <= 1e-14, mode
        for b, t in enumerate(parts):
            assert ref.rel_max(whole[3][b] * len(a), t[3][0]) <= 1e-14, mode


def test_entry_points_validate_before_they_launch():
    """Out-of-limit arguments return OIBL_E_INVALID / OIBL_E_WORKSPACE with a message; no HIP call is made (there is
    no GPU here, and the pointers are host memory that is never dereferenced)."""
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(4096 + 256)
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    assert h.oibl_tuple_loss_workspace_bytes(4, 10) >= 4 * 11 * 9 * 8
    assert h.oibl_tuple_loss_workspace_bytes(1, 64) > 0 and h.oibl_tuple_loss_workspace_bytes(1, 65) == 0
    assert h.oibl_tuple_loss_workspace_bytes(0, 1) == 0 and h.oibl_tuple_loss_workspace_bytes(1, 0) == 0
    assert h.oibl_soft_label_loss_workspace_bytes(4, 4096) > 0 and h.oibl_soft_label_loss_workspace_bytes(4, 4097) == 0
    assert h.oibl_soft_label_loss_workspace_bytes(0, 9) == 0 and h.oibl_soft_label_loss_workspace_bytes(4, 0) == 0

    def fwd(B=1, M=1, L=4, mode=0, score=0, temp=0.07, a=ptr, ws=ptr, ws_bytes=4096, sa=4):
        return h.oibl_tuple_loss_forward(a, sa, ptr, 4, ptr, 4, 4, B, M, L, mode, score, 0.3, temp, ptr, ptr, ws,
                                         ws_bytes, None)

    def bwd(B=1, M=1, L=4, mode=0, score=0, ga=ptr, gp=ptr, gn=ptr, coef=ptr):
        return h.oibl_tuple_loss_backward(ptr, 4, ptr, 4, ptr, 4, 4, B, M, L, mode, score, coef, ptr, ga, gp, gn, None)

    for call, text in ((lambda: fwd(a=None), b"null"), (lambda: fwd(B=0), b"B"), (lambda: fwd(B=65536), b"B"),
                       (lambda: fwd(M=0), b"M"), (lambda: fwd(M=65), b"64"), (lambda: fwd(L=0), b"L=0"),
                       (lambda: fwd(mode=3), b"mode"), (lambda: fwd(mode=1, score=2), b"score"),
                       (lambda: fwd(mode=1, score=1, temp=0.0), b"temperature"), (lambda: fwd(sa=-4), b"stride"),
                       (lambda: bwd(coef=None), b"null"), (lambda: bwd(ga=None, gp=None, gn=None), b"no output"),
                       (lambda: bwd(M=65), b"64"), (lambda: bwd(B=0), b"B"), (lambda: bwd(mode=-1), b"mode")):
        assert call() == -1
        assert text in h.oibl_last_error(), (text, h.oibl_last_error())
    assert fwd(ws_bytes=8) == -2 and b"workspace" in h.oibl_last_error()
    assert fwd(ws=ptr + 8) == -2

    def soft(B=1, J=1, ts=0.07, tt=0.07, s=ptr, ws_bytes=4096):
        return h.oibl_soft_label_loss_forward(s, ptr, B, J, ts, tt, ptr, ptr, ptr, ws_bytes, None)

    for call, text in ((lambda: soft(s=None), b"null"), (lambda: soft(B=0), b"B"), (lambda: soft(J=0), b"J"),
                       (lambda: soft(J=4097), b"4096"), (lambda: soft(ts=0.0), b"temperatures"),
                       (lambda: soft(tt=-1.0), b"temperatures"),
                       (lambda: h.oibl_soft_label_loss_backward(ptr, 1, 4097, ptr, ptr, None), b"4096"),
                       (lambda: h.oibl_soft_label_loss_backward(None, 1, 1, ptr, ptr, None), b"null")):
        assert call() == -1
        assert text in h.oibl_last_error(), (text, h.oibl_last_error())
    assert soft(ws_bytes=0) == -2


def test_ops_validate_their_arguments_on_the_host():
    import torch
    from openibl_amd import ops
    from openibl_amd.lib import OpenIBLAmdError
    a, n = torch.zeros((2, 8)), torch.zeros((2, 3, 8))
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ops.tuple_loss(a, a, n, "triplet")
    with pytest.raises(ValueError, match="unknown loss"):
        ops.tuple_loss(a, a, n, "contrastive")
    with pytest.raises(ValueError, match="unknown score"):
        ops.tuple_loss(a, a, n, "sare_ind", score="cosine")
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ops.soft_label_loss(torch.zeros((2, 9)), torch.zeros((2, 9)), 0.07, 0.07)


# ---- the edge suite's cases (ref.EDGE_CASES, ref.EDGE_SOFT; tests/golden/tuple_loss_edges.npz) ----------------------
def edges_golden():
    if "e" not in _cache:
        _cache["e"] = load_golden("tuple_loss_edges")
    return _cache["e"]


EDGE_PAIRS = [(name, mode) for name in ref.EDGE_CASES for mode in ref.edge_modes(name)]


@pytest.mark.parametrize("name,mode", [(n, m) for n, m in EDGE_PAIRS if n in ref.EDGE_GOLDEN])
def test_edge_formulas_reproduce_the_reference_in_float64(name, mode):
    """Saturated logits, coincident rows, tuples switched off and on, an upstream gradient of -2: the float64 helper
    against the reference's own float64 autograd, to the tolerance of the plain cases."""
    g = edges_golden()
    assert (int(g[f"{name}_seed"]), tuple(g[f"{name}_shape"])) == (ref.EDGE_CASES[name][0], ref.EDGE_CASES[name][1:4])
    scale = ref.EDGE_SCALE.get(name, 1.0)
    assert float(g[f"{name}_scale"]) == scale
    loss, da, dp, dn = ref.edge_want(name, mode)
    want = float(g[f"{name}_{mode}_loss"])
    assert abs(loss - want) <= TOL * abs(want), (loss, want)
    for k, t in (("da", da), ("dp", dp), ("dn", dn)):
        e = ref.rel_max(ref.sample(scale * t, ref.EDGE_SAMPLE), g[f"{name}_{mode}_{k}"])
        assert e <= TOL, (name, mode, k, e)


@pytest.mark.parametrize("name", list(ref.EDGE_SOFT_GOLDEN))
def test_edge_soft_label_formula_reproduces_the_reference_in_float64(name):
    g = edges_golden()
    seed, B, J, ts, tt, regime = ref.EDGE_SOFT[name]
    assert (int(g[f"soft_{name}_seed"]), tuple(g[f"soft_{name}_shape"]), tuple(g[f"soft_{name}_temps"])) == \
        (seed, (B, J), (ts, tt))
    loss, ds = ref.soft_label_loss(*ref.edge_soft(name), ts, tt)
    want, want_ds = float(g[f"soft_{name}_loss"]), g[f"soft_{name}_ds"]
    assert np.isfinite(loss) and np.isfinite(ds).all()
    assert abs(loss - want) <= TOL * abs(want), (loss, want)
    if regime in ("same", "same_sat"):
        # the true gradient is 0: the helper says so exactly, the reference's log_softmax leaves roundings of the
        # gradient's natural scale 1 / (B ts)
        assert not ds.any() and np.abs(want_ds).max() <= TOL / (B * ts)
    else:
        assert ref.rel_max(ref.sample(ds, ref.EDGE_SAMPLE), want_ds) <= TOL


def _err(got, want):
    """|got - want| / |want| for scalars, the absolute difference where want is exactly 0."""
    got, want = float(got), float(want)
    return abs(got - want) / abs(want) if want != 0.0 else abs(got)


@pytest.mark.parametrize("name,mode", EDGE_PAIRS)
def test_float64_and_extended_precision_agree_within_the_reassociation_term(name, mode):
    """The reference side of the device's bar 2^-23 + 4 L 2^-53 S: the float64 helper against its np.longdouble twin
    stays inside the second term alone.  A case that does not is badly chosen (a result that is all cancellation)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    term = ref.edge_bar(name, mode) - ref.FP32_TERM
    w, x = ref.edge_want(name, mode), ref.edge_want(name, mode, np.longdouble)
    errs = [abs(w[0] - x[0]) / abs(x[0]) if w[0] != 0.0 else abs(x[0])]
    errs += [0.0 if not np.abs(g - h).max() else float(np.abs(g - h).max() / np.abs(g).max()) for g, h in zip(w[1:], x[1:])]
    assert max(errs) < term, (name, mode, errs, term)


@pytest.mark.parametrize("name", list(ref.EDGE_SOFT))
def test_soft_label_float64_and_extended_precision_agree(name):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 on this platform")
    _, B, J, ts, tt, _ = ref.EDGE_SOFT[name]
    term = ref.soft_bar_terms(name)[1]
    w, x = ref.soft_label_loss(*ref.edge_soft(name), ts, tt), ref.soft_label_loss(*ref.edge_soft(name), ts, tt, np.longdouble)
    e_loss = abs(w[0] - x[0]) / abs(x[0]) if w[0] != 0.0 else abs(x[0])
    d = float(np.abs(w[1] - x[1]).max())
    e_ds = d / float(np.abs(w[1]).max()) if w[1].any() else d
    assert max(e_loss, e_ds) < term, (name, e_loss, e_ds, term)


@pytest.mark.parametrize("name,mode", EDGE_PAIRS)
def test_edge_inputs_stay_out_of_the_underflow_band_and_off_the_hinges(name, mode):
    """Every coefficient and every loss is exactly 0 or at least 1e-30, every logit gap <= 60 or >= 800 (measured
    from the row's largest logit for sare_joint, from the positive's for sare_ind), no hinge argument within 1e-3 of
    0: fp32 flushing, denormal exps and the active set cannot separate the device from float64."""
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    a, p, n = ref.edge_rows(name, mode)
    assert a.dtype == np.float32 and not a.flags.writeable
    s = ref.scores(a, p, n, kind, score)[0]
    with np.errstate(under="ignore"):
        loss, u = ref.coefficients(s, kind, score, margin, temp)
    assert np.isfinite(u).all() and np.isfinite(loss)
    assert loss == 0.0 or abs(loss) >= ref.UNDERFLOW
    assert (np.abs(u[u != 0.0]) >= ref.UNDERFLOW).all(), np.abs(u[u != 0.0]).min()
    if kind == "triplet":
        assert np.abs(ref.hinge_arguments(a, p, n, margin)).min() >= ref.HINGE_GAP
    else:
        z = s / temp if score == "dot" else -s
        gap = z.max(1, keepdims=True) - z if kind == "sare_joint" else np.abs(z[:, 1:] - z[:, :1])
        assert ((gap <= ref.GAP_LOW) | (gap >= ref.GAP_HIGH)).all(), (name, mode)


def test_edge_regimes_are_the_stated_ones():
    """r1: negatives above the positive by >= 800 and rows whose weight is exactly 0; r2: negatives whose weight is
    exactly 0 next to ones that count; r3: the stated coincidences; r4: every hinge off, on, and one tuple of each."""
    for mode in ("joint_sqdist", "joint_dot", "ind_sqdist", "ind_dot"):
        kind, score, margin, temp, _ = ref.MODES[mode]
        for name in ("r1", "r1_big", "r2", "r2_big"):
            a, p, n = ref.edge_rows(name, mode)
            s = ref.scores(a, p, n, kind, score)[0]
            z = s / temp if score == "dot" else -s
            t = z[:, 1:] - z[:, :1]
            u = ref.coefficients(s, kind, score, margin, temp)[1]
            if name.startswith("r1"):
                assert (t.max(1) >= ref.GAP_HIGH).all() and (u[:, 1:] == 0.0).any() and np.abs(s).max() > 400 * temp
            else:
                assert (t < 0.0).all() and (u[:, 1:] == 0.0).sum() >= 3 * len(a) and (u[:, 1:] != 0.0).sum() >= 3 * len(a)
            if score == "dot":
                np.testing.assert_allclose(np.linalg.norm(n.astype(np.float64), axis=-1), ref.REGIME_NORM, rtol=1e-6)
    a, p, n = ref.edge_rows("r3", "triplet")
    assert np.array_equal(p[0], a[0]) and np.array_equal(n[0, 0], a[0]) and np.array_equal(n[0, 2], n[0, 3])
    assert np.array_equal(n[1, 0], p[1]) and np.array_equal(n[1, 2], n[1, 3]) and np.array_equal(n[1, 4], a[1])
    assert not np.array_equal(p[1], a[1])
    s = ref.scores(a, p, n, "triplet", "sqdist")[0]
    assert abs(np.sqrt(s[0, 0]) - np.sqrt(a.shape[1]) * ref.PD_EPS) <= 1e-18       # d_p = sqrt(L) 1e-6
    loss, u = ref.coefficients(ref.scores(a, p, n, "sare_ind", "dot")[0], "sare_ind", "dot", 0.3, 0.07)
    assert u[1, 1] == 0.5 / (n.shape[0] * n.shape[1]) / 0.07                        # the sigmoid of a tie is 1/2
    for mode in ("triplet", "triplet_m03"):
        m = ref.MODES[mode][2]
        assert (ref.hinge_arguments(*ref.edge_rows("r4_off", mode), -10.0) < 0).all()
        assert (ref.hinge_arguments(*ref.edge_rows("r4_on", mode), 10.0) > 0).all()
        h = ref.hinge_arguments(*ref.edge_rows("r4_mixed", mode), m)
        assert (h[0] < 0).all() and (h[1] > 0).all()
        w = ref.edge_want("r4_off", mode)
        assert w[0] == 0.0 and not any(g.any() for g in w[1:])
        w = ref.edge_want("r4_mixed", mode)
        assert not w[1][0].any() and not w[2][0].any() and not w[3][0].any() and w[3][1].all(-1).all()


def test_soft_edge_regimes_are_the_stated_ones():
    for name, (seed, B, J, ts, tt, regime) in ref.EDGE_SOFT.items():
        s, t = ref.edge_soft(name)
        assert s.dtype == np.float32 and s.shape == (B, J) and not s.flags.writeable
        loss, ds = ref.soft_label_loss(s, t, ts, tt)
        assert np.isfinite(loss) and np.isfinite(ds).all()
        assert loss == 0.0 or loss >= ref.UNDERFLOW
        assert (np.abs(ds[ds != 0.0]) >= ref.UNDERFLOW).all()
        for x, temp in ((s, ts), (t, tt)):
            gap = (x.astype(np.float64).max(1, keepdims=True) - x) / temp
            assert ((gap <= ref.GAP_LOW) | (gap >= ref.GAP_HIGH)).all(), name
            if (name.startswith("s2") or name == "s3_sat") and not (regime == "teacher_onehot" and x is s):
                assert gap.max() >= ref.GAP_HIGH             # (a one-hot teacher is read against a plain student)
        if regime in ("same", "same_sat"):
            assert np.array_equal(s, t) and ts == tt and not ds.any()
        if regime == "both_same":
            assert loss == 0.0 and not ds.any()
        if regime == "student_other":                        # the largest finite loss: (HOT - the rest) / ts
            assert loss > (ref.HOT - 0.5) / ts and (ds != 0.0).sum() == 2 * B
        if regime == "teacher_onehot":                       # -log p at one index
            k = np.arange(B) % J
            z = s.astype(np.float64) / ts
            want = np.mean(np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) - (z[np.arange(B), k] - z.max(1)))
            assert abs(loss - want) <= 1e-14 * want
