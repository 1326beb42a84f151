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
