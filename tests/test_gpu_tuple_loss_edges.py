"""The fused losses on the device (csrc/loss.hip; ops.tuple_loss, ops.soft_label_loss) at their limits and in saturation,
against the numpy float64 evaluation of the same formulas (tests/helpers/tuple_loss_ref.py: EDGE_CASES, EDGE_SOFT), which
tests/test_tuple_loss_cpu.py ties to the reference's own float64 autograd (tests/golden/tuple_loss_edges.npz) and to its
np.longdouble twin.

The bar is derived, not taken from the reference's fp32 run (whose logits carry 1e-7 |z|: useless at |z| = 850).  The
kernels accumulate in fp64 and round once, so per case and mode, for the loss (relative) and each gradient (rel_max):
    2^-23  +  4 L 2^-53 S        one fp32 rounding, doubled  +  an fp64 sum over L terms re-associated, through a softmax
with S the largest sum_e |term_e| over the rows of the case (sum |a_e x_e| / temp, or sum d_e^2; at least 1); for the
soft-label loss L = 1, S = max |x| / temp, plus 2^-53 J for the softmax sums.  Where a float64 coefficient is exactly 0
(a switched-off hinge, a weight that underflowed) the device's row must be exactly 0; the inputs keep every coefficient
at exactly 0 or >= 1e-30 and every hinge argument 1e-3 away from 0 (asserted on the CPU).

G1  the finish kernel across waves: 260 and 280 table entries, 70 / 300 / 513 tuples (thread loops of 2 and 3 trips)
G2  B = 65535 runs, B = 65536 and M = 65 raise
G3  ragged rows: L = 1, 2, 3, 5, 7, 33, 36, 2051, 8196, 8200 (empty chunks, a last chunk of one group, partial groups)
G4  strides the validation admits: a last-dimension stride of 3 at L = 1, expanded (stride 0) anchors and negatives
G5  unaligned gradient pointers through the C entry point: 4-byte stores of full groups, guard elements untouched
R1  hard negatives dominate (logit gaps up to 1.7e3)   R2  the positive dominates (weights exactly 0)
R3  coincident rows   R4  whole tuples switched off / on   R5  the upstream gradient, two losses on one graph, streams
S1  J around the 256-thread stride, B > 256   S2  one-hot teachers and students   S3  student = teacher: gradient 0

Measured on an MI355X, worst case per group, error against float64 (loss | largest of the three gradients; bar):
  G1 5.2e-8 | 5.4e-8 (1.19e-7)   G2 3.0e-8 | 3.5e-8 (1.19e-7)   G3 4.1e-8 | 5.7e-8 (1.19e-7)   G4 3.4e-8 | 5.2e-8
  G5 3.8e-8 | 5.0e-8   R1 2.7e-8 | 4.7e-8 (1.19e-7; 1.45e-7 at L = 32768)   R2 4.3e-8 | 4.9e-8   R3 4.7e-8 | 5.8e-8
  R4 3.8e-8 | 4.3e-8   R5 3.1e-8 | 5.7e-8   S1 2.8e-8 | 4.2e-8   S2 3.6e-8 | 4.8e-8   S3 3.4e-8 | exactly 0
At most 0.49 of any bar: every figure is the rounding of the fp32 result (2^-24 = 6.0e-8).  The tie of R3 in sare_ind
with the dot score: table entry 0.59523809523809501 against uscale / (2 count) = 0.59523809523809512, 1 ulp of fp64
(a contracted product; see test_coincident_rows); exact for the squared distance."""
import numpy as np
import pytest
import torch

from helpers import tuple_loss_ref as ref
from openibl_amd import lib, ops

pytestmark = pytest.mark.gpu

G1 = ("g1_b4m64l8", "g1_b70m3l8", "g1_b300m2l8", "g1_b513m1l4")
G3 = tuple(k for k in ref.EDGE_CASES if k.startswith("g3_"))
REGIMES = ("r1", "r2", "r3", "r4_off", "r4_on", "r4_mixed", "r5", "r1_big", "r2_big")
AGAINST_FLOAT64 = G1 + ("g2_b65535m1l4",) + G3 + REGIMES
PAIRS = [(name, mode) for name in AGAINST_FLOAT64 for mode in ref.edge_modes(name)]
ALL_MODES = list(ref.MODES)


def leaves(rows, dev):
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dev).requires_grad_(True) for t in rows]


def run(name, mode, a, p, n, scale=None):
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    loss = ops.tuple_loss(a, p, n, kind, margin=margin, temp=temp, score=score)
    (loss if scale is None else scale * loss).backward()
    return loss.detach()


def grads(*tensors):
    return [t.grad.clone() for t in tensors]


def check_against_float64(name, mode, loss, got):
    """Print the errors beside the bar and assert them; rows whose float64 coefficient is exactly 0 must be exactly 0."""
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    w_loss, *w_grads = ref.edge_want(name, mode)
    bar = ref.edge_bar(name, mode)
    got = [g.cpu().numpy() for g in got]
    e_loss = abs(float(loss) - w_loss) / abs(w_loss) if w_loss != 0.0 else abs(float(loss))
    errs = [e_loss] + [ref.rel_max(g, w) for g, w in zip(got, w_grads)]
    print(f"{name} {mode}: loss {float(loss):.9g} (float64 {w_loss:.12g}); loss | da | dp | dn "
          + " ".join(f"{e:.3e}" for e in errs) + f"; bar {bar:.3e}")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and np.isfinite(float(loss))
    assert all(np.isfinite(g).all() for g in got), (name, mode)
    for k, e in zip(("loss", "da", "dp", "dn"), errs):
        assert e <= bar, (name, mode, k, e, bar)
    if w_loss == 0.0:
        assert float(loss) == 0.0
    u = ref.coefficients(ref.scores(*ref.edge_rows(name, mode), kind, score)[0], kind, score, margin, temp)[1]
    assert not got[2][u[:, 1:] == 0.0].any(), (name, mode, "negatives whose coefficient is 0")
    assert not got[1][u[:, 0] == 0.0].any() and not got[0][(u == 0.0).all(1)].any(), (name, mode)
    return errs


@pytest.mark.parametrize("name,mode", PAIRS)
def test_loss_and_gradients_against_float64(dev, name, mode):
    a, p, n = leaves(ref.edge_rows(name, mode), dev)
    loss = run(name, mode, a, p, n)
    check_against_float64(name, mode, loss, grads(a, p, n))
    assert torch.equal(run(name, mode, a, p, n), loss)                   # and the same bits a second time


def _ulp_apart(x, y):
    """|x - y| in units of the fp32 spacing at max(|x|, |y|), elementwise maximum."""
    big = torch.maximum(x.abs(), y.abs())
    spacing = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
    return float(((x.double() - y.double()).abs() / spacing).max())


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("name", G1)
def test_first_and_last_tuple_against_the_same_two_as_a_batch_of_two(dev, name, mode):
    """Tuple 0 (wave 0 of the finish kernel) and the last tuple (its last wave, or the last trip of its thread loop)
    depend on the batch through 1 / count only: times B / 2 they are the batch of two, to the bit where B / 2 is a
    power of two ((4, 64, 8) against (2, 64, 8)), within 1 ulp of the fp32 product otherwise."""
    B = ref.EDGE_CASES[name][1]
    a, p, n = leaves(ref.edge_rows(name, mode), dev)
    run(name, mode, a, p, n)
    two = [t.detach()[[0, B - 1]].clone().requires_grad_(True) for t in (a, p, n)]
    run(name, mode, *two)
    ratio = B / 2.0
    for whole, pair in zip((a, p, n), two):
        scaled = whole.grad[[0, B - 1]] * ratio
        if B == 4:
            assert torch.equal(scaled, pair.grad), (name, mode)
        else:
            d = _ulp_apart(scaled, pair.grad)
            assert d <= 1.0, (name, mode, d)


def test_limits_raise_and_launch_nothing(dev):
    z = lambda *s: torch.zeros(s, device=dev)                                                     # noqa: E731
    with pytest.raises(ValueError, match=r"\(65536, 1, 4\)"):
        ops.tuple_loss(z(65536, 4), z(65536, 4), z(65536, 1, 4), "sare_ind")
    with pytest.raises(ValueError, match=r"\(2, 65, 4\)"):
        ops.tuple_loss(z(2, 4), z(2, 4), z(2, 65, 4), "sare_joint")
    with pytest.raises(ValueError, match=r"\(65536, 1\)"):
        ops.soft_label_loss(z(65536, 1), z(65536, 1), 0.07, 0.07)
    h = lib.load()
    t = z(65536, 4)
    assert h.oibl_tuple_loss_forward(t.data_ptr(), 4, t.data_ptr(), 4, t.data_ptr(), 4, 4, 65536, 1, 4, 0, 0, 0.3, 0.07,
                                     t.data_ptr(), t.data_ptr(), t.data_ptr(), 1 << 20, None) == -1
    assert b"65535" in h.oibl_last_error()
    assert h.oibl_tuple_loss_backward(t.data_ptr(), 4, t.data_ptr(), 4, t.data_ptr(), 4, 4, 65536, 1, 4, 0, 0,
                                      t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), None) == -1
    assert h.oibl_soft_label_loss_forward(t.data_ptr(), t.data_ptr(), 65536, 1, 0.07, 0.07, t.data_ptr(), t.data_ptr(),
                                          t.data_ptr(), 1 << 20, None) == -1
    torch.cuda.synchronize()
    assert not t.any()


# ---- G4: strides ---------------------------------------------------------------------------------------------------
def _direct(name, mode, a, p, n):
    """Forward and backward through the two entry points of ops, no autograd: (loss, ga, gp, gn), compact."""
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    loss, coef = ops.tuple_loss_forward(a, p, n, kind, margin=margin, temp=temp, score=score)
    one = torch.ones((), dtype=torch.float32, device=a.device)
    return (loss,) + tuple(ops.tuple_loss_backward(a, p, n, coef, one, kind, score))


@pytest.mark.parametrize("mode", ALL_MODES)
def test_one_column_rows_with_a_last_dimension_stride_of_three(dev, mode):
    name = "g4_l1"
    a_np, p_np, n_np = ref.edge_rows(name, mode)
    B, M, _ = n_np.shape
    x = torch.full((B, 2 + M, 3), 7.0, device=dev)
    x[:, :, 0] = torch.from_numpy(np.concatenate((a_np[:, None], p_np[:, None], n_np), axis=1)[:, :, 0]).to(dev)
    x.requires_grad_(True)
    v = x[..., ::3]
    assert v.shape == (B, 2 + M, 1) and v.stride() == ((2 + M) * 3, 3, 3)
    loss = run(name, mode, v[:, 0], v[:, 1], v[:, 2:])
    a, p, n = leaves((a_np, p_np, n_np), dev)
    assert torch.equal(run(name, mode, a, p, n), loss)
    assert torch.equal(x.grad[:, 0, :1], a.grad) and torch.equal(x.grad[:, 1, :1], p.grad)
    assert torch.equal(x.grad[:, 2:, :1], n.grad) and not x.grad[..., 1:].any()
    check_against_float64(name, mode, loss, grads(a, p, n))


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("name", ("g4_l33", "g4_l36"))
def test_expanded_anchors_and_negatives(dev, name, mode):
    """Stride 0 in a leading dimension: one anchor for every tuple, one negative for every row of a tuple.  The
    kernels give the bits of the materialised copy; the gradient that reaches the source is autograd's fp32 sum of the
    compact gradient's rows (two of them: a sum whose order cannot matter)."""
    a, p, n = leaves(ref.edge_rows(name, mode), dev)
    B, M, L = n.shape
    assert B == 2 and M == 2
    for which in ("anchors", "negatives"):
        for t in (a, p, n):
            t.grad = None
        ea = a[:1].expand(B, L) if which == "anchors" else a
        en = n[:, :1].expand(B, M, L) if which == "negatives" else n
        assert (ea.stride(0) == 0) == (which == "anchors") and (en.stride(1) == 0) == (which == "negatives")
        views = _direct(name, mode, ea.detach(), p.detach(), en.detach())
        copies = _direct(name, mode, ea.detach().contiguous(), p.detach(), en.detach().contiguous())
        for v, c in zip(views, copies):
            assert torch.equal(v, c), (name, mode, which)
        loss = run(name, mode, ea, p, en)
        assert torch.equal(loss, copies[0])
        if which == "anchors":
            assert torch.equal(a.grad[:1], copies[1].sum(0, keepdim=True)) and not a.grad[1:].any()
            assert torch.equal(n.grad, copies[3])
        else:
            assert torch.equal(n.grad[:, :1], copies[3].sum(1, keepdim=True)) and not n.grad[:, 1:].any()
            assert torch.equal(a.grad, copies[1])
        assert torch.equal(p.grad, copies[2])
    c = leaves(ref.edge_rows(name, mode), dev)
    check_against_float64(name, mode, run(name, mode, *c), grads(*c))


# ---- G5: unaligned outputs through the C entry point ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES)
def test_unaligned_gradient_pointers_give_the_bits_of_aligned_ones(dev, mode):
    """L = 1000 (full groups of 4 columns) with gradient pointers 4 bytes off a 16-byte boundary: vec_out = 0, the
    4-byte stores of a full group.  Every pointer is valid for its whole extent; the sentinels around it stay."""
    name, front, back, sentinel = "g5_l1000", 5, 7, -12345.0
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    a, p, n = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in ref.edge_rows(name, mode))
    B, M, L = n.shape
    loss, coef = ops.tuple_loss_forward(a, p, n, kind, margin=margin, temp=temp, score=score)
    one = torch.ones((), dtype=torch.float32, device=dev)
    aligned = ops.tuple_loss_backward(a, p, n, coef, one, kind, score)
    h = lib.load()
    sizes = (B * L, B * L, B * M * L)
    for unaligned in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        bufs = [torch.full((front + size + back,), sentinel, device=dev) if u else torch.full((size,), sentinel, device=dev)
                for size, u in zip(sizes, unaligned)]
        ptrs = [b.data_ptr() + (4 * front if u else 0) for b, u in zip(bufs, unaligned)]
        assert all(b.data_ptr() % 16 == 0 for b in bufs) and [q % 16 for q in ptrs] == [4 if u else 0 for u in unaligned]
        lib.check(h.oibl_tuple_loss_backward(a.data_ptr(), L, p.data_ptr(), L, n.data_ptr(), M * L, L, B, M, L,
                                             ops.LOSS_KINDS[kind], ops.LOSS_SCORES[score], coef.data_ptr(),
                                             one.data_ptr(), *ptrs, torch.cuda.current_stream(dev).cuda_stream),
                  "tuple_loss_backward")
        torch.cuda.synchronize()
        for b, u, size, want in zip(bufs, unaligned, sizes, aligned):
            body = b[front:front + size] if u else b
            assert torch.equal(body, want.reshape(-1)), (mode, unaligned)
            if u:
                assert bool((b[:front] == sentinel).all()) and bool((b[front + size:] == sentinel).all()), (mode, unaligned)
    check_against_float64(name, mode, loss, aligned)


# ---- R3, R4, R5: what the float64 bar does not say ------------------------------------------------------------------
@pytest.mark.parametrize("mode", ALL_MODES)
def test_coincident_rows(dev, mode):
    """Two equal negatives get bit-equal gradients and table entries.  A negative equal to the positive has s_j = s_0
    to the bit, so the sigmoid of sare_ind is 1/2 and its table entry uscale (0.5 / count): exactly for the squared
    distance (z = -s), and for the dot score within 2^-52 max(1, |z_0|) — should the compiler contract z_j = s_j / temp
    into the subtraction of the rounded z_0, half an ulp of z_0 is left in the gap, and sigmoid'(0) = 1/4."""
    name = "r3"
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    a, p, n = leaves(ref.edge_rows(name, mode), dev)
    B, M, L = n.shape
    run(name, mode, a, p, n)
    assert torch.equal(n.grad[0, 2], n.grad[0, 3]) and torch.equal(n.grad[1, 2], n.grad[1, 3])
    assert torch.isfinite(a.grad).all() and torch.isfinite(p.grad).all() and torch.isfinite(n.grad).all()
    coef = ops.tuple_loss_forward(a.detach(), p.detach(), n.detach(), kind, margin=margin, temp=temp, score=score)[1].cpu()
    assert float(coef[0, 3]) == float(coef[0, 4]) and float(coef[1, 3]) == float(coef[1, 4])
    if kind == "sare_ind":
        uscale = 1.0 / temp if score == "dot" else 2.0
        want = uscale * (0.5 * (1.0 / (B * M)))
        z0 = np.abs(ref.scores(*ref.edge_rows(name, mode), kind, score)[0][:, 0]) / temp
        for b in (0, 1):                                        # tuple 0: negative 0 = anchor = positive
            slack = 0.0 if score == "sqdist" else 2.0 ** -52 * max(1.0, float(z0[b])) * want
            print(f"{name} {mode}: tie of tuple {b}: table {float(coef[b, 1]):.17g}, uscale / (2 count) {want:.17g}")
            assert abs(float(coef[b, 1]) - want) <= slack, (mode, b, float(coef[b, 1]), want)
    if kind == "triplet":                                       # d_p = sqrt(L) 1e-6: u_0 = -active / (count d_p)
        s0 = ref.scores(*ref.edge_rows(name, mode), kind, score)[0][0, 0]
        active = int((ref.hinge_arguments(*ref.edge_rows(name, mode), margin)[0] >= 0).sum())
        want = -active / (B * M * np.sqrt(s0))
        assert abs(float(coef[0, 0]) - want) <= ref.reassociation_term(L, 1.0) * abs(want)


@pytest.mark.parametrize("mode", ("triplet", "triplet_m03"))
def test_whole_tuples_switched_off_and_on(dev, mode):
    zeros = lambda t: torch.equal(t, torch.zeros_like(t))                                          # noqa: E731
    a, p, n = leaves(ref.edge_rows("r4_off", mode), dev)
    loss = run("r4_off", mode, a, p, n)
    assert float(loss) == 0.0 and zeros(a.grad) and zeros(p.grad) and zeros(n.grad)
    assert not torch.isnan(a.grad).any() and not torch.isnan(p.grad).any() and not torch.isnan(n.grad).any()
    for name in ("r4_on", "r4_mixed"):
        kind, score, margin, temp, _ = ref.edge_mode(name, mode)
        rows = ref.edge_rows(name, mode)
        B, M, L = rows[2].shape
        a, p, n = leaves(rows, dev)
        run(name, mode, a, p, n)
        coef = ops.tuple_loss_forward(a.detach(), p.detach(), n.detach(), kind, margin=margin, temp=temp)[1].cpu().numpy()
        dp = np.sqrt(ref.scores(*rows, kind, score)[0][:, 0])
        on = np.array([M, M] if name == "r4_on" else [0, M])
        want = -on / (B * M * dp)
        assert np.abs(coef[:, 0] - want).max() <= ref.reassociation_term(L, 1.0) * np.abs(want).max(), (name, mode)
        if name == "r4_mixed":
            assert float(coef[0, 0]) == 0.0 and not coef[0].any() and coef[1].all()
            assert zeros(a.grad[0]) and zeros(p.grad[0]) and zeros(n.grad[0]) and bool(n.grad[1].abs().amax(-1).gt(0).all())


@pytest.mark.parametrize("mode", ALL_MODES)
def test_the_upstream_gradient_two_losses_on_one_graph_and_a_side_stream(dev, mode):
    name = "r5"
    a, p, n = leaves(ref.edge_rows(name, mode), dev)
    loss = run(name, mode, a, p, n)
    plain = grads(a, p, n)

    def again(scale):
        for t in (a, p, n):
            t.grad = None
        assert torch.equal(run(name, mode, a, p, n, scale=scale), loss)
        return grads(a, p, n)

    for g in again(0.0):
        assert torch.equal(g, torch.zeros_like(g)) and not torch.isnan(g).any()
    for g, f in zip(again(-2.0), plain):
        assert torch.equal(g, -2.0 * f)
    # loss_hard + 0.5 loss_soft on one graph, as SFRSTrainer.train forms it
    seed, Bs, J, ts, tt, _ = ref.EDGE_SOFT["s1_b3j257"]
    s_np, t_np = ref.edge_soft("s1_b3j257")
    s = torch.from_numpy(s_np.copy()).to(dev).requires_grad_(True)
    t = torch.from_numpy(t_np.copy()).to(dev)
    ops.soft_label_loss(s, t, ts, tt).backward()
    soft_alone = s.grad.clone()
    for v in (a, p, n, s):
        v.grad = None
    kind, score, margin, temp, _ = ref.edge_mode(name, mode)
    hard, soft = ops.tuple_loss(a, p, n, kind, margin=margin, temp=temp, score=score), ops.soft_label_loss(s, t, ts, tt)
    (hard + 0.5 * soft).backward()
    for g, f in zip(grads(a, p, n), plain):
        assert torch.equal(g, f)
    assert torch.equal(s.grad, 0.5 * soft_alone)
    # a side stream: its own workspace, the same bits
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    for v in (a, p, n):
        v.grad = None
    with torch.cuda.stream(side):
        loss_side = run(name, mode, a, p, n)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(loss_side, loss)
    for g, f in zip(grads(a, p, n), plain):
        assert torch.equal(g, f)


# ---- the soft-label loss -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.EDGE_SOFT))
def test_soft_label_loss_against_float64(dev, name):
    seed, B, J, ts, tt, regime = ref.EDGE_SOFT[name]
    s_np, t_np = ref.edge_soft(name)
    s = torch.from_numpy(s_np.copy()).to(dev).requires_grad_(True)
    t = torch.from_numpy(t_np.copy()).to(dev)
    loss = ops.soft_label_loss(s, t, ts, tt)
    loss.backward()
    w_loss, w_ds = ref.soft_label_loss(s_np, t_np, ts, tt)
    bar = sum(ref.soft_bar_terms(name))
    got = s.grad.cpu().numpy()
    e_loss = abs(float(loss) - w_loss) / abs(w_loss) if w_loss != 0.0 else abs(float(loss))
    e_ds = ref.rel_max(got, w_ds)
    print(f"soft {name}: loss {float(loss):.9g} (float64 {w_loss:.12g}); loss | ds {e_loss:.3e} {e_ds:.3e}; bar {bar:.3e}")
    assert np.isfinite(float(loss)) and np.isfinite(got).all()          # no 0 x inf behind an underflowed softmax
    assert e_loss <= bar and e_ds <= bar, (name, e_loss, e_ds, bar)
    if w_loss == 0.0:
        assert float(loss) == 0.0
    assert not got[w_ds == 0.0].any(), (name, "float64 says exactly 0")
    if regime in ("same", "same_sat"):
        # student = teacher bit for bit, equal temperatures: both softmaxes are the same numbers (sl_scaled keeps the
        # product x / temp one rounded value in the row maximum and in the terms), the gradient is exactly 0
        assert not s.grad.any(), (name, float(s.grad.abs().max()))
    assert torch.equal(ops.soft_label_loss(s, t, ts, tt).detach(), loss.detach())
