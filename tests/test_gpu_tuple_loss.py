"""The fused losses on the device (csrc/loss.hip; ops.tuple_loss, ops.soft_label_loss) against the numpy float64
evaluation of the same formulas (tests/helpers/tuple_loss_ref.py), which tests/test_tuple_loss_cpu.py ties to the
reference's own float64 autograd (tests/golden/tuple_loss.npz).

Bars, per case and mode: 8 x the error of the REFERENCE's fp32 autograd against its own float64 run, as
tests/helpers/make_tuple_loss_golden.py stored it (`ref_err`: |loss32 - loss64| / |loss64| and the relative max-norm of
each gradient over the full tensor).  The kernels compute in fp64 and round once, so each figure is the rounding of
the fp32 result.  Measured on an MI355X, relative max-norm, over the four shapes and six modes:
  reference (fp32 against float64)  loss 5.2e-10 .. 8.8e-7   gradients 1.1e-8 .. 1.1e-6
  device (against float64)          loss 5.2e-10 .. 5.0e-8   gradients 6.9e-9 .. 5.9e-8    at most 0.125 of any bar
  (3, 10, 32768): triplet 2.2e-8 | 4.7e-8 4.5e-8 3.3e-8, joint sqdist 3.2e-8 | 3.7e-8 3.7e-8 4.9e-8, joint dot 3.6e-9 |
    4.5e-8 3.6e-8 4.3e-8, ind sqdist 1.9e-8 | 3.7e-8 3.8e-8 4.9e-8, ind dot 9.0e-9 | 3.8e-8 3.1e-8 2.7e-8
  soft label: reference 3.8e-8 .. 5.6e-8 | 3.7e-7 .. 5.5e-7, device 3.5e-8 .. 5.0e-8 | 3.0e-8 .. 4.3e-8; (1, 1): exactly 0
The batch test: the issue asks for bit equality of tuple 0 in a batch of 3 against tuple 0 alone "where the factor is
a power of two"; 3 is none, so the batch of 3 is held to 1 ulp in every mode and bit equality is asserted where the
count ratio is 2 (batches of 2 and 4), also in every mode."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import tuple_loss_ref as ref
from openibl_amd import ops
from openibl_amd.lib import OpenIBLAmdError

pytestmark = pytest.mark.gpu

_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_golden("tuple_loss")
    return _cache["g"]


def rows(name, dev):
    """The case's compact rows on the device (leaves) and as numpy, once per session."""
    if name not in _cache:
        _cache[name] = ref.case_rows(name)
    return [torch.from_numpy(np.ascontiguousarray(t)).to(dev).requires_grad_(True) for t in _cache[name]]


def want(name, mode):
    if (name, mode) not in _cache:
        kind, score, margin, temp, _ = ref.MODES[mode]
        _cache[name, mode] = ref.tuple_loss(*ref.case_rows(name), kind, score, margin, temp)
    return _cache[name, mode]


def run(mode, a, p, n, scale=None):
    kind, score, margin, temp, _ = ref.MODES[mode]
    loss = ops.tuple_loss(a, p, n, kind, margin=margin, temp=temp, score=score)
    (loss if scale is None else scale * loss).backward()
    return loss.detach()


@pytest.mark.parametrize("mode", list(ref.MODES))
@pytest.mark.parametrize("name", list(ref.CASES))
def test_loss_and_gradients_against_float64(dev, name, mode):
    a, p, n = rows(name, dev)
    loss = run(mode, a, p, n)
    w_loss, *w_grads = want(name, mode)
    bars = 8.0 * golden()[f"{name}_{mode}_ref_err"]
    got = [abs(float(loss) - w_loss) / abs(w_loss)] + [ref.rel_max(t.grad.cpu().numpy(), w)
                                                       for t, w in zip((a, p, n), w_grads)]
    print(f"{name} {mode}: loss {float(loss):.9f} (float64 {w_loss:.12f}); loss | da | dp | dn "
          + " ".join(f"{e:.3e}" for e in got) + "; bars " + " ".join(f"{b:.3e}" for b in bars))
    assert loss.dtype == torch.float32 and loss.dim() == 0
    for k, e, b in zip(("loss", "da", "dp", "dn"), got, bars):
        assert e <= b, (name, mode, k, e, b)
    if ref.MODES[mode][0] == "triplet":                      # an inactive hinge leaves its negative at exactly zero
        h = ref.hinge_arguments(*ref.case_rows(name), ref.MODES[mode][2])
        assert np.array_equal((n.grad.abs().amax(-1) > 0).cpu().numpy(), h > 0)


@pytest.mark.parametrize("name", list(ref.SOFT_CASES))
def test_soft_label_loss_against_float64(dev, name):
    seed, B, J, ts, tt = ref.SOFT_CASES[name]
    s_np, t_np = ref.draw_soft(seed, B, J)
    s = torch.from_numpy(s_np).to(dev).requires_grad_(True)
    t = torch.from_numpy(t_np).to(dev).requires_grad_(True)
    loss = ops.soft_label_loss(s, t, ts, tt)
    loss.backward()
    w_loss, w_ds = ref.soft_label_loss(s_np, t_np, ts, tt)
    bars = 8.0 * golden()[f"soft_{name}_ref_err"]
    e_loss = abs(float(loss) - w_loss) / abs(w_loss) if w_loss != 0.0 else abs(float(loss))
    e_ds = ref.rel_max(s.grad.cpu().numpy(), w_ds)
    print(f"soft {name}: loss {float(loss):.9f} (float64 {w_loss:.12f}); loss | ds {e_loss:.3e} {e_ds:.3e}; bars "
          f"{bars[0]:.3e} {bars[1]:.3e}")
    assert e_loss <= bars[0] and e_ds <= bars[1]
    assert t.grad is None                                    # the teacher is a label
    first = s.grad.clone()
    s.grad = None
    (2.0 * ops.soft_label_loss(s, t, ts, tt)).backward()
    assert torch.equal(s.grad, 2.0 * first)
    assert torch.equal(ops.soft_label_loss(s, t, ts, tt).detach(), loss.detach())


@pytest.mark.parametrize("mode", list(ref.MODES))
def test_region_views_unreferenced_rows_and_two_runs(dev, mode):
    """The generation >= 1 layout: strided views of a [B][2 + M][9][L] tensor for the anchor and the positive, the
    negatives gathered by the argmax of the stored score.  Rows the loss does not read get exactly zero; strided
    inputs and contiguous copies give the same bits; two runs are bit-identical."""
    name = "b2m10l4096_regions"
    seed, B, M, L, _ = ref.CASES[name]
    vec_np, score_np = ref.draw_regions(seed, B, M, L)
    np.testing.assert_array_equal(score_np, golden()[f"{name}_score"])
    vec = torch.from_numpy(vec_np).to(dev).requires_grad_(True)
    arg = torch.from_numpy(score_np).to(dev).argmax(-1)
    assert np.array_equal(arg.cpu().numpy(), ref.select_regions(vec_np, score_np)[3])

    def through_views():
        vec.grad = None
        anchors, positives = vec[:, 0, 0], vec[:, 1, 0]
        select = torch.gather(vec[:, 2:], 2, arg.view(B, M, 1, 1).expand(B, M, 1, L))[:, :, 0]
        assert not anchors.is_contiguous() and anchors.stride(0) == (2 + M) * 9 * L
        loss = run(mode, anchors, positives, select)
        return loss, vec.grad.clone()

    loss, g = through_views()
    a, p, n = rows(name, dev)
    loss_c = run(mode, a, p, n)
    assert torch.equal(loss, loss_c)
    used = torch.zeros((B, 2 + M, 9), dtype=torch.bool, device=dev)
    used[:, :2, 0] = True
    used[torch.arange(B, device=dev)[:, None], 2 + torch.arange(M, device=dev)[None, :], arg] = True
    assert float(g[~used].abs().max()) == 0.0
    assert torch.equal(g[:, 0, 0], a.grad) and torch.equal(g[:, 1, 0], p.grad)
    assert torch.equal(g[torch.arange(B, device=dev)[:, None], 2 + torch.arange(M, device=dev)[None, :], arg], n.grad)
    loss2, g2 = through_views()
    assert torch.equal(loss2, loss) and torch.equal(g2, g)

    # the generation-0 layout: region 0 of every row, all three inputs strided (negatives: row stride 9 L)
    vec.grad = None
    loss_v = run(mode, vec[:, 0, 0], vec[:, 1, 0], vec[:, 2:, 0])
    gv = vec.grad.clone()
    c = [t.detach().clone().contiguous().requires_grad_(True) for t in (vec[:, 0, 0], vec[:, 1, 0], vec[:, 2:, 0])]
    assert torch.equal(run(mode, *c), loss_v)
    assert torch.equal(gv[:, 0, 0], c[0].grad) and torch.equal(gv[:, 1, 0], c[1].grad) and torch.equal(gv[:, 2:, 0], c[2].grad)
    assert float(gv[:, :, 1:].abs().max()) == 0.0


@pytest.mark.parametrize("mode", list(ref.MODES))
def test_unaligned_rows_give_the_bits_of_aligned_ones(dev, mode):
    """L = 1000 rows at an odd element offset (4-byte loads) against the aligned copies (16-byte loads), and L = 1001:
    a last group of one column."""
    name = "b2m3l1000"
    a, p, n = rows(name, dev)
    loss = run(mode, a, p, n)
    B, M, L = n.shape
    flat = torch.zeros(B * (2 + M) * L + 1, device=dev)
    flat[1:] = torch.cat((a.detach()[:, None], p.detach()[:, None], n.detach()), dim=1).reshape(-1)
    x = flat[1:].view(B, 2 + M, L).requires_grad_(True)
    assert x.data_ptr() % 16 == 4
    assert torch.equal(run(mode, x[:, 0], x[:, 1], x[:, 2:]), loss)
    assert torch.equal(x.grad[:, 0], a.grad) and torch.equal(x.grad[:, 1], p.grad) and torch.equal(x.grad[:, 2:], n.grad)
    # one more column: the float64 formulas again
    rows_np = ref.draw_rows(ref.CASES[name][0] + 50, B, M, L + 1)
    y = torch.from_numpy(rows_np).to(dev).requires_grad_(True)
    loss1 = run(mode, y[:, 0], y[:, 1], y[:, 2:])
    kind, score, margin, temp, _ = ref.MODES[mode]
    w = ref.tuple_loss(rows_np[:, 0], rows_np[:, 1], rows_np[:, 2:], kind, score, margin, temp)
    bars = 8.0 * golden()[f"{name}_{mode}_ref_err"]
    got = y.grad.cpu().numpy()
    assert abs(float(loss1) - w[0]) <= max(bars[0], 2.0 ** -24) * abs(w[0])
    for k, (g_, w_) in enumerate(((got[:, 0], w[1]), (got[:, 1], w[2]), (got[:, 2:], w[3]))):
        assert ref.rel_max(g_, w_) <= bars[1 + k], (mode, k)


def _ulp_apart(x, y):
    """|x - y| in units of the fp32 spacing at max(|x|, |y|), elementwise maximum."""
    x64, y64 = x.double(), y.double()
    big = torch.maximum(x.abs(), y.abs())
    spacing = (torch.nextafter(big, torch.full_like(big, float("inf"))) - big).double()
    return float(((x64 - y64).abs() / spacing).max())


@pytest.mark.parametrize("mode", list(ref.MODES))
def test_a_tuple_depends_on_its_batch_mates_through_the_count_only(dev, mode):
    """Tuple 0 of the batch of 3 against tuple 0 alone: the gradients times the count ratio 3 (computed in fp32) within
    1 ulp in every mode — 3 is no power of two, so one more rounding separates the two — and, where the ratio is a
    power of two (tuples 0..1 as a batch of 2 against tuple 0 alone; tuples 0..1 against 0..1 twice as a batch of 4),
    to the last bit in every mode."""
    a, p, n = rows("b3m10l32768", dev)
    run(mode, a, p, n)

    def sub(idx):
        t = [v.detach()[idx].clone().requires_grad_(True) for v in (a, p, n)]
        run(mode, *t)
        return t

    one = sub([0])
    for whole, alone in zip((a, p, n), one):
        d = _ulp_apart(whole.grad[:1] * 3.0, alone.grad)
        assert d <= 1.0, (mode, d)
    two = sub([0, 1])
    four = sub([0, 1, 0, 1])
    for t2, t1, t4 in zip(two, one, four):
        assert torch.equal(t2.grad[:1] * 2.0, t1.grad), mode
        assert torch.equal(t4.grad[:2] * 2.0, t2.grad) and torch.equal(t4.grad[2:], t4.grad[:2]), mode


def test_needs_input_grad_and_the_upstream_scalar(dev):
    a, p, n = rows("b2m3l1000", dev)
    for mode in ref.MODES:
        for t in (a, p, n):
            t.grad = None
        run(mode, a, p, n)
        full = [t.grad.clone() for t in (a, p, n)]
        for t in (a, p, n):
            t.grad = None
        run(mode, a, p, n, scale=2.0)
        for t, f in zip((a, p, n), full):
            assert torch.equal(t.grad, 2.0 * f), mode
        # one input at a time: the same bits, nothing for the others
        for i in range(3):
            ins = [t.detach().clone().requires_grad_(j == i) for j, t in enumerate((a, p, n))]
            run(mode, *ins)
            for j, t in enumerate(ins):
                assert (t.grad is None) if j != i else torch.equal(t.grad, full[i]), (mode, i, j)
    # nothing wanted: the backward launches nothing and hands out None
    ins = [t.detach() for t in (a, p, n)]
    loss, coef = ops.tuple_loss_forward(*ins, "triplet")
    assert not ops.tuple_loss(*ins, "triplet").requires_grad and coef.dtype == torch.float64
    assert ops._TupleLoss.backward(type("Ctx", (), {"saved_tensors": (*ins, coef), "needs_input_grad": (False,) * 7,
                                                    "kind": "triplet", "score": "sqdist"})(), loss) == (None,) * 7


def test_arguments_outside_the_limits_raise_and_launch_nothing(dev):
    z = lambda *s: torch.zeros(s, device=dev)                                                     # noqa: E731
    with pytest.raises(ValueError, match=r"\(2, 8\).*\(2, 65, 8\)"):
        ops.tuple_loss(z(2, 8), z(2, 8), z(2, 65, 8), "triplet")
    with pytest.raises(ValueError, match="negatives"):
        ops.tuple_loss(z(2, 8), z(2, 8), z(2, 0, 8), "triplet")
    with pytest.raises(ValueError, match=r"\(3, 8\)"):
        ops.tuple_loss(z(2, 8), z(3, 8), z(2, 3, 8), "sare_ind")
    with pytest.raises(ValueError, match="contiguous"):
        ops.tuple_loss(z(2, 16)[:, ::2], z(2, 8), z(2, 3, 8), "sare_ind")
    with pytest.raises(ValueError, match="float32"):
        ops.tuple_loss(z(2, 8).double(), z(2, 8), z(2, 3, 8), "sare_ind")
    with pytest.raises(ValueError, match="unknown loss"):
        ops.tuple_loss(z(2, 8), z(2, 8), z(2, 3, 8), "hinge")
    with pytest.raises(ValueError, match=r"\(2, 4097\)"):
        ops.soft_label_loss(z(2, 4097), z(2, 4097), 0.07, 0.07)
    with pytest.raises(ValueError, match="positive"):
        ops.soft_label_loss(z(2, 9), z(2, 9), 0.0, 0.07)
    with pytest.raises(ValueError, match=r"\(2, 9\).*\(2, 8\)"):
        ops.soft_label_loss(z(2, 9), z(2, 8), 0.07, 0.07)
    # the C entry point itself: an error status, no launch (a launch on the null stream with these arguments would fault)
    from openibl_amd import lib
    h = lib.load()
    t = z(2, 8)
    rc = h.oibl_tuple_loss_forward(t.data_ptr(), 8, t.data_ptr(), 8, t.data_ptr(), 8, 8, 2, 65, 8, 0, 0, 0.3, 0.07,
                                   t.data_ptr(), t.data_ptr(), t.data_ptr(), 0, None)
    assert rc == -1 and b"64" in h.oibl_last_error()
    with pytest.raises(OpenIBLAmdError):
        lib.check(rc, "tuple_loss_forward")
    torch.cuda.synchronize()
