"""Gradients of the SFRS region head on the device (csrc/region_backward.hip; ops.region_vlad_backward /
region_scores_backward / region_vlad_train / region_scores_train; EmbedRegionNet.forward_train) against the numpy
float64 evaluation of the same formulas (tests/helpers/region_grad_ref.py), which tests/test_region_backward_cpu.py ties
to the reference's own autograd (tests/golden/region_backward.npz).

Bars, per gradient: 8 x the rel-L2 error of the REFERENCE's fp32 autograd against its own float64 run on the golden of
the same regime and mode, as tests/helpers/make_region_backward_golden.py stored it (`ref_err`), never above 1e-4.  A
shape without a golden takes its regime's bars.
                                                  dW        dC        dX
  reference, trained 3x(4x6), normalised          8.44e-7   1.70e-7   2.42e-7   -> bars 6.75e-6  1.36e-6  1.94e-6
  reference, raw 3x(4x6)                          3.02e-6   4.33e-7   2.86e-6   -> bars 2.42e-5  3.47e-6  2.29e-5
  reference, tuple 1x4x(8x8), SFRS gen-0 loss     2.51e-6   2.84e-6   2.12e-6   -> bars 2.01e-5  2.28e-5  1.70e-5
  reference, end to end: dW1..3 3.34e-6 3.77e-6 4.55e-6, db1..3 3.00e-6 3.52e-6 2.99e-6, dWv 4.76e-6, dCv 4.32e-6
  reference, scores' backward (fp32 bmm): 5.7e-8 .. 7.1e-8                      -> bars 4.6e-7 .. 5.7e-7
The kernels' measured errors, also in DESIGN §4.5 — dW | dC | dX against float64, MI355X:
  goldens: trained 3.34e-7 | 4.41e-8 | 2.81e-7, raw 7.14e-7 | 7.30e-8 | 6.82e-7, tuple 6.17e-7 | 1.84e-6 | 5.33e-7
    (forward Y 1.8e-7, 6.2e-7, 4.2e-7; against the reference's fp32 numbers 9.3e-7 | 1.7e-7 | 4.2e-7, 3.1e-6 | 4.3e-7 |
    2.8e-6, 2.6e-6 | 3.3e-6 | 2.2e-6)
  trained: 2x(2x2) 3.83e-7 | 3.94e-8 | 2.72e-7, 1x(2x4) 1.78e-6 | 9.55e-7 | 1.20e-6, 2x(4x6) 4.25e-7 | 3.61e-8 | 2.81e-7,
    1x(2x62) 1.01e-6 | 3.01e-7 | 3.32e-7, 2x(8x16) 5.75e-7 | 4.86e-8 | 2.47e-7, 1x(6x22) 8.95e-7 | 2.51e-7 | 3.11e-7,
    1x(16x16) 7.78e-7 | 9.80e-8 | 2.64e-7, 1x(10x26) 7.75e-7 | 1.04e-7 | 2.53e-7, 2x(30x40) 1.26e-6 | 9.85e-8 | 2.80e-7
  raw: 2x(4x6) 6.60e-7 | 5.90e-8 | 6.24e-7, 1x(6x22) 5.66e-7 | 6.01e-8 | 5.30e-7, 1x(10x26) 5.95e-7 | 5.68e-8 | 5.42e-7
  one region alone, dX: 4x6 region 5 2.76e-7, region 1 2.67e-7; 6x22 2.61e-7, 2.55e-7
  region 0 alone against ops.netvlad_backward: 7.99e-7 | 8.79e-8 | 1.22e-7
  17x(4x6) 4.52e-7 | 3.62e-8 | 2.93e-7; all-zero pixel: its row 2.38e-7, the others 3.64e-7 | 3.73e-8 | 2.82e-7;
    all-zero quarter, the other rows 1.28e-6 | 8.49e-7 | 6.69e-7
  scores' backward: 2.53e-8 at every (T, n)
  end to end: dW1..3 6.62e-6 8.17e-6 9.55e-6, db1..3 7.79e-6 8.08e-6 5.38e-6, dWv 1.08e-5, dCv 1.37e-5
    (bars 2.67e-5 3.01e-5 3.64e-5, 2.40e-5 2.82e-5 2.39e-5, 3.80e-5, 3.46e-5); loss_hard 0.276596129 (float64
    0.276596056), loss_soft 2.452647686 (2.452647680); a bf16 backbone: scores 3.4e-4, vectors 5.5e-3

Map shapes (pixels per quarter in brackets; a chunk is 32 pixels of one quarter): 2x2 [1], 2x4 [2], 4x6 [6, odd quarter
width], 2x62 [31, quarter height 1], 8x16 [32], 6x22 [33], 16x16 [64], 10x26 [65], 30x40 [300, the workload's].  The
decomposition has no other edge: chunks never cross a quarter, the dW pass walks all pixels of the image in chunks of
32 (4 Pq: 4, 8, 24, 124, 128, 132, 256, 260, 1200 — below, at and above multiples of 32)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from helpers import netvlad_grad_ref as nref
from helpers import region_grad_ref as ref
from openibl_amd import ops, synth

pytestmark = pytest.mark.gpu

K, C, L = 64, 512, 64 * 512
GOLDENS = {"trained": "trained_3x4x6", "raw": "raw_3x4x6", "tuple": "tuple_1x4x8x8"}
KEYS = ("dW", "dC", "dX")
SHAPES = [(2, 2, 2), (1, 2, 4), (2, 4, 6), (1, 2, 62), (2, 8, 16), (1, 6, 22), (1, 16, 16), (1, 10, 26), (2, 30, 40)]
RAW_SHAPES = [(2, 4, 6), (1, 6, 22), (1, 10, 26)]
_cache = {}


def golden():
    if "golden" not in _cache:
        _cache["golden"] = load_golden("region_backward")
    return _cache["golden"]


def bars(regime):
    e = golden()[f"{GOLDENS[regime]}_ref_err"]
    return {k: min(8.0 * float(v), 1e-4) for k, v in zip(KEYS, e)}


def case(regime, seed, N, h, w_, clear=None):
    """Inputs (numpy fp32: x, w, c, G [N][9][K*C]) and the float64 gradients of a case, once per session.  `clear`: a
    tuple of index tuples into x set to zero before anything is computed."""
    key = (regime, seed, N, h, w_, repr(clear))
    if key not in _cache:
        if regime == "trained":
            x, w, c, _, _ = nref.draw_trained_inputs(seed, N, h, w_)
        else:
            x, w, c, _ = nref.draw_inputs(seed, N, h, w_)
        for idx in clear or ():
            x[idx] = 0.0
        G = np.random.RandomState(seed + 100).randn(N, 9, K * C).astype(np.float32)
        _cache[key] = ((x, w, c, G), ref.head_and_grads(x, w, c, G, regime == "trained"))
    return _cache[key]


def golden_case(regime):
    """The golden of a regime regenerated from its seed: (x, w, c, G, Gs, normalize), float64 results (of the fp32 G
    and Gs the device is given)."""
    if ("golden", regime) not in _cache:
        _cache[("golden", regime)] = ref.golden_head_case(GOLDENS[regime], golden())
    return _cache[("golden", regime)]


def run(dev, inputs, normalize, want=("w", "c", "x")):
    x, w, c, G = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in inputs)
    return ops.region_vlad_backward(x, w, c, G, normalize_input=normalize, want=want)


def check(name, got, want, regime, keys=KEYS):
    bar = bars(regime)
    errs = {}
    for k, g in zip(KEYS, got):
        if k in keys:
            assert g.dtype == torch.float32 and tuple(g.shape) == want[k].shape
            assert torch.isfinite(g).all(), (name, k)
            errs[k] = ref.rel_l2(g.cpu().numpy(), want[k])
    print(name, " ".join(f"{k} {v:.3e} (bar {bar[k]:.2e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bar[k], (name, k, v, bar[k])


# ---- accuracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["trained", "raw", "tuple"])
def test_golden_cases_through_the_c_abi(dev, regime):
    """forward, scores' backward, head's backward as three calls: dY = G + region_scores_backward(Y, Gs)."""
    g, name = golden(), GOLDENS[regime]
    (x, w, c, G, Gs, normalize), want = golden_case(regime)
    N, h, w_, _ = x.shape
    xt, wt, ct, Gt, Gst = (torch.from_numpy(t).to(dev) for t in (x, w, c, G, Gs))
    Y = ops.region_vlad(xt, wt, ct, normalize)
    score = ops.region_scores(Y, 1)
    ey, es = ref.rel_l2(Y.cpu().numpy(), want["Y"]), ref.rel_l2(score.cpu().numpy(), want["score"])
    dY = Gt + ops.region_scores_backward(Y, Gst, 1)
    edy = ref.rel_l2(dY.cpu().numpy(), want["dY"])
    print(f"{name}: forward Y {ey:.3e} score {es:.3e}, dY {edy:.3e}")
    assert ey <= 5e-6 and es <= 5e-6
    got = ops.region_vlad_backward(xt, wt, ct, dY.contiguous(), normalize_input=normalize)
    check(name, got, want, regime)
    # and against the reference's own numbers: the kernel and the reference are each inside their bar of float64
    bar, ref_err = bars(regime), dict(zip(KEYS, g[f"{name}_ref_err"]))
    hs, dxs = int(g[f"{name}_head_stride"]), int(g[f"{name}_dx_stride"])
    parts = {"dW": got[0].cpu().numpy().ravel()[::hs], "dC": got[1].cpu().numpy().ravel()[::hs],
             "dX": got[2].cpu().numpy().reshape(N, h * w_, C)[:, ::dxs]}
    for k in KEYS:
        e = ref.rel_l2(parts[k], g[f"{name}_{k}"])
        print(f"  {k} against the reference's fp32 autograd: {e:.3e}")
        assert e <= bar[k] + float(ref_err[k]), (k, e)


@pytest.mark.parametrize("N,h,w_", SHAPES)
def test_chunk_and_quarter_edges_trained(dev, N, h, w_):
    inputs, want = case("trained", 300 + h + w_, N, h, w_)
    check(f"trained {N}x({h}x{w_})", run(dev, inputs, True), want, "trained")


@pytest.mark.parametrize("N,h,w_", RAW_SHAPES)
def test_chunk_and_quarter_edges_raw(dev, N, h, w_):
    inputs, want = case("raw", 400 + h + w_, N, h, w_)
    check(f"raw {N}x({h}x{w_})", run(dev, inputs, False), want, "raw")


@pytest.mark.parametrize("h,w_", [(4, 6), (6, 22)])
def test_addressing_a_region_reaches_its_quarters_only(dev, h, w_):
    """G non-zero in region 5 (q0) alone: grad_feat is exactly 0.0 outside the top-left quarter; in region 1 (the top
    half) alone: exactly 0.0 in the bottom half — and not zero inside."""
    (x, w, c, G), _ = case("trained", 300 + h + w_, 2 if (h, w_) == (4, 6) else 1, h, w_)
    for region, inside in ((5, (slice(0, h // 2), slice(0, w_ // 2))), (1, (slice(0, h // 2), slice(0, w_)))):
        G1 = np.zeros_like(G)
        G1[:, region] = G[:, region]
        gx = run(dev, (x, w, c, G1), True, want=("x",))[2].cpu().numpy()
        mask = np.zeros((h, w_), dtype=bool)
        mask[inside] = True
        assert np.all(gx[:, ~mask] == 0.0), region
        assert np.all(np.abs(gx[:, mask]).max(-1) > 0.0), region
        want = ref.head_and_grads(x, w, c, G1, True)
        check(f"{h}x{w_} region {region} alone", (None, None, torch.from_numpy(gx)), want, "trained", keys=("dX",))


def test_region_zero_is_the_merged_head(dev):
    """G non-zero in region 0 alone: the whole image's NetVLAD — ops.netvlad_backward of G[:, 0], within the sum of
    both kernels' bars (the merged head's: 8 x its trained golden's ref_err)."""
    (x, w, c, G), _ = case("trained", 300 + 8 + 16, 2, 8, 16)
    G0 = np.zeros_like(G)
    G0[:, 0] = G[:, 0]
    got = run(dev, (x, w, c, G0), True)
    xt, wt, ct = (torch.from_numpy(t).to(dev) for t in (x, w, c))
    plain = ops.netvlad_backward(xt, wt, ct, torch.from_numpy(np.ascontiguousarray(G[:, 0])).to(dev))
    e = load_golden("netvlad_backward_trained_2x12x16")["ref_err"]
    mine = bars("trained")
    for k, a, b, ev in zip(KEYS, got, plain, e):
        err = ref.rel_l2(a.cpu().numpy(), b.cpu().numpy())
        both = mine[k] + min(8.0 * float(ev), 1e-4)
        print(f"region 0 alone against netvlad_backward: {k} {err:.3e} (sum of the bars {both:.2e})")
        assert err <= both, k


# ---- determinism, independence of outputs -------------------------------------------------------------------------
def test_each_output_alone_equals_the_full_call_and_two_runs_are_bit_identical(dev):
    inputs, _ = case("trained", 300 + 10 + 26, 1, 10, 26)
    full = run(dev, inputs, True)
    for i, letter in enumerate(("w", "c", "x")):
        alone = run(dev, inputs, True, want=(letter,))
        assert [t is None for t in alone] == [j != i for j in range(3)]
        assert torch.equal(alone[i], full[i]), letter
    pair = run(dev, inputs, True, want=("w", "c"))
    assert pair[2] is None and torch.equal(pair[0], full[0]) and torch.equal(pair[1], full[1])
    big, _ = case("trained", 300 + 30 + 40, 2, 30, 40)
    a, b = run(dev, big, True), run(dev, big, True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_batch_mates_seventeen_images_and_a_zero_gradient(dev):
    x, w, c, _, _ = nref.draw_trained_inputs(501, 17, 4, 6)
    G = np.random.RandomState(502).randn(17, 9, K * C).astype(np.float32)
    G[3] = 0.0
    gw, gc, gx = run(dev, (x, w, c, G), True)
    assert torch.isfinite(gw).all() and torch.isfinite(gc).all() and torch.isfinite(gx).all()
    assert float(gx[3].abs().max()) == 0.0 and float(gx[2].abs().max()) > 0.0
    for lo, hi in ((7, 8), (5, 10)):                 # alone, and inside a batch of 5
        part = run(dev, (x[lo:hi], w, c, G[lo:hi]), True, want=("x",))[2]
        assert torch.equal(part, gx[lo:hi]), (lo, hi)
    want = ref.head_and_grads(x, w, c, G, True)
    check("17x(4x6)", (gw, gc, gx), want, "trained")


def test_degenerate_pixels_are_finite(dev):
    """An all-zero pixel (its row is dxh / eps: compared apart) and a quarter of all-zero pixels."""
    inputs, want = case("trained", 611, 2, 4, 6, clear=((1, 1, 2),))
    gw, gc, gx = run(dev, inputs, True)
    assert torch.isfinite(gx).all()
    got, w64 = gx.cpu().numpy().copy(), want["dX"].copy()
    e_row = ref.rel_l2(got[1, 1, 2], w64[1, 1, 2])
    got[1, 1, 2] = 0.0
    w64[1, 1, 2] = 0.0
    print(f"all-zero pixel: its row {e_row:.3e}")
    assert e_row <= bars("trained")["dX"]
    check("all-zero pixel, the other rows", (gw, gc, torch.from_numpy(got)), dict(want, dX=w64), "trained")
    inputs, want = case("trained", 612, 1, 4, 6, clear=((0, slice(2, 4), slice(3, 6)),))
    gw, gc, gx = run(dev, inputs, True)
    assert torch.isfinite(gw).all() and torch.isfinite(gc).all() and torch.isfinite(gx).all()
    got, w64 = gx.cpu().numpy().copy(), want["dX"].copy()
    got[0, 2:4, 3:6] = 0.0
    w64[0, 2:4, 3:6] = 0.0
    check("all-zero quarter, the other rows", (gw, gc, torch.from_numpy(got)), dict(want, dX=w64), "trained")


# ---- the scores' backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(4))
def test_region_scores_backward(dev, i):
    g = golden()
    seed, T, n = map(int, g["scores_cases"][i])
    bar = min(8.0 * float(g["scores_ref_err"][i]), 1e-4)
    Y, Gs = ref.draw_vectors(seed, T, n)
    want = ref.scores_backward(Y, Gs, T)
    Yt, Gst = torch.from_numpy(Y).to(dev), torch.from_numpy(Gs).to(dev)
    got = ops.region_scores_backward(Yt, Gst, T)
    e = ref.rel_l2(got.cpu().numpy(), want)
    print(f"scores' backward T={T} n={n}: {e:.3e} (bar {bar:.2e})")
    assert got.dtype == torch.float32 and tuple(got.shape) == Y.shape and e <= bar
    assert torch.equal(got, ops.region_scores_backward(Yt, Gst, T))
    if n > 1:
        # pair 1 with the anchor alone: the pair's rows are the same bits
        v = Yt.view(T, 1 + n, 9, L)
        two = torch.cat([v[:, :1], v[:, 2:3]], dim=1).reshape(T * 2, 9, L).contiguous()
        alone = ops.region_scores_backward(two, Gst[:, 1:2].contiguous(), T)
        assert torch.equal(alone.view(T, 2, 9, L)[:, 1], got.view(T, 1 + n, 9, L)[:, 2])


# ---- autograd functions -------------------------------------------------------------------------------------------
def test_autograd_functions(dev, monkeypatch):
    (x, w, c, G, Gs, normalize), want = golden_case("trained")
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    wt = torch.from_numpy(w).to(dev).reshape(K, C, 1, 1).requires_grad_(True)        # conv.weight's shape
    ct = torch.from_numpy(c).to(dev).requires_grad_(True)
    Gt, Gst = torch.from_numpy(G).to(dev), torch.from_numpy(Gs).to(dev)
    vec = ops.region_vlad_train(xt, wt, ct, True)
    score = ops.region_scores_train(vec, 1)
    assert torch.equal(vec, ops.region_vlad(xt.detach(), wt.detach(), ct.detach(), True))
    assert torch.equal(score, ops.region_scores(vec.detach(), 1))
    ((vec * Gt).sum() + (score * Gst).sum()).backward()           # both uses of vec: autograd adds the two gradients
    assert tuple(wt.grad.shape) == (K, C, 1, 1)
    check("autograd, the trained golden", (wt.grad.reshape(K, C), ct.grad, xt.grad), want, "trained")
    first = (wt.grad.clone(), ct.grad.clone())

    # a frozen parameter gets none and its stage is not asked for
    asked = []
    real = ops.region_vlad_backward

    def spy(*args, **kwargs):
        asked.append(tuple(kwargs["want"]))
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "region_vlad_backward", spy)
    x2 = torch.from_numpy(x).to(dev)
    w2 = wt.detach().clone().requires_grad_(True)
    c2 = ct.detach().clone()
    vec = ops.region_vlad_train(x2, w2, c2, True)
    ((vec * Gt).sum() + (ops.region_scores_train(vec, 1) * Gst).sum()).backward()
    assert asked == [("w",)] and c2.grad is None and torch.equal(w2.grad, first[0])
    c3 = ct.detach().clone().requires_grad_(True)
    vec = ops.region_vlad_train(x2, w2.detach(), c3, True)
    ((vec * Gt).sum() + (ops.region_scores_train(vec, 1) * Gst).sum()).backward()
    assert asked[-1] == ("c",) and torch.equal(c3.grad, first[1])
    # nothing requires a gradient: no graph
    assert not ops.region_vlad_train(x2, w2.detach(), c2, True).requires_grad
    # a bf16 map is widened
    vb = ops.region_vlad_train(x2.bfloat16(), w2.detach(), c2, True)
    assert vb.dtype == torch.float32 and torch.equal(vb, ops.region_vlad(x2.bfloat16(), w2.detach(), c2, True))


# ---- EmbedRegionNet.forward_train -----------------------------------------------------------------------------------
def _make(state_dict, dev, tuple_size=1, precision="fp32"):
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    m = models.create("embedregionnet", base, pool, tuple_size=tuple_size)
    m.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    return m.to(dev).eval().set_precision(precision)


@pytest.mark.parametrize("precision", ["fp32", "f16mx", "bf16x3"])
def test_forward_train_frozen_backbone_is_bit_equal_to_region_similarity(dev, state_dict, precision):
    model = _make(state_dict, dev, 2, precision)
    if precision == "f16mx":
        model.base_model.F16MX_MIN_TILES = 0
    x = synth.images(6, 64, 96, seed=91).to(dev)
    want = model.region_similarity(x)
    model.train()
    got = model.forward_train(x)
    for a, b in zip(got, want):
        assert a.requires_grad and a.shape == b.shape and torch.equal(a.detach(), b)
    assert tuple(got[0].shape) == (2, 2, 9, 9) and tuple(got[1].shape) == (2, 1, 9, L) and tuple(got[2].shape) == (2, 2, 9, L)
    (got[0].sum() + got[1][:, 0, 3].sum() + got[2][:, 1, 7].sum()).backward()
    with_grad = sorted(n for n, p in model.named_parameters() if p.grad is not None)
    assert with_grad == ["net_vlad.centroids", "net_vlad.conv.weight"], with_grad


def test_forward_train_from_a_bf16_model_and_one_sgd_step(dev, state_dict):
    x = synth.images(3, 64, 96, seed=92).to(dev)
    exact = _make(state_dict, dev, 1, "fp32").region_similarity(x)
    model = _make(state_dict, dev, 1, "bf16")
    got = model.forward_train(x)
    for a, b in zip(got, exact):
        assert torch.isfinite(a).all()
        e = ref.rel_l2(a.detach().cpu().numpy(), b.cpu().numpy())
        print(f"bf16 backbone: {tuple(a.shape)} against the fp32 model {e:.3e}")
        assert e <= 5e-2
    model = _make(state_dict, dev, 1, "fp32")
    before = model.region_similarity(x)[0].clone()
    score, va, vb = model.forward_train(x)
    loss = (score[:, :, 0] ** 2).sum() + ((va[:, 0, 0] - vb[:, 0, 0]) ** 2).sum()
    loss.backward()
    torch.optim.SGD(model.net_vlad.parameters(), lr=1e-2).step()
    after = model.region_similarity(x)[0]
    assert not torch.equal(after, before)


def sfrs_losses(model, cache, easy, diff, neg_num, margin=0.1 ** 0.5, temp=0.07, train_layers="conv5"):
    """SFRSTrainer._forward at generation 0 (ibl/trainers.py:235-259) with Trainer's triplet (:275-280), one tuple
    per row of the batch."""
    B = easy.shape[0] // (neg_num + 2)
    sim_easy, vlad_anchors, vlad_pairs = model.forward_train(easy, train_layers=train_layers)
    with torch.no_grad():
        sim_diff_label, _, _ = cache.region_similarity(diff)
    sim_diff, _, _ = model.forward_train(diff, train_layers=train_layers)
    anchors, positives, negatives = vlad_anchors[:, 0, 0], vlad_pairs[:, 0, 0], vlad_pairs[:, 1:, 0]
    a = anchors.unsqueeze(1).expand_as(negatives).reshape(-1, L)
    p = positives.unsqueeze(1).expand_as(negatives).reshape(-1, L)
    loss_hard = F.triplet_margin_loss(a, p, negatives.reshape(-1, L), margin=margin, p=2, reduction="mean")
    log_sim_diff = F.log_softmax(sim_diff[:, :, 0].reshape(B, -1) / temp, dim=1)
    label = F.softmax(sim_diff_label[:, :, 0].reshape(B, -1) / temp, dim=1).detach()
    loss_soft = (-label * log_sim_diff).mean(0).sum()
    return loss_hard, loss_soft


def test_forward_train_conv5_one_sfrs_step_against_the_reference(dev, state_dict):
    g = golden()
    n_img, H, W, neg_num = map(int, g["e2e_shape"])
    images = synth.images(n_img, H, W, seed=int(g["e2e_seed"])).to(dev)
    model = _make(state_dict, dev, 1, "fp32").train()
    cache = _make(state_dict, dev, 1, "fp32").train()            # generation 0: model_cache is a copy of the student
    easy, diff = images[:neg_num + 2], torch.cat([images[:1], images[neg_num + 2:]], dim=0)
    loss_hard, loss_soft = sfrs_losses(model, cache, easy, diff, neg_num)
    (loss_hard + 0.5 * loss_soft).backward()
    want_h, want_s = map(float, g["e2e64_losses"])
    got_h, got_s = float(loss_hard.detach()), float(loss_soft.detach())
    print(f"loss_hard {got_h:.9f} (float64 {want_h:.9f}), loss_soft {got_s:.9f} (float64 {want_s:.9f})")
    assert abs(got_h - want_h) <= 1e-5 * want_h and abs(got_s - want_s) <= 1e-5 * want_s
    b, nv = model.base_model.base, model.net_vlad
    got = {"dWv": nv.conv.weight.grad.reshape(K, C), "dCv": nv.centroids.grad}
    for i, li in enumerate((24, 26, 28)):
        got[f"dW{i + 1}"], got[f"db{i + 1}"] = b[li].weight.grad, b[li].bias.grad
    trunk = [p for i in range(24) for p in b[i].parameters()]
    assert len(trunk) == 20 and all(p.grad is None for p in trunk)
    keys = ("dW1", "dW2", "dW3", "db1", "db2", "db3", "dWv", "dCv")
    ref_err = dict(zip(keys, g["e2e_ref_err"]))
    rows, hs = int(g["e2e_w_rows"]), int(g["e2e_head_stride"])
    for k in keys:
        t = got[k].cpu().numpy()
        assert np.isfinite(t).all(), k
        part = t[:rows] if k.startswith("dW") and k != "dWv" else t[::hs] if k in ("dWv", "dCv") else t
        bar = min(8.0 * float(ref_err[k]), 1e-4)
        e64, e32 = ref.rel_l2(part, g[f"e2e64_{k}"]), ref.rel_l2(part, g[f"e2e_{k}"])
        print(f"  {k} {e64:.3e} (bar {bar:.2e}); against the reference's fp32 autograd {e32:.3e}")
        assert e64 <= bar, (k, e64, bar)
        assert e32 <= bar + float(ref_err[k]), (k, e32)
    for layers in ("conv4", "conv3", "conv2", "full"):
        with pytest.raises(NotImplementedError, match="pool4"):
            model.forward_train(easy, train_layers=layers)
    with pytest.raises(ValueError, match="unknown train_layers"):
        model.forward_train(easy, train_layers="conv6")
    with pytest.raises(NotImplementedError):
        model(easy)                                              # forward() in train() still raises


def test_forward_train_input_errors(dev, state_dict):
    m2 = _make(state_dict, dev, 2)
    with pytest.raises(ValueError, match="multiple of tuple_size"):
        m2.forward_train(synth.images(3, 64, 96, seed=13).to(dev))
    with pytest.raises(ValueError, match="2 x 3"):
        m2.forward_train(synth.images(4, 32, 48, seed=13).to(dev))
    with pytest.raises(ValueError, match="2 x 3"):
        m2.forward_train(synth.images(4, 32, 48, seed=13).to(dev), train_layers="conv5")
    w, c = m2.net_vlad._params()
    with pytest.raises(ValueError, match="5 x 6"):
        ops.region_vlad_backward(torch.zeros((1, 5, 6, C), device=dev), w, c, torch.zeros((1, 9, L), device=dev))
    with pytest.raises(ValueError, match="want"):
        ops.region_vlad_backward(torch.zeros((1, 4, 6, C), device=dev), w, c, torch.zeros((1, 9, L), device=dev), want=())
    with pytest.raises(ValueError):
        ops.region_scores_backward(torch.zeros((3, 9, L), device=dev), torch.zeros((1, 1, 9, 9), device=dev), 1)
