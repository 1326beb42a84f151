"""SFRS region similarities on the device (EmbedRegionNet.region_similarity, ops.region_vlad / region_scores,
csrc/region.hip) against vectors the REFERENCE ITSELF produced in training mode (tests/golden/region_*.npz) and,
at sizes without a fixture, against the fp64 comparator that tests/test_region_golden_cpu.py ties to those vectors.

Bounds: every (image, region) vector within the project's 1e-4 rel-L2; every score within 2.1e-4 absolute — for unit
vectors each within eps of their targets |delta score| <= 2 eps + eps^2, eps = 1e-4."""
import pytest
import torch

from conftest import load_golden
from helpers import region_ref
from openibl_amd import ops, synth

pytestmark = pytest.mark.gpu

TOL_VEC = 1e-4
TOL_SCORE = 2.1e-4
L = 64 * 512


def _make(state_dict, dev, tuple_size=1, precision="fp32", kind="embedregionnet"):
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    m = models.create(kind, base, pool, tuple_size=tuple_size) if kind == "embedregionnet" else \
        models.create(kind, base, pool)
    m.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    return m.to(dev).eval().set_precision(precision)


def _worst_vec(name, got, want):
    """max over (image, region) of the rel-L2 of [..., 9, cols] vectors."""
    got, want = got.double().cpu().reshape(-1, want.shape[-1]), want.double().cpu().reshape(-1, want.shape[-1])
    worst = float(((got - want).norm(dim=1) / want.norm(dim=1)).max())
    print(f"{name}: worst (image, region) vector rel-L2 {worst:.3e} over {got.shape[0]} vectors")
    return worst


def _worst_score(name, got, want):
    worst = float((got.double().cpu() - torch.as_tensor(want).double().cpu()).abs().max())
    print(f"{name}: worst |score - want| {worst:.3e} over {got.numel()} scores")
    return worst


def _fixture_run(state_dict, dev, name, precision):
    g = load_golden(name)
    n, _, h, w = [int(v) for v in g["shape"]]
    x = synth.images(n, h, w, seed=int(g["image_seed"])).to(dev)
    model = _make(state_dict, dev, 1, precision)
    score, va, vb = model.region_similarity(x)
    assert tuple(score.shape) == (1, n - 1, 9, 9) and tuple(va.shape) == (1, 1, 9, L) and tuple(vb.shape) == (1, n - 1, 9, L)
    assert score.dtype == va.dtype == vb.dtype == torch.float32 and score.device.type == "cuda"
    s = int(g["vlad_stride"])
    ran = dict(model.base_model.precision_runs)
    ev = max(_worst_vec(f"{name} {precision} vlad_A", va[..., ::s], torch.from_numpy(g["vlad_A"])),
             _worst_vec(f"{name} {precision} vlad_B", vb[..., ::s], torch.from_numpy(g["vlad_B"])))
    es = _worst_score(f"{name} {precision} score", score, g["score"])
    return ev, es, ran


@pytest.mark.parametrize("precision", ["fp32", "f16mx", "bf16x3"])
@pytest.mark.parametrize("name", ["region_small", "region_480x640"])
def test_region_similarity_matches_reference(dev, state_dict, name, precision):
    ev, es, ran = _fixture_run(state_dict, dev, name, precision)
    print(f"{name} {precision}: backbone ran as {ran}")
    if name == "region_480x640" and precision == "f16mx":
        assert ran.get("f16mx", 0) >= 1, ran          # the fixture that puts the f16mx backbone in front of the head
    assert ev <= TOL_VEC and es <= TOL_SCORE, (ev, es)


@pytest.mark.parametrize("name", ["region_small", "region_480x640"])
def test_region_similarity_bf16_is_reported(dev, state_dict, name):
    """bf16 is outside the 1e-4 bar everywhere: its errors are printed, only finiteness is asserted."""
    ev, es, _ = _fixture_run(state_dict, dev, name, "bf16")
    print(f"{name} bf16 (not asserted): vectors {ev:.3e}, scores {es:.3e}")
    assert ev == ev and es == es


@pytest.fixture(scope="module")
def maps48(dev, state_dict):
    """The device's own fp32 conv5_3 maps of 48 images of 480 x 640 (NHWC), and the model's head parameters."""
    model = _make(state_dict, dev, 1, "fp32")
    x = synth.images(48, 480, 640, seed=33)
    feat = torch.cat([model.base_model.features_nhwc(x[i:i + 12].to(dev)) for i in range(0, 48, 12)], dim=0)
    assert feat.dtype == torch.float32 and tuple(feat.shape) == (48, 30, 40, 512)
    w, c = model.net_vlad._params()
    return feat, w, c


@pytest.mark.parametrize("n_img,tuple_size", [(12, 1), (48, 4)])
def test_region_head_at_the_sfrs_tuple_size(dev, state_dict, maps48, n_img, tuple_size):
    feat, w, c = maps48
    feat = feat[:n_img].contiguous()
    vec = ops.region_vlad(feat, w, c, True)
    score = ops.region_scores(vec, tuple_size)
    assert tuple(vec.shape) == (n_img, 9, L) and tuple(score.shape) == (tuple_size, n_img // tuple_size - 1, 9, 9)
    want_vec = region_ref.region_vectors(feat.cpu().permute(0, 3, 1, 2), w.cpu(), c.cpu())
    want_score = region_ref.region_scores(want_vec, tuple_size)
    ev = _worst_vec(f"head alone, {n_img} images", vec, want_vec)
    es = _worst_score(f"head alone, {n_img} images, tuple_size {tuple_size}", score, want_score)
    norms = vec.double().norm(dim=-1)
    print(f"unit norm: max | |v| - 1 | = {float((norms - 1).abs().max()):.3e}")
    assert ev <= TOL_VEC and es <= TOL_SCORE
    assert float((norms - 1).abs().max()) <= TOL_VEC


def test_tuples_are_independent_and_batch_mates_do_not_matter(dev, state_dict, maps48):
    """T > 1 is defined as the T = 1 result per tuple, stacked; an image's region vectors are the same bits in a
    batch of 1, 5, 12 or 48 images (the slab decomposition does not depend on the batch, nothing is accumulated
    atomically)."""
    feat, w, c = maps48
    vec48 = ops.region_vlad(feat, w, c, True)
    for lo, hi in ((0, 1), (7, 8), (5, 10), (12, 24), (36, 48), (47, 48)):
        part = ops.region_vlad(feat[lo:hi].contiguous(), w, c, True)
        assert torch.equal(part, vec48[lo:hi]), (lo, hi)
    s4 = ops.region_scores(vec48, 4)
    for t in range(4):
        s1 = ops.region_scores(vec48[12 * t:12 * (t + 1)].contiguous(), 1)
        assert torch.equal(s1[0], s4[t]), t
    # the same through the model's surface, on small images: tuple_size 3 against three tuple_size 1 calls on the
    # tuples' maps.  (The maps come from ONE backbone call: the backbone picks its split-K plan by the batch size, so
    # its own output is batch-invariant only up to fp32 association — not this head's business.)
    x = synth.images(9, 64, 96, seed=34).to(dev)
    m3, m1 = _make(state_dict, dev, 3), _make(state_dict, dev, 1)
    score, va, vb = m3.region_similarity(x)
    assert tuple(score.shape) == (3, 2, 9, 9) and tuple(va.shape) == (3, 1, 9, L) and tuple(vb.shape) == (3, 2, 9, L)
    fmap = ops.nhwc_to_nchw_f32(m3.base_model.features_nhwc(x))
    for t in range(3):
        s, a, b = m1._compute_region_sim(fmap[3 * t:3 * t + 1], fmap[3 * t + 1:3 * t + 3])
        assert torch.equal(s[0], score[t]) and torch.equal(a[0], va[t]) and torch.equal(b[0], vb[t]), t
    # and against separate backbone calls per tuple, to the project's bar
    for t in range(3):
        s, a, b = m1.region_similarity(x[3 * t:3 * t + 3])
        assert _worst_vec(f"tuple {t} alone", torch.cat([a, b], 1), torch.cat([va[t:t + 1], vb[t:t + 1]], 1)) <= TOL_VEC
        assert _worst_score(f"tuple {t} alone", s[0], score[t]) <= TOL_SCORE


@pytest.mark.parametrize("hw", [(64, 96), (480, 640)])
def test_region_zero_is_the_image_vlad_and_scores_are_the_dots(dev, state_dict, hw):
    """Region 0 is the whole image: against EmbedNet's eval VLAD (the existing kernels) of the same weights and
    images; score against the fp64 dots of the vectors the call returned."""
    x = synth.images(4, hw[0], hw[1], seed=35).to(dev)
    region = _make(state_dict, dev, 2)
    plain = _make(state_dict, dev, kind="embednet")
    score, va, vb = region.region_similarity(x)
    _, vlad = plain(x)
    vec = torch.cat([va, vb], dim=1).reshape(4, 9, L)
    e0 = _worst_vec(f"region 0 against EmbedNet's VLAD {hw}", vec[:, 0], vlad)
    want = region_ref.region_scores(vec.cpu(), 2)
    es = _worst_score(f"score against the fp64 dots of the returned vectors {hw}", score, want)
    assert e0 <= TOL_VEC and es <= TOL_SCORE
    # the eval branch is untouched: still EmbedNet's forward bit for bit; training-mode forward still raises
    p1, v1 = region(x)
    p2, v2 = plain(x)
    assert torch.equal(p1, p2) and torch.equal(v1, v2)
    region.train()
    try:
        with pytest.raises(NotImplementedError):
            region(x)
        s2, a2, b2 = region.region_similarity(x)            # works in either module mode
        assert torch.equal(s2, score) and torch.equal(a2, va) and torch.equal(b2, vb)
    finally:
        region.eval()


def test_a_pair_that_copies_the_anchor(dev, state_dict):
    """score[t, j] of a pair that is the anchor image again is symmetric with a unit diagonal; all vectors have
    unit norm; shapes and dtypes."""
    x = synth.images(3, 96, 128, seed=36)
    x[2] = x[0]
    score, va, vb = _make(state_dict, dev, 1).region_similarity(x.to(dev))
    assert tuple(score.shape) == (1, 2, 9, 9) and score.dtype == torch.float32
    s = score[0, 1].double().cpu()
    print(f"copy of the anchor: max |S - S^T| {float((s - s.T).abs().max()):.3e}, "
          f"max |diag - 1| {float((s.diagonal() - 1).abs().max()):.3e}")
    assert float((s - s.T).abs().max()) <= TOL_SCORE and float((s.diagonal() - 1).abs().max()) <= TOL_SCORE
    norms = torch.cat([va, vb], dim=1).double().norm(dim=-1)
    assert float((norms - 1).abs().max()) <= TOL_VEC
    # halves overlap their quarters: not a degenerate table
    assert float(score[0, 0].min()) < 0.999


def test_region_errors(dev, state_dict):
    m1, m2 = _make(state_dict, dev, 1), _make(state_dict, dev, 2)
    with pytest.raises(ValueError, match="4 x 5"):
        m1.region_similarity(synth.images(2, 70, 90, seed=13).to(dev))          # odd map side
    with pytest.raises(ValueError, match="multiple of tuple_size"):
        m2.region_similarity(synth.images(3, 64, 96, seed=13).to(dev))
    with pytest.raises(ValueError, match="at least one pair"):
        m2.region_similarity(synth.images(2, 64, 96, seed=13).to(dev))          # two tuples of one image
    with pytest.raises(ValueError, match="at least one pair"):
        m1.region_similarity(synth.images(1, 64, 96, seed=13).to(dev))
    w, c = m1.net_vlad._params()
    with pytest.raises(ValueError, match="5 x 6"):
        ops.region_vlad(torch.zeros((1, 5, 6, 512), device=dev), w, c)
    with pytest.raises(ValueError):
        ops.region_scores(torch.zeros((3, 9, L), device=dev), 2)


def test_compute_region_sim_takes_nchw_maps(dev, state_dict):
    """The reference's entry point for callers that hold conv5 maps: same numbers as region_similarity."""
    x = synth.images(6, 64, 96, seed=37).to(dev)
    m = _make(state_dict, dev, 2)
    score, va, vb = m.region_similarity(x)
    feat = ops.nhwc_to_nchw_f32(m.base_model.features_nhwc(x))                   # [6][512][4][6]
    per = feat.view(2, 3, *feat.shape[1:])
    fa = per[:, 0].contiguous()
    fb = per[:, 1:].reshape(4, *feat.shape[1:]).contiguous()
    s2, a2, b2 = m._compute_region_sim(fa, fb)
    assert torch.equal(s2, score) and torch.equal(a2, va) and torch.equal(b2, vb)
    with pytest.raises(ValueError):
        m._compute_region_sim(fa, fb[:3])
