"""Gradients of the NetVLAD descriptor head on the device (csrc/netvlad_backward.hip, ops.netvlad_backward /
netvlad_head, NetVLAD.head_with_grad, EmbedNet.forward_train) against the numpy float64 evaluation of the same
formulas (tests/helpers/netvlad_grad_ref.py), which tests/test_netvlad_backward_cpu.py ties to the reference's own
autograd (tests/golden/netvlad_backward_*.npz).

Bars, per gradient: 8 x the rel-L2 error of the REFERENCE's fp32 autograd against float64 on the golden case with the
same `normalize_input`, as tests/helpers/make_netvlad_backward_golden.py printed it and stored it in the fixture
(`ref_err`), never above 1e-4.  Both are fp32 evaluations of the same sums in different orders.
                                  dW        dC        dX
  reference, 2x(3x5) normalised   2.59e-6   1.03e-7   3.55e-7     -> bars 2.07e-5  8.21e-7  2.84e-6
  reference, 3x(4x6) raw          2.78e-6   5.07e-7   2.61e-6     -> bars 2.22e-5  4.05e-6  2.09e-5
The kernels' measured errors are in DESIGN §4.5: 3.9e-7 | 3.2e-8 | 2.6e-7 and 6.6e-7 | 5.6e-8 | 6.3e-7 on these two cases."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from helpers import netvlad_grad_ref as ref
from openibl_amd import ops, synth

pytestmark = pytest.mark.gpu

K, C = 64, 512
GOLDENS = {True: "netvlad_backward_2x3x5_norm", False: "netvlad_backward_3x4x6_raw"}
_cache = {}


def bars(normalize):
    """{"dW", "dC", "dX"} -> 8 x the reference's own fp32 error on the golden case of this mode, capped at 1e-4."""
    e = load_golden(GOLDENS[bool(normalize)])["ref_err"]
    return {k: min(8.0 * float(v), 1e-4) for k, v in zip(("dW", "dC", "dX"), e)}


def case(seed, N, h, w_, normalize, zero_pixel=None):
    """Inputs (numpy fp32) and the float64 gradients of a case, computed once per session."""
    key = (seed, N, h, w_, bool(normalize), zero_pixel)
    if key not in _cache:
        x, w, c, G = ref.draw_inputs(seed, N, h, w_)
        if zero_pixel is not None:
            x[zero_pixel] = 0.0
        _cache[key] = ((x, w, c, G), ref.head_and_grads(x, w, c, G, normalize))
    return _cache[key]


def run(dev, inputs, normalize, want=("w", "c", "x")):
    x, w, c, G = (torch.from_numpy(t).to(dev) for t in inputs)
    return ops.netvlad_backward(x, w, c, G, normalize_input=normalize, want=want)


def check(name, got, want, normalize, keys=("dW", "dC", "dX")):
    bar = bars(normalize)
    errs = {}
    for k, g in zip(("dW", "dC", "dX"), got):
        if k in keys:
            assert g.dtype == torch.float32 and tuple(g.shape) == want[k].shape
            assert torch.isfinite(g).all(), (name, k)
            errs[k] = ref.rel_l2(g.cpu().numpy(), want[k])
    print(name, " ".join(f"{k} {v:.3e} (bar {bar[k]:.2e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bar[k], (name, k, v, bar[k])


@pytest.mark.parametrize("normalize", [True, False])
def test_golden_cases_through_the_c_abi(dev, normalize):
    g = load_golden(GOLDENS[normalize])
    N, h, w_, _ = map(int, g["shape"])
    assert bool(g["normalize_input"]) == normalize
    inputs, want = case(int(g["seed"]), N, h, w_, normalize)
    got = run(dev, inputs, normalize)
    check(GOLDENS[normalize], got, want, normalize)
    # and against the reference's own numbers: the kernel and the reference are each inside their bar of float64
    bar = bars(normalize)
    for k, t in zip(("dW", "dC", "dX"), got):
        e = ref.rel_l2(t.cpu().numpy(), g[k])
        print(f"  {k} against the reference's fp32 autograd: {e:.3e}")
        assert e <= bar[k] + float(g["ref_err"][("dW", "dC", "dX").index(k)])


@pytest.mark.parametrize("N,h,w_", [(1, 3, 5), (3, 5, 7), (2, 7, 11), (2, 30, 40)])
def test_shapes_without_a_golden(dev, N, h, w_):
    """Below one 32-pixel chunk, a chunk plus a tail of 3, several chunks with a tail, the production map."""
    inputs, want = case(100 + h, N, h, w_, True)
    check(f"{N}x({h}x{w_})", run(dev, inputs, True), want, True)


def test_raw_input_with_a_tail(dev):
    inputs, want = case(205, 3, 5, 7, False)
    check("3x(5x7) raw", run(dev, inputs, False), want, False)


def test_each_output_alone_equals_the_full_call(dev):
    inputs, _ = case(107, 2, 7, 11, True)
    full = run(dev, inputs, True)
    for i, letter in enumerate(("w", "c", "x")):
        alone = run(dev, inputs, True, want=(letter,))
        assert [t is None for t in alone] == [j != i for j in range(3)]
        assert torch.equal(alone[i], full[i]), letter


def test_two_runs_are_bit_identical(dev):
    inputs, _ = case(130, 2, 30, 40, True)
    a, b = run(dev, inputs, True), run(dev, inputs, True)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_grad_feat_of_an_image_does_not_depend_on_its_batch_mates(dev):
    inputs, _ = case(105, 3, 5, 7, True)
    x, w, c, G = inputs
    gx3 = run(dev, inputs, True, want=("x",))[2]
    gx1 = run(dev, (x[:1].copy(), w, c, G[:1].copy()), True, want=("x",))[2]
    assert torch.equal(gx3[0], gx1[0])


def test_an_all_zero_pixel(dev):
    """r_p sits on the clamp: a constant denominator, dx_p = dxh_p / eps.  That row and the others are compared
    separately (the row is 1e12 times larger than the rest)."""
    inputs, want = case(107, 2, 7, 11, True, zero_pixel=(1, 3, 4))
    gx = run(dev, inputs, True, want=("x",))[2].cpu().numpy()
    assert np.isfinite(gx).all()
    bar = bars(True)["dX"]
    row = ref.rel_l2(gx[1, 3, 4], want["dX"][1, 3, 4])
    rest_g, rest_w = gx.copy(), want["dX"].copy()
    rest_g[1, 3, 4] = 0.0
    rest_w[1, 3, 4] = 0.0
    rest = ref.rel_l2(rest_g, rest_w)
    print(f"zero pixel: its row {row:.3e}, the other rows {rest:.3e} (bar {bar:.2e}); |row|max {np.abs(gx[1, 3, 4]).max():.3e}")
    assert np.abs(want["dX"][1, 3, 4]).max() > 1e6
    assert row <= bar and rest <= bar


def test_netvlad_head_forward_and_autograd(dev, monkeypatch):
    inputs, _ = case(105, 3, 5, 7, True)
    x, w, c, G = (torch.from_numpy(t).to(dev) for t in inputs)
    _, plain = ops.netvlad(x, w, c, True, want_norm=True)
    direct = ops.netvlad_backward(x, w, c, G, True)
    xg, wg, cg = (t.clone().requires_grad_(True) for t in (x, w, c))
    y = ops.netvlad_head(xg, wg, cg, True)
    assert torch.equal(y, plain)
    y.backward(G)
    for got, want_ in zip((wg.grad, cg.grad, xg.grad), direct):
        assert torch.equal(got, want_)
    # only what autograd needs: the map and the centroids frozen -> None for both, the same dW bits
    asked = []
    inner = ops.netvlad_backward

    def spy(*args, **kwargs):
        asked.append(tuple(kwargs["want"]))
        out = inner(*args, **kwargs)
        asked.append(tuple(t is None for t in out))
        return out

    monkeypatch.setattr(ops, "netvlad_backward", spy)
    wg2 = w.clone().requires_grad_(True)
    ops.netvlad_head(x, wg2, c, True).backward(G)
    monkeypatch.setattr(ops, "netvlad_backward", inner)
    assert asked == [("w",), (False, True, True)] and torch.equal(wg2.grad, direct[0])
    # conv.weight's own shape passes through
    w4 = w.reshape(K, C, 1, 1).clone().requires_grad_(True)
    ops.netvlad_head(x, w4, c, True).backward(G)
    assert tuple(w4.grad.shape) == (K, C, 1, 1) and torch.equal(w4.grad.reshape(K, C), direct[0])
    # nothing requires a gradient: no graph
    assert not ops.netvlad_head(x, w, c, True).requires_grad


def _tuple_loss(vlad, B, n, margin=0.3):
    """Trainer._get_loss(..., 'triplet') of the reference (ibl/trainers.py:82-95)."""
    out = vlad.view(B, n, -1)
    L = out.size(-1)
    neg = out[:, 2:]
    anc = out[:, 0].unsqueeze(1).expand_as(neg).contiguous().view(-1, L)
    pos = out[:, 1].unsqueeze(1).expand_as(neg).contiguous().view(-1, L)
    return F.triplet_margin_loss(anc, pos, neg.contiguous().view(-1, L), margin=margin, p=2, reduction="mean")


def test_embednet_forward_train(dev, state_dict):
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    model = models.create("embednet", base, pool)
    model.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    model = model.to(dev).set_precision("fp32")
    B, n = 3, 4                                             # three tuples: anchor, positive, two negatives
    x = synth.images(B * n, 32, 48, seed=77).to(dev)
    model.eval()
    _, vlad_eval = model(x)
    model.train()
    pool_x, vlad_x = model.forward_train(x)
    assert torch.equal(vlad_x, vlad_eval) and tuple(pool_x.shape) == (B * n, 512)
    assert vlad_x.requires_grad and not pool_x.requires_grad

    nv = model.net_vlad
    leaf = vlad_x.detach().requires_grad_(True)
    _tuple_loss(leaf, B, n).backward()
    loss0 = _tuple_loss(vlad_x, B, n)
    loss0.backward()
    assert all(p.grad is None for p in model.base_model.parameters())
    feat = model.base_model.features_nhwc(x)
    want = ref.head_and_grads(feat.float().cpu().numpy(), nv.conv.weight.detach().reshape(K, C).cpu().numpy(),
                              nv.centroids.detach().cpu().numpy(), leaf.grad.cpu().numpy(), nv.normalize_input)
    assert float(loss0) > 0 and np.abs(want["dW"]).max() > 0
    check("forward_train", (nv.conv.weight.grad.reshape(K, C), nv.centroids.grad, None), want, nv.normalize_input,
          keys=("dW", "dC"))

    # three SGD steps on the fixed batch; the step aims at a 5 % first-order decrease of the loss
    g2 = float(sum((p.grad.double() ** 2).sum() for p in nv.parameters()))
    opt = torch.optim.SGD(nv.parameters(), lr=0.05 * float(loss0) / g2)
    losses = [float(loss0)]
    for _ in range(3):
        opt.step()
        opt.zero_grad()
        loss = _tuple_loss(model.forward_train(x)[1], B, n)
        loss.backward()
        losses.append(float(loss))
    print("forward_train: losses", losses)
    assert losses[-1] < losses[0]

    # the eval forward reflects the stepped weights: it equals the training forward on them, not the first one
    model.eval()
    _, after = model(x)
    assert torch.equal(after, model.forward_train(x)[1].detach())
    assert not torch.equal(after, vlad_eval)


def test_forward_train_in_the_default_arithmetic_and_from_a_bf16_map(dev, state_dict):
    """f16mx (the default; its conv5 map is fp32, behind the range guard): vlad_x is the eval forward's bits.  A bf16
    map is widened to fp32 first: the head's output is the fp32 head's on the widened map, and the map's gradient
    comes back in bf16."""
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    model = models.create("embednet", base, pool)
    model.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    model = model.to(dev).eval().set_precision("f16mx")
    x = synth.images(4, 32, 48, seed=78).to(dev)
    _, vlad_eval = model(x)
    pool_x, vlad_x = model.forward_train(x)
    assert torch.equal(vlad_x, vlad_eval) and vlad_x.requires_grad
    vlad_x.sum().backward()
    assert model.net_vlad.centroids.grad is not None and torch.isfinite(model.net_vlad.conv.weight.grad).all()

    inputs, _ = case(105, 3, 5, 7, True)
    xf, w, c, G = (torch.from_numpy(t).to(dev) for t in inputs)
    xb = xf.to(torch.bfloat16).requires_grad_(True)
    y = ops.netvlad_head(xb, w, c, True)
    wide = xb.detach().float()
    assert torch.equal(y, ops.netvlad(wide, w, c, True, want_norm=True)[1])
    y.backward(G)
    want = ops.netvlad_backward(wide, w, c, G, True, want=("x",))[2]
    assert xb.grad.dtype == torch.bfloat16 and torch.equal(xb.grad, want.to(torch.bfloat16))


def test_region_net_in_training_mode_still_raises(dev, state_dict):
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    region = models.create("embedregionnet", base, pool, tuple_size=1).to(dev)
    region.train()
    with pytest.raises(NotImplementedError):
        region(synth.images(2, 32, 48, seed=3).to(dev))
