"""conv5 training on the device: the gradients of a 3x3 convolution (csrc/conv_backward.hip, ops.conv3x3_backward /
conv3x3_train), the frozen trunk up to pool4 (ops.vgg16_pool4) and EmbedNet.forward_train(x, train_layers='conv5'),
against the float64 evaluation of tests/helpers/conv_grad_ref.py, which tests/test_conv_backward_cpu.py ties to the
reference's own autograd (tests/golden/conv5_backward.npz).

Bars, per gradient: 8 x the rel-L2 error of the REFERENCE's fp32 autograd against float64 as the generator stored it
(`ref_err`), never above 1e-4: two fp32 evaluations of the same sums in different orders.  Layer level: the (3, 5, 7)
layer case, for dW and db the smallest of the three layers' figures; end to end: the end-to-end case's figures.
                          dX        dW (min of 3)   db (min of 3)
  reference, 3x(5x7)      3.40e-7   2.93e-7         1.76e-7       -> bars 2.72e-6  2.34e-6  1.41e-6
  reference, end to end   dW1..3 3.96e-6 4.20e-6 5.92e-6  db1..3 3.96e-6 3.95e-6 4.94e-6  dWv 6.08e-6  dCv 6.79e-6
The kernels' measured errors (MI355X; all of them in DESIGN §4.5), dW | db | dX: one layer 1 x (30 x 40) 2.0e-7 | 2.6e-8 |
1.2e-6, 3 x (5 x 7) 1.2e-7 | 2.9e-8 | 1.1e-6; the 3 x (5 x 7) chain dX 1.6e-6, dW1..3 1.4e-6 1.4e-6 1.2e-6, db1..3 1.5e-6
1.1e-6 2.7e-8; end to end dW1..3 9.5e-6 1.0e-5 1.4e-5, db1..3 9.7e-6 1.0e-5 1.3e-5, dWv 1.4e-5, dCv 1.6e-5.

Shapes of the layer-level cases (M = N h w pixels; the weight gradient walks them in steps of 32, chains of 256 and at
most 7 K splits, the input gradient in tiles of 128 pixels): 1 (the centre tap alone), 12, 105, 154, 1200 (the
production map), 78 (13 images), 256 | 257 (one chain | a second chain of one pixel), 1792 | 2050 (7 chains, one per
split | 9 chains, splits 0 and 1 take two)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import conv_grad_ref as ref
from openibl_amd import lib as _lib
from openibl_amd import ops, synth

pytestmark = pytest.mark.gpu

C = 512
SHAPES = [(1, 1, 1), (2, 2, 3), (3, 5, 7), (2, 7, 11), (1, 30, 40), (13, 2, 3), (1, 16, 16), (1, 1, 257),
          (1, 28, 64), (1, 41, 50)]
_cache = {}


def golden():
    if "golden" not in _cache:
        _cache["golden"] = load_golden("conv5_backward")
    return _cache["golden"]


def layer_bars():
    e = dict(zip(ref.GRAD_KEYS, golden()["layer_3x5x7_ref_err"]))
    return {"dX": min(8.0 * e["dX"], 1e-4), "dW": min(8.0 * min(e["dW1"], e["dW2"], e["dW3"]), 1e-4),
            "db": min(8.0 * min(e["db1"], e["db2"], e["db3"]), 1e-4)}


def chain_bars(prefix, keys):
    e = dict(zip(keys, golden()[f"{prefix}_ref_err"]))
    return {k: min(8.0 * float(v), 1e-4) for k, v in e.items()}, e


def layer_case(N, h, w, mask):
    """Inputs (numpy fp32) and float64 gradients of one layer, computed once per session: x, weight, G of
    draw_inputs(1000 + M); the mask is the layer's own post-ReLU output (float64 forward, rounded to fp32)."""
    key = (N, h, w, mask)
    if key not in _cache:
        x, ws, bs, G = ref.draw_inputs(1000 + N * h * w, N, h, w)
        act = ref.conv_forward(x, ws[0], bs[0], True).astype(np.float32) if mask else None
        _cache[key] = ((x, ws[0], G, act), ref.layer_grads(x, ws[0], G, act))
    return _cache[key]


def run(dev, inputs, want=("w", "b", "x")):
    x, w, G, act = (None if t is None else torch.from_numpy(t).to(dev) for t in inputs)
    return ops.conv3x3_backward(x, w, G, out_act=act, want=want)


def check(name, got, want, bars, keys=("dW", "db", "dX")):
    errs = {}
    for k, g in zip(("dW", "db", "dX"), got):
        if k in keys:
            assert g.dtype == torch.float32 and tuple(g.shape) == want[k].shape, (name, k)
            assert torch.isfinite(g).all(), (name, k)
            errs[k] = ref.rel_l2(g.cpu().numpy(), want[k])
    print(name, " ".join(f"{k} {v:.3e} (bar {bars[k]:.2e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bars[k], (name, k, v, bars[k])


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("N,h,w", SHAPES)
def test_layer_against_float64(dev, N, h, w, mask):
    inputs, want = layer_case(N, h, w, mask)
    check(f"{N}x({h}x{w}){' relu' if mask else ''}", run(dev, inputs), want, layer_bars())


@pytest.mark.parametrize("name", ["layer_2x2x3", "layer_3x5x7"])
def test_golden_chain_through_conv3x3_train(dev, name):
    """The three layers as autograd functions on the golden inputs: against the float64 chain, and against the
    reference's own numbers (both are inside their bar of float64: bar + ref_err)."""
    g = golden()
    N, h, w, _ = map(int, g[f"{name}_shape"])
    x, ws, bs, G = ref.draw_inputs(int(g[f"{name}_seed"]), N, h, w)
    if ("chain", name) not in _cache:
        _cache[("chain", name)] = ref.chain_grads(x, ws, bs, G)
    want = _cache[("chain", name)]
    xt = torch.from_numpy(x).to(dev).requires_grad_(True)
    wt = [torch.from_numpy(t).to(dev).requires_grad_(True) for t in ws]
    bt = [torch.from_numpy(t).to(dev).requires_grad_(True) for t in bs]
    t = xt
    for i in range(3):
        t = ops.conv3x3_train(t, wt[i], bt[i], relu=i < 2)
    t.backward(torch.from_numpy(G).to(dev))
    got = {"dX": xt.grad}
    for i in range(3):
        got[f"dW{i + 1}"], got[f"db{i + 1}"] = wt[i].grad, bt[i].grad
    bars, ref_err = chain_bars("layer_3x5x7", ref.GRAD_KEYS)
    _, own_err = chain_bars(name, ref.GRAD_KEYS)
    ey = ref.rel_l2(t.detach().cpu().numpy(), want["y"])
    ys = int(g[f"{name}_y_stride"])
    print(name, f"y {ey:.3e}; against the reference {ref.rel_l2(t.detach().cpu().numpy()[..., ::ys], g[f'{name}_y']):.3e}")
    assert ey <= 2e-6
    for k in ref.GRAD_KEYS:
        a = got[k].cpu().numpy()
        e64 = ref.rel_l2(a, want[k])
        stored = g[f"{name}_{k}"]
        eref = ref.rel_l2(a[:ref.W_ROWS] if k.startswith("dW") else a, stored)
        print(f"  {k} {e64:.3e} (bar {bars[k]:.2e}); against the reference's fp32 autograd {eref:.3e}")
        assert e64 <= bars[k], (name, k, e64, bars[k])
        assert eref <= bars[k] + float(own_err[k]), (name, k, eref)


def test_masked_positions_contribute_exactly_zero(dev):
    """out_act with exact zeros and negative values: the gradient there is excluded — whatever grad_out holds (here
    1e30) — and the outputs are the bits of the call on the pre-masked grad_out without out_act."""
    x, ws, _, G = ref.draw_inputs(31, 2, 7, 11)
    rs = np.random.RandomState(32)
    act = rs.standard_normal(G.shape).astype(np.float32)
    act[rs.uniform(size=G.shape) < 0.3] = 0.0
    assert (act == 0).sum() > 1000 and (act < 0).sum() > 1000 and (act > 0).sum() > 1000
    dz = np.where(act > 0, G, np.float32(0.0)).astype(np.float32)
    poisoned = np.where(act > 0, G, np.float32(1e30)).astype(np.float32)
    masked = run(dev, (x, ws[0], poisoned, act))
    plain = run(dev, (x, ws[0], dz, None))
    for a, b in zip(masked, plain):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    check("mask", masked, ref.layer_grads(x, ws[0], poisoned, act), layer_bars())


def test_each_output_alone_equals_the_full_call(dev):
    inputs, _ = layer_case(2, 7, 11, True)
    full = run(dev, inputs)
    for i, letter in enumerate(("w", "b", "x")):
        alone = run(dev, inputs, want=(letter,))
        assert [t is None for t in alone] == [j != i for j in range(3)]
        assert torch.equal(alone[i], full[i]), letter


def test_two_runs_are_bit_identical(dev):
    inputs, _ = layer_case(1, 41, 50, True)
    a, b = run(dev, inputs), run(dev, inputs)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_grad_in_of_an_image_does_not_depend_on_its_batch_mates(dev):
    inputs, _ = layer_case(3, 5, 7, True)
    x, w, G, act = inputs
    gx3 = run(dev, inputs, want=("x",))[2]
    gx1 = run(dev, (x[:1].copy(), w, G[:1].copy(), act[:1].copy()), want=("x",))[2]
    assert torch.equal(gx3[0], gx1[0])


def test_conv3x3_train_asks_only_for_what_autograd_needs(dev, monkeypatch):
    x, ws, bs, G = ref.draw_inputs(33, 2, 2, 3)
    xd, wd, bd, Gd = (torch.from_numpy(t).to(dev) for t in (x, ws[0], bs[0], G))
    y_plain = ops.conv3x3_nhwc(xd, ops.pack_conv3x3(wd, "fp32"), bd, True, False, "fp32")
    direct = ops.conv3x3_backward(xd, wd, Gd, out_act=y_plain)
    asked = []
    inner = ops.conv3x3_backward

    def spy(*args, **kwargs):
        asked.append(tuple(kwargs["want"]))
        return inner(*args, **kwargs)

    monkeypatch.setattr(ops, "conv3x3_backward", spy)
    wg, bg = wd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    y = ops.conv3x3_train(xd, wg, bg, True)                  # the input carries no graph: no grad_in stage
    assert torch.equal(y, y_plain)
    y.backward(Gd)
    assert asked == [("w", "b")] and torch.equal(wg.grad, direct[0]) and torch.equal(bg.grad, direct[1])
    xg, bg2 = xd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    ops.conv3x3_train(xg, wd, bg2, True).backward(Gd)        # a frozen weight: no weight-gradient stage
    assert asked[1] == ("x", "b") and torch.equal(xg.grad, direct[2]) and torch.equal(bg2.grad, direct[1])
    assert not ops.conv3x3_train(xd, wd, bd, True).requires_grad


# ---- the frozen trunk ---------------------------------------------------------------------------------------------
def _trunk_layers(dev, x, convs, with_scratch):
    """conv1_1 .. conv4_3 + pool in fp32, one C call per layer -> (pool4, [conv5 packed weights], [conv5 biases]).
    with_scratch: every layer gets the split-K scratch the backbone entry gives it (oibl_conv3x3_workspace_bytes):
    the same kernels in the same association as oibl_vgg16_*_forward; without: ops.conv3x3_nhwc, one pass."""
    h = _lib.load()
    t = ops.conv1_1_nchw(x, convs[0][0], convs[0][1], "fp32")
    for l in range(1, 10):
        cin, cout, relu, pool = ops.VGG16_CFG[l]
        pw = ops.pack_conv3x3(convs[l][0], "fp32")
        if not with_scratch:
            t = ops.conv3x3_nhwc(t, pw, convs[l][1], bool(relu), bool(pool), "fp32")
            continue
        N, H, W, _ = map(int, t.shape)
        out = torch.empty((N, H // 2, W // 2, cout) if pool else (N, H, W, cout), dtype=torch.float32, device=dev)
        nb = h.oibl_conv3x3_workspace_bytes(N, H, W, cin, cout, pool, ops.F32)
        ws = ops.workspace(nb, dev, "test_trunk") if nb else None
        _lib.check(h.oibl_conv3x3_nhwc_ws(t.data_ptr(), N, H, W, cin, pw.data_ptr(), convs[l][1].data_ptr(), cout, relu,
                                          pool, ops.F32, out.data_ptr(), ws.data_ptr() if nb else None, nb, None,
                                          torch.cuda.current_stream(dev).cuda_stream), "conv3x3_nhwc_ws")
        t = out
    return t


def test_vgg16_pool4_in_every_precision(dev, state_dict):
    """fp32: the bits of the fp32 trunk run layer by layer with the scratch the backbone entry gives its layers (the
    entry splits K on small batches: against the one-pass layers of ops.conv3x3_nhwc it is an fp32 re-association,
    held to the oracle tolerance 2e-6); bf16x3 and f16mx: 1e-4 rel-L2, the project's parity bar; bf16: printed.  The
    conv5_3 map of `vgg16_conv5` is the same bits before and after, and in fp32 it is conv5_1..3 on pool4."""
    x = synth.images(4, 32, 48, seed=79).to(dev)
    convs = [(state_dict[f"base_model.base.{i}.weight"].to(dev), state_dict[f"base_model.base.{i}.bias"].to(dev))
             for i in ops.VGG16_CONV_IDX]
    want = _trunk_layers(dev, x, convs, True)
    one_pass = _trunk_layers(dev, x, convs, False)
    assert tuple(want.shape) == (4, 2, 3, 512) and float(want.abs().max()) > 0
    for prec in ("fp32", "f16mx", "bf16x3", "bf16"):
        ws = [convs[0][0]] + [ops.pack_conv3x3(w, prec) for w, _ in convs[1:]]
        bs = [b for _, b in convs]
        before = ops.vgg16_conv5(x, ws, bs, prec).clone()
        pool4, flag = ops.vgg16_pool4(x, ws, bs, prec, return_flag=True)
        assert pool4.dtype == torch.float32 and tuple(pool4.shape) == (4, 2, 3, 512)
        assert (flag is not None) == (prec == "f16mx") and (flag is None or int(flag.item()) == 0)
        e = ref.rel_l2(pool4.cpu().numpy(), want.cpu().numpy())
        print(f"pool4 {prec}: rel-L2 against the fp32 trunk {e:.3e}")
        if prec == "fp32":
            assert torch.equal(pool4, want)
            e1 = ref.rel_l2(pool4.cpu().numpy(), one_pass.cpu().numpy())
            print(f"pool4 fp32 against the one-pass layers: {e1:.3e}")
            assert e1 <= 2e-6
            t = pool4
            for l in (10, 11, 12):
                t = ops.conv3x3_nhwc(t, ws[l], bs[l], l < 12, False, "fp32")
            e5 = ref.rel_l2(t.cpu().numpy(), before.cpu().numpy())
            print(f"conv5_1..3 on pool4 against vgg16_conv5: {e5:.3e}")
            assert e5 <= 2e-6
        elif prec != "bf16":
            assert e <= 1e-4, (prec, e)
        assert torch.isfinite(pool4).all()
        assert torch.equal(ops.vgg16_conv5(x, ws, bs, prec), before), prec


# ---- EmbedNet.forward_train(x, train_layers='conv5') ----------------------------------------------------------------
def _model(dev, state_dict, precision):
    from ibl import models
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    model = models.create("embednet", base, pool)
    model.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    return model.to(dev).set_precision(precision)


def _e2e(state_dict):
    g = golden()
    B, n, H, W = map(int, g["e2e_shape"])
    if "e2e" not in _cache:
        state = {k: v for k, v in state_dict.items() if not k.startswith("pca_layer")}
        images = synth.images(B * n, H, W, seed=int(g["e2e_seed"]))
        _cache["e2e"] = (images, ref.embednet_grads(images, state, B, n))
    return (B, n) + _cache["e2e"]


def _grads(model):
    b, nv = model.base_model.base, model.net_vlad
    out = {"dWv": nv.conv.weight.grad, "dCv": nv.centroids.grad}
    for i, li in enumerate((24, 26, 28)):
        out[f"dW{i + 1}"], out[f"db{i + 1}"] = b[li].weight.grad, b[li].bias.grad
    return out


def test_forward_train_conv5(dev, state_dict):
    g = golden()
    B, n, images, want = _e2e(state_dict)
    model = _model(dev, state_dict, "fp32")
    x = images.to(dev)
    model.eval()
    _, vlad_eval = model(x)
    model.train()
    pool_x, vlad_x = model.forward_train(x, train_layers="conv5")
    ev = ref.rel_l2(vlad_x.detach().cpu().numpy(), vlad_eval.cpu().numpy())
    print(f"forward_train conv5: vlad_x against the eval forward {ev:.3e}, against float64 "
          f"{ref.rel_l2(vlad_x.detach().cpu().numpy(), want['vlad']):.3e}")
    assert ev <= 2e-6
    assert vlad_x.requires_grad and not pool_x.requires_grad and pool_x.grad_fn is None
    assert tuple(pool_x.shape) == (B * n, 512) and ref.rel_l2(pool_x.cpu().numpy(), model(x)[0].cpu().numpy()) <= 2e-6
    loss0 = ref.tuple_loss(vlad_x, B, n)
    loss0.backward()
    print(f"loss {float(loss0.detach()):.9f}, the reference's {float(g['e2e_loss']):.9f}, float64 {want['loss']:.9f}")
    assert abs(float(loss0) - want["loss"]) <= 1e-5 * want["loss"]
    trunk = [p for i in range(24) for p in model.base_model.base[i].parameters()]
    assert len(trunk) == 20 and all(p.grad is None for p in trunk)
    bars, ref_err = chain_bars("e2e", ref.E2E_KEYS)
    got = {k: v.reshape(want[k].shape).cpu().numpy() for k, v in _grads(model).items()}
    hs = int(g["e2e_head_stride"])
    for k in ref.E2E_KEYS:
        e64 = ref.rel_l2(got[k], want[k])
        part = got[k][:ref.W_ROWS] if k in ("dW1", "dW2", "dW3") else got[k][::hs] if k in ("dWv", "dCv") else got[k]
        eref = ref.rel_l2(part, g[f"e2e_{k}"])
        print(f"  {k} {e64:.3e} (bar {bars[k]:.2e}); against the reference's fp32 autograd {eref:.3e}")
        assert np.isfinite(got[k]).all() and e64 <= bars[k], (k, e64, bars[k])
        assert eref <= bars[k] + float(ref_err[k]), (k, eref)
    first = {k: v.clone() for k, v in _grads(model).items()}

    # a frozen parameter gets no gradient, the others the same bits
    model.zero_grad(set_to_none=True)
    model.base_model.base[24].weight.requires_grad_(False)
    ref.tuple_loss(model.forward_train(x, train_layers="conv5")[1], B, n).backward()
    again = _grads(model)
    assert again["dW1"] is None
    for k in ref.E2E_KEYS:
        assert k == "dW1" or torch.equal(again[k], first[k]), k
    model.base_model.base[24].weight.requires_grad_(True)
    model.base_model.base[24].weight.grad = first["dW1"]

    # three SGD steps on the fixed batch; the step aims at a 5 % first-order decrease of the loss
    params = [p for i in (24, 26, 28) for p in model.base_model.base[i].parameters()] + list(model.net_vlad.parameters())
    assert len(params) == 8
    g2 = float(sum((p.grad.double() ** 2).sum() for p in params))
    opt = torch.optim.SGD(params, lr=0.05 * float(loss0) / g2)
    w_before = model.base_model.base[26].weight.detach().clone()
    losses = [float(loss0)]
    for _ in range(3):
        opt.step()
        opt.zero_grad()
        loss = ref.tuple_loss(model.forward_train(x, train_layers="conv5")[1], B, n)
        loss.backward()
        losses.append(float(loss))
    print("forward_train conv5: losses", losses)
    assert losses[-1] < losses[0] and not torch.equal(model.base_model.base[26].weight.detach(), w_before)
    # the eval forward reflects the stepped conv5 weights
    model.eval()
    _, after = model(x)
    now = model.forward_train(x, train_layers="conv5")[1].detach()
    assert ref.rel_l2(after.cpu().numpy(), now.cpu().numpy()) <= 2e-6
    assert ref.rel_l2(after.cpu().numpy(), vlad_eval.cpu().numpy()) > 1e-4


def test_forward_train_conv5_in_f16mx(dev, state_dict):
    B, n, images, _ = _e2e(state_dict)
    model = _model(dev, state_dict, "f16mx").eval()
    model.base_model.F16MX_MIN_TILES = 0            # f16mx whenever it can run: 12 images of 32 x 48 are below the knob
    x = images.to(dev)
    _, vlad_eval = model(x)
    runs = dict(model.base_model.precision_runs)
    _, vlad_x = model.forward_train(x, train_layers="conv5")
    assert model.base_model.precision_runs.get("f16mx", 0) == runs.get("f16mx", 0) + 1
    e = ref.rel_l2(vlad_x.detach().cpu().numpy(), vlad_eval.cpu().numpy())
    print(f"forward_train conv5 in f16mx: vlad_x against the eval forward {e:.3e}")
    assert e <= 1e-4
    ref.tuple_loss(vlad_x, B, n).backward()
    for k, v in _grads(model).items():
        assert v is not None and torch.isfinite(v).all() and float(v.abs().max()) > 0, k


def test_forward_train_refuses_deeper_layers_and_keeps_the_frozen_default(dev, state_dict):
    model = _model(dev, state_dict, "fp32")
    x = synth.images(4, 32, 48, seed=78).to(dev)
    for layers in ("conv4", "conv3", "conv2", "full"):
        with pytest.raises(NotImplementedError, match="pool4"):
            model.forward_train(x, train_layers=layers)
    _, vlad_x = model.forward_train(x)
    assert torch.equal(vlad_x, model.eval()(x)[1])
    vlad_x.sum().backward()
    assert all(p.grad is None for p in model.base_model.parameters())
    assert model.net_vlad.centroids.grad is not None and model.net_vlad.conv.weight.grad is not None
