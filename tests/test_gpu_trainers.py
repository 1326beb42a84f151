"""ibl.trainers.Trainer / SFRSTrainer on the device: `_forward` against the reference's own end-to-end losses and
parameter gradients (tests/golden/conv5_backward.npz: Trainer._get_loss('triplet') on 3 tuples of 4 images;
tests/golden/region_backward.npz: SFRSTrainer._forward(..., 'triplet', gen=0) on one tuple) within those files' own
bounds, and `train(...)` for two iterations on an in-memory loader in every loss type (and both SFRS generations):
finite losses, every trainable tensor stepped, every frozen tensor bit-unchanged.

End to end against tests/golden/trainer_e2e.npz (the reference's trainers in float64; tests/helpers/
make_trainer_e2e_golden.py): Trainer._forward in 'sare_ind' / 'sare_joint' on two tuples, conv5 trainable or the backbone
frozen; SFRSTrainer._forward with tuple_size 2 in every loss type at generations 0 and 1; SFRSTrainer.train for three
real optimiser steps against the reference's trajectory and against the loss stale weights would give; and, without a
reference, every later iteration of both trainers against a freshly built model in the state of that moment, and the
eval forward after training against a fresh model loaded from the trained state dict.

Measured on an MI355X (bars: a loss 1e-5 relative; a gradient min(8 ref_err, 1e-4) rel-L2; a trajectory loss
max(1e-5, 8 x the reference's own fp32-against-float64 difference), which is 1e-5 in every iteration):
  Trainer single step      loss 4.3e-08 | 6.1e-10 | 6.1e-10 (sare_ind | sare_joint | frozen); gradients 7.0e-06 .. 2.0e-05,
                           bars 3.5e-05 .. 6.7e-05, at most 0.51 of a bar (sare_joint dW2 2.00e-05 of 3.94e-05)
  SFRSTrainer single step  loss_hard 2.0e-07 | 6.0e-08 | 4.7e-08 (triplet | sare_ind | sare_joint, either generation),
                           loss_soft 2.1e-08 (gen 0) | 4.9e-08 (gen 1); gradients 3.2e-06 .. 1.6e-05, bars 1.8e-05 .. 9.9e-05,
                           at most 0.36 of a bar (sare_ind gen 0 dW2 9.51e-06 of 2.66e-05); regions picked [[0, 0], [0, 0]]
  SFRSTrainer three steps  lr 1e-1; loss_hard 2.0e-07 | 1.4e-07 | 1.1e-07, loss_soft 4.9e-08 | 8.7e-08 | 7.6e-08, their
                           sum 3.8e-09 | 9.9e-08 | 8.4e-08; the stale loss 1372 and 2928 bars away in iterations 2 and 3
  fresh model, that state  bit-equal in iterations 2 and 3 of both trainers; from the initial state 2.9e-04 | 1.4e-04
                           (Trainer, lr 1e-1) and 1.4e-02 | 2.9e-02 (SFRSTrainer) away; eval forward after training
                           bit-equal to the fresh model's, descriptors moved by 0.14 | 0.64 rel-L2
The fixture holds no Trainer trajectory and no parameter updates: the reference does not meet the conditions set for
them (the generator's docstring has the figures); the fresh-model test covers the later steps of Trainer."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import conv_grad_ref as cref
from helpers import region_grad_ref as rref
from helpers import trainer_e2e_ref as eref
from openibl_amd import ops, synth

pytestmark = pytest.mark.gpu

K, C = 64, 512
E2E_KEYS = ("dW1", "dW2", "dW3", "db1", "db2", "db3", "dWv", "dCv")


def _model(state_dict, dev, arch, tuple_size=1, train_layers="conv5", freeze_backbone=False):
    from ibl import models
    base = models.create("vgg16", pretrained=False, train_layers=train_layers)
    pool = models.create("netvlad", dim=base.feature_dim)
    m = models.create(arch, base, pool, tuple_size=tuple_size) if arch == "embedregionnet" else \
        models.create(arch, base, pool)
    m.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    # what VGG.__init__ does with pretrained weights: the layers below train_layers are frozen (base[:24] for 'conv5')
    frozen = list(base.parameters()) if freeze_backbone else \
        [p for l in list(base.base.children())[:type(base)._fix_layers[train_layers]] for p in l.parameters()]
    for p in frozen:
        p.requires_grad_(False)
    return m.to(dev).set_precision("fp32")


def _grads(model):
    b, nv = model.base_model.base, model.net_vlad
    out = {"dWv": nv.conv.weight.grad.reshape(K, C), "dCv": nv.centroids.grad}
    for i, li in enumerate((24, 26, 28)):
        out[f"dW{i + 1}"], out[f"db{i + 1}"] = b[li].weight.grad, b[li].bias.grad
    return {k: v.cpu().numpy() for k, v in out.items()}


class _Wrapped(torch.nn.Module):
    """A `.module` container, as DataParallel / DistributedDataParallel are."""

    def __init__(self, module):
        super().__init__()
        self.module = module


def test_trainer_forward_reproduces_the_reference_end_to_end(dev, state_dict):
    from ibl.trainers import Trainer
    g = load_golden("conv5_backward")
    B, n, H, W = map(int, g["e2e_shape"])
    images = synth.images(B * n, H, W, seed=int(g["e2e_seed"])).to(dev)
    model = _model(state_dict, dev, "embednet").train()
    trainer = Trainer(_Wrapped(model), margin=0.1 ** 0.5)
    loss = trainer._forward(images.view(B, n, 3, H, W), True, "triplet")
    loss.backward()
    want = float(g["e2e_loss"])
    print(f"Trainer._forward: loss {float(loss):.9f}, the reference's {want:.9f}")
    assert abs(float(loss) - want) <= 1e-5 * want
    got, ref_err = _grads(model), dict(zip(cref.E2E_KEYS, g["e2e_ref_err"]))
    hs = int(g["e2e_head_stride"])
    for k in cref.E2E_KEYS:
        part = got[k][:cref.W_ROWS] if k in ("dW1", "dW2", "dW3") else got[k][::hs] if k in ("dWv", "dCv") else got[k]
        bar = min(8.0 * float(ref_err[k]), 1e-4) + float(ref_err[k])
        e = cref.rel_l2(part, g[f"e2e_{k}"])
        print(f"  {k} against the reference's fp32 autograd {e:.3e} (bar {bar:.2e})")
        assert np.isfinite(got[k]).all() and e <= bar, (k, e, bar)
    trunk = [p for i in range(24) for p in model.base_model.base[i].parameters()]
    assert len(trunk) == 20 and all(p.grad is None for p in trunk)
    # the same loss from the frozen-backbone path's graph: train_layers is derived as None
    for p in model.base_model.parameters():
        p.requires_grad_(False)
    model.zero_grad(set_to_none=True)
    trainer._forward(images.view(B, n, 3, H, W), True, "triplet").backward()
    assert model.net_vlad.centroids.grad is not None and all(p.grad is None for p in model.base_model.parameters())
    with pytest.raises(NotImplementedError, match="pool_x"):
        trainer._forward(images.view(B, n, 3, H, W), False, "triplet")
    with pytest.raises(ValueError, match="loss_type"):
        trainer._forward(images.view(B, n, 3, H, W), True, "contrastive")


def test_sfrs_trainer_forward_reproduces_the_reference_end_to_end(dev, state_dict):
    from ibl.trainers import SFRSTrainer
    g = load_golden("region_backward")
    n_img, H, W, neg_num = map(int, g["e2e_shape"])
    images = synth.images(n_img, H, W, seed=int(g["e2e_seed"])).to(dev)
    model = _model(state_dict, dev, "embedregionnet").train()
    cache = _model(state_dict, dev, "embedregionnet").train()      # generation 0: model_cache is a copy of the student
    trainer = SFRSTrainer(model, cache, margin=0.1 ** 0.5, neg_num=neg_num, temp=[0.07, 0.07])
    easy, diff = images[None, :neg_num + 2], torch.cat([images[None, :1], images[None, neg_num + 2:]], dim=1)
    loss_hard, loss_soft = trainer._forward(easy, diff, "triplet", 0)
    (loss_hard + 0.5 * loss_soft).backward()
    want_h, want_s = map(float, g["e2e64_losses"])
    print(f"SFRSTrainer._forward: loss_hard {float(loss_hard):.9f} (float64 {want_h:.9f}), loss_soft "
          f"{float(loss_soft):.9f} (float64 {want_s:.9f})")
    assert abs(float(loss_hard) - want_h) <= 1e-5 * want_h and abs(float(loss_soft) - want_s) <= 1e-5 * want_s
    got, ref_err = _grads(model), dict(zip(E2E_KEYS, g["e2e_ref_err"]))
    rows, hs = int(g["e2e_w_rows"]), int(g["e2e_head_stride"])
    for k in E2E_KEYS:
        part = got[k][:rows] if k in ("dW1", "dW2", "dW3") else got[k][::hs] if k in ("dWv", "dCv") else got[k]
        bar = min(8.0 * float(ref_err[k]), 1e-4)
        e64, e32 = rref.rel_l2(part, g[f"e2e64_{k}"]), rref.rel_l2(part, g[f"e2e_{k}"])
        print(f"  {k} {e64:.3e} (bar {bar:.2e}); against the reference's fp32 autograd {e32:.3e}")
        assert np.isfinite(got[k]).all() and e64 <= bar and e32 <= bar + float(ref_err[k]), (k, e64, e32, bar)
    assert all(p.grad is None for p in cache.parameters())


def _loader(B, per_tuple, H, W, seed, batches=2):
    """An in-memory loader: per batch one entry per tuple position, (images [B][3][H][W], file names, ...)."""
    from ibl.utils.data import IterLoader
    data = []
    for i in range(batches):
        imgs = synth.images(B * per_tuple, H, W, seed=seed + i).view(B, per_tuple, 3, H, W)
        data.append([(imgs[:, j].contiguous(), [f"{i}_{j}"] * B) for j in range(per_tuple)])
    return IterLoader(data, length=batches)


def _snapshot(*models):
    return [{k: v.detach().clone() for k, v in m.named_parameters()} for m in models]


def _check_step(model, before, capsys, pattern):
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert trainable and len(trainable) < len(before)
    for k, p in model.named_parameters():
        assert torch.isfinite(p).all(), k
        assert torch.equal(p.detach(), before[k]) != (k in trainable), k
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch: [3-1]")]
    assert len(lines) == 2 and lines[1].startswith("Epoch: [3-1][2/2]\tTime ") and pattern in lines[1], lines
    import re
    return [float(v) for ln in lines for v in re.findall(r"Loss\w* (\S+) \(", ln)]


@pytest.mark.parametrize("loss_type,frozen", [("triplet", False), ("sare_ind", True), ("sare_joint", False)])
def test_trainer_train_steps_the_trainable_tensors_only(dev, state_dict, capsys, loss_type, frozen):
    from ibl.trainers import Trainer
    model = _model(state_dict, dev, "embednet", freeze_backbone=frozen)
    before = _snapshot(model)[0]
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    trainer = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index)
    trainer.train(3, 1, _loader(2, 4, 32, 48, seed=40), opt, 2, print_freq=1, vlad=True, loss_type=loss_type)
    assert model.training
    losses = _check_step(model, before, capsys, "\tLoss ")
    assert len(losses) == 2 and all(np.isfinite(losses)) and all(v > 0 for v in losses)
    assert len({k for k, p in model.named_parameters() if p.requires_grad}) == (2 if frozen else 8)


@pytest.mark.parametrize("gen", [0, 1])
@pytest.mark.parametrize("loss_type", ["triplet", "sare_ind", "sare_joint"])
def test_sfrs_trainer_train_steps_the_student_only(dev, state_dict, capsys, monkeypatch, loss_type, gen):
    from ibl.trainers import SFRSTrainer
    B, neg_num, n_diff = 2, 2, 2
    model = _model(state_dict, dev, "embedregionnet", tuple_size=B, freeze_backbone=(loss_type == "sare_ind"))
    cache = _model(state_dict, dev, "embedregionnet", tuple_size=B)
    before, cache_before = _snapshot(model, cache)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    trainer = SFRSTrainer(model, cache, margin=0.1 ** 0.5, neg_num=neg_num, gpu=dev.index, temp=[0.07, 0.06])
    loader = _loader(B, 2 + neg_num + n_diff, 64, 64, seed=50)

    # what the first iteration must select at generation 1: the argmax of the detached scores of the student as it stands
    first = torch.stack([item[0] for item in loader.loader[0]]).permute(1, 0, 2, 3, 4)[:, :neg_num + 2].to(dev)
    with torch.no_grad():
        sim_easy, _, vlad_pairs = model.train().forward_train(first.reshape(-1, 3, 64, 64),
                                                              train_layers=None if loss_type == "sare_ind" else "conv5")
    arg = sim_easy[:, 1:, 0].argmax(-1)
    expect = vlad_pairs[torch.arange(B, device=dev)[:, None], 1 + torch.arange(neg_num, device=dev)[None, :], arg]
    seen = []
    real = ops.tuple_loss

    def spy(anchors, positives, negatives, kind, **kw):
        seen.append((negatives.detach().clone(), kind, kw))
        return real(anchors, positives, negatives, kind, **kw)

    monkeypatch.setattr(ops, "tuple_loss", spy)
    trainer.train(gen, 3, 1, loader, opt, 2, print_freq=1, lambda_soft=0.5, loss_type=loss_type)
    assert len(seen) == 2 and seen[0][1] == loss_type and seen[0][2]["score"] == "dot"
    if gen == 1:
        assert torch.equal(trainer.hard_regions(sim_easy[:, 1:, 0]), arg)
        assert torch.equal(seen[0][0], expect)
        print("regions chosen at generation 1:", arg.tolist())
    else:
        assert torch.equal(seen[0][0], vlad_pairs[:, 1:, 0])
    losses = _check_step(model, before, capsys, "\tLoss_hard ")
    assert len(losses) == 4 and all(np.isfinite(losses))
    for k, p in cache.named_parameters():
        assert torch.equal(p.detach(), cache_before[k]), k


def test_deeper_train_layers_raise_from_forward_train(dev, state_dict):
    from ibl.trainers import Trainer
    model = _model(state_dict, dev, "embednet", train_layers="conv4")
    x = synth.images(4, 32, 48, seed=3).to(dev).view(1, 4, 3, 32, 48)
    with pytest.raises(NotImplementedError, match="pool4"):
        Trainer(model)._forward(x, True, "triplet")


# ---- end to end against tests/golden/trainer_e2e.npz: every loss, two tuples, generation 1, three steps -------------
# (the figures measured on the MI355X stand in the docstrings below and in DESIGN 4.5)

@pytest.fixture(scope="module")
def e2e():
    return load_golden("trainer_e2e")


def _spy_forward_train(model):
    """Record the train_layers every forward_train call of `model` receives."""
    seen, real = [], model.forward_train

    def spy(x, train_layers=None):
        seen.append(train_layers)
        return real(x, train_layers=train_layers)

    model.forward_train = spy
    return seen


def _check_e2e_loss(label, got, want, bar=1e-5):
    e = abs(got - want) / abs(want)
    print(f"  {label} {got:.9f} (float64 {want:.9f}) {e:.3e} (bar {bar:.2e})")
    assert np.isfinite(got) and e <= bar, (label, got, want, e, bar)


def _check_e2e_grads(g, name, got, keys):
    ref_err, rows, hs = dict(zip(keys, g[f"{name}_ref_err"])), int(g["w_rows"]), int(g["head_stride"])
    for k in keys:
        bar = min(8.0 * float(ref_err[k]), 1e-4)
        e = rref.rel_l2(eref.part(k, got[k], rows, hs), g[f"{name}_{k}"])
        print(f"  {k} {e:.3e} (bar {bar:.2e})")
        assert np.isfinite(got[k]).all() and e <= bar, (name, k, e, bar)


@pytest.mark.parametrize("name", list(eref.SINGLE_TRAINER))
def test_trainer_single_step_against_the_reference(dev, state_dict, e2e, name):
    """Trainer._forward on 2 tuples of 4 images (32 x 48) in 'sare_ind' and 'sare_joint', conv5 trainable or the whole
    backbone frozen: the loss within 1e-5 of the reference's float64 loss, every gradient within min(8 ref_err, 1e-4)
    rel-L2 of the float64 sample.  Measured: the module docstring and DESIGN 4.5."""
    from ibl.trainers import Trainer
    loss_type, frozen = eref.SINGLE_TRAINER[name]
    model = _model(state_dict, dev, "embednet", freeze_backbone=frozen).train()
    seen = _spy_forward_train(model)
    loss = Trainer(_Wrapped(model), margin=eref.MARGIN)._forward(eref.batch(eref.TRAINER_SHAPE, 0).to(dev), True, loss_type)
    loss.backward()
    assert seen == [None if frozen else "conv5"]
    print(name)
    _check_e2e_loss("loss", float(loss), float(e2e[f"{name}_losses"][0]))
    nv, base = model.net_vlad, model.base_model
    if frozen:
        assert all(p.grad is None for p in base.parameters())
        got = {"dWv": nv.conv.weight.grad.reshape(K, C).cpu().numpy(), "dCv": nv.centroids.grad.cpu().numpy()}
        _check_e2e_grads(e2e, name, got, eref.HEAD_KEYS)
    else:
        trunk = [p for i in range(24) for p in base.base[i].parameters()]
        assert len(trunk) == 20 and all(p.grad is None for p in trunk)
        _check_e2e_grads(e2e, name, _grads(model), eref.KEYS)


def _sfrs_pair(state_dict, dev):
    B = eref.SFRS_SHAPE["B"]
    model = _model(state_dict, dev, "embedregionnet", tuple_size=B).train()
    cache = _model(state_dict, dev, "embedregionnet", tuple_size=B).train()    # model_cache: a copy of the student
    return model, cache


@pytest.mark.parametrize("name", list(eref.SINGLE_SFRS))
def test_sfrs_trainer_single_step_against_the_reference(dev, state_dict, e2e, name):
    """SFRSTrainer._forward with tuple_size = 2 (neg_num 2, two difficult positives, 64 x 96, temp [0.07, 0.06]) in
    every loss type at generations 0 and 1, loss_hard + 0.5 loss_soft differentiated: both losses within 1e-5 of the
    reference's float64 losses (the reference run tuple by tuple), every gradient within min(8 ref_err, 1e-4), the
    regions picked at generation 1 the reference's, model_cache untouched.  Measured: the module docstring and DESIGN 4.5."""
    from ibl.trainers import SFRSTrainer
    loss_type, gen = eref.SINGLE_SFRS[name]
    s = eref.SFRS_SHAPE
    model, cache = _sfrs_pair(state_dict, dev)
    cache_before = _snapshot(cache)[0]
    trainer = SFRSTrainer(model, cache, margin=eref.MARGIN, neg_num=s["neg_num"], temp=eref.TEMP)
    easy, diff = (t.to(dev) for t in eref.split(eref.batch(s, 0), s["neg_num"]))
    if gen == 1:
        with torch.no_grad():
            sim_easy, _, _ = model.forward_train(easy.reshape(-1, 3, s["H"], s["W"]), train_layers="conv5")
        picks = trainer.hard_regions(sim_easy[:, 1:, 0]).cpu().numpy()
        print("regions picked:", picks.tolist())
        assert np.array_equal(picks, e2e[f"{name}_picks"])
    seen = _spy_forward_train(model)
    loss_hard, loss_soft = trainer._forward(easy, diff, loss_type, gen)
    (loss_hard + eref.LAMBDA_SOFT * loss_soft).backward()
    assert seen == ["conv5", "conv5"]
    print(name)
    _check_e2e_loss("loss_hard", float(loss_hard), float(e2e[f"{name}_losses"][0]))
    _check_e2e_loss("loss_soft", float(loss_soft), float(e2e[f"{name}_losses"][1]))
    _check_e2e_grads(e2e, name, _grads(model), eref.KEYS)
    trunk = [p for i in range(24) for p in model.base_model.base[i].parameters()]
    assert len(trunk) == 20 and all(p.grad is None for p in trunk)
    for k, p in cache.named_parameters():
        assert p.grad is None and torch.equal(p.detach(), cache_before[k]), k


_trained = {}


def _train_three(kind, dev, state_dict, lr):
    """Three iterations of the project's real train() on an in-memory loader with the scripts' optimiser, once per
    module: the unrounded losses of every _forward, the state dict the model had when each _forward began, and the
    eval-mode output on the first batch before training (which also leaves the inference path's packed copies of the
    initial weights in the model: what a stale cache would serve afterwards)."""
    if kind in _trained:
        return _trained[kind]
    from ibl.trainers import SFRSTrainer, Trainer
    if kind == "trainer":
        s, loss_type = eref.TRAINER_SHAPE, "sare_ind"
        model = _model(state_dict, dev, "embednet")
        cache = None
        trainer = Trainer(model, margin=eref.MARGIN, gpu=dev.index)
    else:
        s, loss_type = eref.SFRS_SHAPE, "triplet"
        model, cache = _sfrs_pair(state_dict, dev)
        trainer = SFRSTrainer(model, cache, margin=eref.MARGIN, neg_num=s["neg_num"], gpu=dev.index, temp=eref.TEMP)
    x = eref.batch(s, 0)[:, :4].reshape(-1, 3, s["H"], s["W"]).contiguous().to(dev)
    before = [t.clone() for t in model.eval()(x)]
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=lr, momentum=eref.MOMENTUM,
                          weight_decay=eref.WEIGHT_DECAY)
    losses, states, real = [], [], trainer._forward

    def record(*args):
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        out = real(*args)
        losses.append([float(v) for v in (out if isinstance(out, tuple) else (out,))])
        return out

    trainer._forward = record
    loader = _loader(s["B"], eref.per_tuple(s), s["H"], s["W"], seed=s["seed"], batches=eref.ITERS)
    if kind == "trainer":
        trainer.train(3, 1, loader, opt, eref.ITERS, print_freq=1, vlad=True, loss_type=loss_type)
    else:
        trainer.train(1, 3, 1, loader, opt, eref.ITERS, print_freq=1, lambda_soft=eref.LAMBDA_SOFT, loss_type=loss_type)
    trainer._forward = real
    _trained[kind] = dict(model=model, cache=cache, trainer=trainer, losses=np.array(losses), states=states, x=x,
                          before=before, shape=s, loss_type=loss_type)
    return _trained[kind]


def _total(losses):
    return losses[:, 0] if losses.shape[1] == 1 else losses[:, 0] + eref.LAMBDA_SOFT * losses[:, 1]


def test_sfrs_trainer_three_steps_against_the_reference(dev, state_dict, e2e):
    """SFRSTrainer.train for three iterations ('triplet', generation 1, lambda_soft 0.5, SGD momentum 0.9, weight decay
    1e-3, the stored lr) against the reference's float64 trajectory: loss_hard, loss_soft and their weighted sum of
    every iteration within max(1e-5, 8 x the reference's own fp32-against-float64 difference); and iterations 2 and 3
    more than 10 bars away from the loss the INITIAL weights give on their batches (the fixture keeps them >= 100 bars
    apart): a step that read stale copies of the weights fails here.  Measured: the module docstring and DESIGN 4.5."""
    name = "traj_sfrs"
    run = _train_three("sfrs", dev, state_dict, float(e2e[f"{name}_lr"]))
    got, l64, l32, stale = run["losses"], e2e[f"{name}_losses"], e2e[f"{name}_losses32"], e2e[f"{name}_stale"]
    assert got.shape == l64.shape == (eref.ITERS, 2)
    for i in range(eref.ITERS):
        print(f"iteration {i + 1}")
        for j, label in enumerate(("loss_hard", "loss_soft")):
            _check_e2e_loss(label, got[i, j], l64[i, j], max(1e-5, 8.0 * abs(l32[i, j] - l64[i, j]) / l64[i, j]))
        t, t64, t32, ts = _total(got)[i], _total(l64)[i], _total(l32)[i], _total(stale)[i]
        bar = max(1e-5, 8.0 * abs(t32 - t64) / t64)
        _check_e2e_loss("loss", t, t64, bar)
        if i:
            away = abs(t - ts) / (bar * t64)
            print(f"  the stale loss {ts:.9f} is {away:.0f} bars away")
            assert away > 10.0, (i, t, ts, away)
    for k, p in run["cache"].named_parameters():
        assert p.grad is None and torch.equal(p.detach(), run["states"][0][k]), k


@pytest.mark.parametrize("kind", ["trainer", "sfrs"])
def test_every_step_and_the_eval_forward_read_the_stepped_weights(dev, state_dict, e2e, kind):
    """No reference needed: after real optimiser steps (lr 1e-1 for Trainer 'sare_ind', the stored lr for SFRS), the
    loss train() computed in iterations 2 and 3 is the loss a FRESHLY built model gives on that batch from the state
    dict of that moment (same kernels, same weights: 1e-6 covers an order of summation), and is more than ten times
    that away from what the fresh model gives from the initial weights.  Then, in eval(): model(x) is bit-equal to a
    fresh model loaded from the trained state_dict(), and both differ from the output before training — the packed
    and cast copies of the inference path were rebuilt."""
    from ibl.trainers import SFRSTrainer, Trainer
    run = _train_three(kind, dev, state_dict, 1e-1 if kind == "trainer" else float(e2e["traj_sfrs_lr"]))
    s, arch = run["shape"], "embednet" if kind == "trainer" else "embedregionnet"
    got = _total(run["losses"])

    def fresh_loss(state, i):
        m = _model(state, dev, arch, tuple_size=s["B"]).train()
        imgs = eref.batch(s, i)
        with torch.no_grad():
            if kind == "trainer":
                return float(Trainer(m, margin=eref.MARGIN)._forward(imgs.to(dev), True, run["loss_type"]))
            c = _model(run["states"][0], dev, arch, tuple_size=s["B"]).train()
            t = SFRSTrainer(m, c, margin=eref.MARGIN, neg_num=s["neg_num"], temp=eref.TEMP)
            easy, diff = (v.to(dev) for v in eref.split(imgs, s["neg_num"]))
            hard, soft = t._forward(easy, diff, run["loss_type"], 1)
            return float(hard) + eref.LAMBDA_SOFT * float(soft)

    for i in (1, 2):
        live, stale = fresh_loss(run["states"][i], i), fresh_loss(run["states"][0], i)
        e, away = abs(got[i] - live) / abs(live), abs(got[i] - stale) / abs(live)
        print(f"{kind} iteration {i + 1}: train() {got[i]:.9f}, fresh model from that state {live:.9f} ({e:.2e}), "
              f"from the initial state {stale:.9f} ({away:.2e})")
        assert e <= 1e-6 and away > 1e-5, (i, got[i], live, stale)

    model = run["model"].eval()
    after = model(run["x"])
    twin = _model(model.state_dict(), dev, arch, tuple_size=s["B"]).eval()
    for a, b, c in zip(after, twin(run["x"]), run["before"]):
        assert torch.isfinite(a).all() and torch.equal(a, b) and not torch.equal(a, c)
    print(f"{kind}: descriptors moved by {float((after[1] - run['before'][1]).norm() / run['before'][1].norm()):.3e}")
