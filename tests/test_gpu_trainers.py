"""ibl.trainers.Trainer / SFRSTrainer on the device: `_forward` against the reference's own end-to-end losses and
parameter gradients (tests/golden/conv5_backward.npz: Trainer._get_loss('triplet') on 3 tuples of 4 images;
tests/golden/region_backward.npz: SFRSTrainer._forward(..., 'triplet', gen=0) on one tuple) within those files' own
bounds, and `train(...)` for two iterations on an in-memory loader in every loss type (and both SFRS generations):
finite losses, every trainable tensor stepped, every frozen tensor bit-unchanged."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import conv_grad_ref as cref
from helpers import region_grad_ref as rref
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
