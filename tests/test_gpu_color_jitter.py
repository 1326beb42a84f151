"""The device colour jitter (csrc/augment.hip, ops.color_jitter, openibl_amd.augment.ColorJitter) against the fixture
tests/golden/color_jitter.npz — PIL's outputs (tests/helpers/make_color_jitter_golden.py) — bit for bit, in both output
kinds; run-to-run and batch-mate independence; and the trainers' `augment` path end to end."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import color_jitter_ref as ref
from openibl_amd import ops
from openibl_amd.augment import ColorJitter

pytestmark = pytest.mark.gpu

CASES = ("exact", "flat", "mean_half", "odd37x53", "odd5x7", "parts96x128", "perm24", "sweep64")


@pytest.fixture(scope="module")
def golden():
    return load_golden("color_jitter")


def _case(golden, name, dev):
    return (torch.from_numpy(golden["x_" + name]).to(dev), torch.from_numpy(golden["rec_" + name]).to(dev),
            torch.from_numpy(golden["y_" + name]))


def _mismatch(got, want):
    bad = (got != want).nonzero()
    return f"{len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


@pytest.mark.parametrize("name", CASES)
def test_uint8_output_is_pils(golden, dev, name):
    x, rec, want = _case(golden, name, dev)
    got = ops.color_jitter(x, rec, out="uint8").cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("name", CASES)
def test_float_output_is_the_host_transform_of_pils_bytes(golden, dev, name):
    x, rec, y = _case(golden, name, dev)
    want = ref.host_normalize(y)
    got = ops.color_jitter(x, rec, out="float").cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want), _mismatch(got, want)


def test_misaligned_slices_of_a_larger_buffer(golden, dev):
    """An input that starts at an odd address (a slice of a caller's buffer): every image is read by bytes.  (Outputs
    whose images start misaligned are what odd5x7 and odd37x53 have from their second image on.)"""
    x, rec, want = _case(golden, "odd37x53", dev)
    buf = torch.zeros(x.numel() + 3, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        xs = buf[off:off + x.numel()].view(x.shape)
        xs.copy_(x)
        assert xs.data_ptr() % 4 == off and torch.equal(ops.color_jitter(xs, rec, out="uint8").cpu(), want)
        assert torch.equal(ops.color_jitter(xs, rec, out="float").cpu(), ref.host_normalize(want))


def test_two_runs_give_identical_bits(golden, dev):
    for name in ("perm24", "parts96x128"):
        x, rec, _ = _case(golden, name, dev)
        for out in ("uint8", "float"):
            assert torch.equal(ops.color_jitter(x, rec, out=out), ops.color_jitter(x, rec, out=out))


def test_an_image_does_not_depend_on_its_batch_mates(golden, dev):
    x, rec, _ = _case(golden, "perm24", dev)
    whole8, wholef = ops.color_jitter(x, rec, out="uint8"), ops.color_jitter(x, rec, out="float")
    for n in range(x.shape[0]):
        assert torch.equal(ops.color_jitter(x[n:n + 1], rec[n:n + 1], out="uint8"), whole8[n:n + 1]), n
        assert torch.equal(ops.color_jitter(x[n:n + 1], rec[n:n + 1], out="float"), wholef[n:n + 1]), n
    # and not on their order
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(0)).to(dev)
    assert torch.equal(ops.color_jitter(x[perm].contiguous(), rec[perm].contiguous(), out="uint8"), whole8[perm])


def test_everything_disabled_is_the_plain_normalisation(golden, dev):
    x = torch.from_numpy(golden["x_odd37x53"]).to(dev)
    off = ColorJitter()
    got = off(x)
    assert off.last_records is None and torch.equal(got.cpu(), ref.host_normalize(x.cpu()))
    assert torch.equal(ColorJitter(out="uint8")(x), x)
    # records that skip everything are the same thing through the two-launch path
    skip = torch.full((x.shape[0], 8), -1, dtype=torch.int32, device=dev)
    assert torch.equal(ops.color_jitter(x, skip, out="float"), got)


def test_color_jitter_draws_and_replays(golden, dev):
    x = torch.from_numpy(golden["x_perm24"]).to(dev)
    jit = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(7), out="uint8")
    got = jit(x)
    rec = jit.last_records
    assert rec.shape == (24, 8) and not rec.is_cuda
    assert np.array_equal(got.cpu().numpy(), ref.model_jitter_records(golden["x_perm24"], rec.numpy()))
    assert torch.equal(jit(x, records=rec), got) and not torch.equal(jit(x), got)      # a replay; a fresh draw


# ---- the trainers --------------------------------------------------------------------------------------------------
def _model(state_dict, dev, arch, tuple_size=1):
    from ibl import models
    base = models.create("vgg16", pretrained=False, train_layers="conv5")
    pool = models.create("netvlad", dim=base.feature_dim)
    m = models.create(arch, base, pool, tuple_size=tuple_size) if arch == "embedregionnet" else \
        models.create(arch, base, pool)
    m.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    for layer in list(base.base.children())[:type(base)._fix_layers["conv5"]]:
        for p in layer.parameters():
            p.requires_grad_(False)
    return m.to(dev).set_precision("fp32").train()


def _raw_batch(B, per_tuple, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (B, per_tuple, H, W, 3), dtype=torch.uint8, generator=g)
    return imgs, [(imgs[:, j].contiguous(), ["name"] * B) for j in range(per_tuple)]


def _finite_grads(model):
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


def _replayed(jit, imgs, dev):
    """The fp32 batch ColorJitter returns for the records of its last call, and the model's word on the same bytes."""
    B, N, H, W, _ = imgs.shape
    rec = jit.last_records
    flat = imgs.view(B * N, H, W, 3)
    again = ColorJitter(0.7, 0.7, 0.7, 0.5)(flat.to(dev), records=rec)
    want = ref.host_normalize(ref.model_jitter_records(flat.numpy(), rec.numpy()))
    assert torch.equal(again.cpu(), want)
    return again.view(B, N, 3, H, W)


def test_trainer_with_augment(dev, state_dict):
    from ibl.trainers import Trainer
    B, per_tuple, H, W = 2, 4, 32, 48
    imgs, batch = _raw_batch(B, per_tuple, H, W, 60)
    model = _model(state_dict, dev, "embednet")
    jit = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(1))
    trainer = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index, augment=jit)
    inputs = trainer._parse_data(batch)
    assert inputs.shape == (B, per_tuple, 3, H, W) and inputs.dtype == torch.float32 and inputs.is_cuda
    loss = trainer._forward(inputs, True, "triplet")
    loss.backward()
    assert torch.isfinite(loss)
    _finite_grads(model)
    replay = _replayed(jit, imgs, dev)
    assert torch.equal(replay, inputs)
    model.zero_grad(set_to_none=True)
    plain = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index)
    assert plain.augment is None and float(plain._forward(replay, True, "triplet").detach()) == float(loss.detach())
    # the jitter did something: the loss of the unjittered bytes is another one
    raw = ref.host_normalize(imgs.view(-1, H, W, 3)).view(B, per_tuple, 3, H, W).to(dev)
    assert not torch.equal(raw, inputs)


def test_sfrs_trainer_with_augment(dev, state_dict):
    from ibl.trainers import SFRSTrainer
    B, neg_num, n_diff, H, W = 2, 2, 2, 64, 64
    imgs, batch = _raw_batch(B, 2 + neg_num + n_diff, H, W, 61)
    model = _model(state_dict, dev, "embedregionnet", tuple_size=B)
    cache = _model(state_dict, dev, "embedregionnet", tuple_size=B)
    trainer = SFRSTrainer(model, cache, margin=0.1 ** 0.5, neg_num=neg_num, gpu=dev.index, temp=[0.07, 0.06])
    trainer.augment = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(2))
    easy, diff = trainer._parse_data(batch)
    assert easy.shape == (B, 2 + neg_num, 3, H, W) and diff.shape == (B, 1 + n_diff, 3, H, W)
    assert torch.equal(easy[:, 0], diff[:, 0])                                 # the anchor was jittered once
    loss_hard, loss_soft = trainer._forward(easy, diff, "sare_ind", 0)
    (loss_hard + 0.5 * loss_soft).backward()
    assert torch.isfinite(loss_hard) and torch.isfinite(loss_soft)
    _finite_grads(model)
    replay = _replayed(trainer.augment, imgs, dev)
    assert torch.equal(replay[:, :neg_num + 2], easy) and torch.equal(replay[:, neg_num + 2:], diff[:, 1:])
    model.zero_grad(set_to_none=True)
    plain = SFRSTrainer(model, cache, margin=0.1 ** 0.5, neg_num=neg_num, gpu=dev.index, temp=[0.07, 0.06])
    h2, s2 = plain._forward(replay[:, :neg_num + 2], torch.cat((replay[:, :1], replay[:, neg_num + 2:]), 1),
                            "sare_ind", 0)
    assert float(h2.detach()) == float(loss_hard.detach()) and float(s2.detach()) == float(loss_soft.detach())
