"""Training tuples from the files' bytes on the device: ops.decode_jitter_resize_jpeg against Pillow's decode ->
jitter -> resize (tests/golden/train_input.npz), augment.Compose(DecodeJpeg(), ColorJitter(...), Resize(...)), and the
trainers' branch for `jpeg.collate_tuples` batches — `_parse_data` against the per-image chain, `train` with and
without prefetch, a damaged file.  Every comparison is bit equality."""
import functools
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import color_jitter_ref as cj
from openibl_amd import jpeg, ops
from openibl_amd.augment import ColorJitter, Compose, DecodeJpeg, Resize

pytestmark = pytest.mark.gpu

NAMES = ("37x53_420", "48x64_grey", "64x48_422", "9x8_444", "120x160_420", "120x160_420_rstrow", "640x16_420",
         "40x56_progressive", "24x30_png")
FIT = tuple(n for n in NAMES if n != "640x16_420")        # 640 rows -> 32 is beyond the resize's limit of 16


@pytest.fixture(scope="module")
def mixed():
    return load_golden("jpeg_mixed")


@pytest.fixture(scope="module")
def golden():
    return load_golden("train_input")


def batch_of(mixed, dev, names=NAMES):
    return jpeg.MixedJpegBatch.from_files([mixed["s_" + n] for n in names]).to(dev)


def records_of(golden, dev, names=NAMES):
    return torch.from_numpy(golden["records"][[NAMES.index(n) for n in names]]).to(dev)


# ---- the chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan,chunk_bytes", [("auto", None), ("serial", None), ("chunked", 16)])
def test_chain_is_pillows_decode_jitter_resize_on_all_nine_files(mixed, golden, dev, scan, chunk_bytes):
    """All nine files, the two of the host route included, to 48 x 32; the eight a height of 32 admits to 32 x 48."""
    for key, size, names in (("u", (48, 32), NAMES), ("t", (32, 48), FIT)):
        u8, status = ops.decode_jitter_resize_jpeg(batch_of(mixed, dev, names), records_of(golden, dev, names), size,
                                                   out="uint8", check=False, scan=scan, chunk_bytes=chunk_bytes)
        assert u8.shape == (len(names), *size, 3) and u8.dtype == torch.uint8
        assert status.dtype == torch.int32 and status.tolist() == [0] * len(names)
        got = u8.cpu().numpy()
        for i, n in enumerate(names):
            assert np.array_equal(got[i], golden[f"{key}_{n}"]), (key, n, scan)
    with pytest.raises(ValueError, match=r"image 6 is 640 x 16.*32 x 48.*limit of 16"):
        ops.decode_jitter_resize_jpeg(batch_of(mixed, dev), records_of(golden, dev), (32, 48))


def test_float_output_is_the_normalised_bytes_and_none_is_the_plain_resize(mixed, golden, dev):
    b, rec = batch_of(mixed, dev), records_of(golden, dev)
    u8 = ops.decode_jitter_resize_jpeg(b, rec, (48, 32), out="uint8")
    fl = ops.decode_jitter_resize_jpeg(b, rec, (48, 32))                       # out='float', check=True
    assert fl.shape == (9, 3, 48, 32) and fl.dtype == torch.float32
    assert torch.equal(fl.cpu(), cj.host_normalize(u8.cpu()))
    assert torch.equal(fl, ops.color_jitter(u8, None, out="float"))
    plain = ops.decode_jitter_resize_jpeg(b, None, (48, 32), out="uint8")
    assert torch.equal(plain, ops.decode_resize_jpeg(b, (48, 32), out="uint8"))
    assert not torch.equal(plain, u8)


def test_a_batch_of_one_size_takes_the_uniform_calls(mixed, golden, dev):
    names = ("120x160_420", "120x160_420_rstrow")
    b = jpeg.JpegBatch.from_files([mixed["s_" + n] for n in names]).to(dev)
    rec = records_of(golden, dev, names)
    got, status = ops.decode_jitter_resize_jpeg(b, rec, (32, 48), out="uint8", check=False)
    want = ops.resize_u8(ops.color_jitter(ops.decode_jpeg(b), rec, out="uint8"), (32, 48), out="uint8")
    assert status.tolist() == [0, 0] and torch.equal(got, want)
    for i, n in enumerate(names):
        assert np.array_equal(got[i].cpu().numpy(), golden["t_" + n])
    assert torch.equal(ops.decode_jitter_resize_jpeg(b, rec, (32, 48)), ops.color_jitter(want, None, out="float"))


def test_a_truncated_file_gives_its_status_and_check_names_it(mixed, golden, dev):
    base = mixed["s_120x160_420"]
    cut = base[:jpeg.parse(base).scan_begin + 3000]
    files = [mixed["s_" + n] for n in NAMES]
    files[4] = cut
    b = jpeg.MixedJpegBatch.from_files(files).to(dev)
    u8, status = ops.decode_jitter_resize_jpeg(b, records_of(golden, dev), (48, 32), out="uint8", check=False)
    assert status.tolist() == [0, 0, 0, 0, jpeg.ST_OUT_OF_BYTES, 0, 0, 0, 0]
    got = u8.cpu().numpy()
    for i, n in enumerate(NAMES):
        if i != 4:
            assert np.array_equal(got[i], golden["u_" + n]), n                 # the batch mates are not affected
    with pytest.raises(ValueError, match=r"decode_jitter_resize_jpeg: damaged JPEG streams: image 4 \(ran out of bytes\)"):
        ops.decode_jitter_resize_jpeg(b, records_of(golden, dev), (48, 32))


# ---- augment --------------------------------------------------------------------------------------------------------
def test_compose_from_the_bytes_replays_its_records_and_equals_the_ops_chain(mixed, dev):
    jitter = ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8", generator=torch.Generator().manual_seed(21))
    chain = Compose(DecodeJpeg(), jitter, Resize(32, 48))
    b = batch_of(mixed, dev, FIT)
    first = chain(b)
    rec = jitter.last_records
    assert first.shape == (8, 3, 32, 48) and first.dtype == torch.float32 and rec.shape == (8, 8) and not rec.is_cuda
    assert chain.stages[0].last_status.tolist() == [0] * 8
    again = chain(b, records=rec)                                              # the keyword reaches the jitter stage
    assert torch.equal(again, first) and jitter.last_records is rec
    assert torch.equal(first, ops.decode_jitter_resize_jpeg(b, rec.to(dev), (32, 48)))
    other = chain(b)                                                           # new draws: another batch
    assert not torch.equal(other, first) and not torch.equal(jitter.last_records, rec)
    # uint8 out of the last stage, and a batch of one size through the same chain
    u8 = Compose(DecodeJpeg(scan="serial"), jitter, Resize(32, 48, out="uint8"))(b, records=rec)
    assert torch.equal(ops.color_jitter(u8, None, out="float"), first)
    names = ("120x160_420", "120x160_420_rstrow")
    same = jpeg.JpegBatch.from_files([mixed["s_" + n] for n in names]).to(dev)
    assert torch.equal(chain(same, records=rec[:2]), ops.decode_jitter_resize_jpeg(same, rec[:2].to(dev), (32, 48)))
    with pytest.raises(ValueError, match="keep_aspect"):
        Compose(DecodeJpeg(), jitter, Resize(32, 48, keep_aspect=True))(b)


# ---- the trainers ---------------------------------------------------------------------------------------------------
TRAIN_FILES = ("37x53_420", "48x64_grey", "64x48_422", "120x160_420", "120x160_420_rstrow", "40x56_progressive",
               "24x30_png", "9x8_444")           # seven stored sizes, two files of the host route


def _write(mixed, folder, count):
    """`count` files f0.jpg .. in `folder`, cycling through TRAIN_FILES shifted by one per round -> the record list."""
    records = []
    for k in range(count):
        name = TRAIN_FILES[(k + k // len(TRAIN_FILES)) % len(TRAIN_FILES)]
        (folder / f"f{k}.jpg").write_bytes(mixed["s_" + name].tobytes())
        records.append((f"f{k}.jpg", k, 0.5 * k, 1.0, name))
    return records


def _loader(records, folder, B, N, batches, target):
    from torch.utils.data import DataLoader
    from ibl.utils.data import IterLoader
    from ibl.utils.data.preprocessor import Preprocessor
    plan = [[list(range((i * B + b) * N, (i * B + b + 1) * N)) for b in range(B)] for i in range(batches)]
    data = Preprocessor([r[:4] for r in records], root=str(folder), raw=True)
    return IterLoader(DataLoader(data, batch_sampler=plan, num_workers=0, pin_memory=True,
                                 collate_fn=functools.partial(jpeg.collate_tuples, target=target)), length=batches)


def _per_image(mixed, records, rec, size, dev):
    """Pillow's decode -> ops.color_jitter -> ops.resize_u8(out='float') of every file on its own."""
    out = []
    for i, r in enumerate(records):
        x = torch.from_numpy(mixed["y_" + r[4]])[None].to(dev)
        out.append(ops.resize_u8(ops.color_jitter(x, rec[i:i + 1].to(dev), out="uint8"), size, out="float")[0])
    return torch.stack(out)


def test_trainers_parse_a_batch_of_file_bytes_like_the_per_image_chain(mixed, dev, tmp_path):
    from ibl.trainers import SFRSTrainer, Trainer
    B, N = 2, 4
    records = _write(mixed, tmp_path, B * N)
    assert len({mixed["y_" + r[4]].shape for r in records}) >= 4               # four stored sizes and more
    jitter = ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8", generator=torch.Generator().manual_seed(31))
    trainer = Trainer(None, gpu=dev.index, augment=Compose(DecodeJpeg(), jitter, Resize(32, 48)))
    loader = _loader(records, tmp_path, B, N, 1, (32, 48))
    loader.new_epoch()
    batch = loader.next()
    assert batch[0].tuples == (B, N) and jpeg.tuple_names(batch) == [r[0] for r in records]
    got = trainer._parse_data(batch)
    assert got.shape == (B, N, 3, 32, 48) and got.dtype == torch.float32 and got.device == dev
    want = _per_image(mixed, records, jitter.last_records, (32, 48), dev)
    assert torch.equal(got.reshape(B * N, 3, 32, 48), want)
    host, names = trainer._files.popleft()
    torch.cuda.synchronize(dev)
    assert host.is_pinned() and host.tolist() == [0] * 8 and names == [r[0] for r in records]

    # SFRS: anchor, positive, one negative, one difficult positive; every image jittered once
    sfrs = SFRSTrainer(None, None, neg_num=1, gpu=dev.index, augment=Compose(DecodeJpeg(), jitter, Resize(32, 64)))
    loader = _loader(records, tmp_path, B, N, 1, (32, 64))
    loader.new_epoch()
    easy, diff = sfrs._parse_data(loader.next())
    want = _per_image(mixed, records, jitter.last_records, (32, 64), dev).view(B, N, 3, 32, 64)
    assert easy.shape == (B, 3, 3, 32, 64) and diff.shape == (B, 2, 3, 32, 64)
    assert torch.equal(easy, want[:, :3]) and torch.equal(diff[:, 1:], want[:, 3:])
    assert torch.equal(diff[:, 0], easy[:, 0]) and torch.equal(diff[:, 0], want[:, 0])     # the anchor is shared


def _model(state_dict, dev):
    from ibl import models
    base = models.create("vgg16", pretrained=False, train_layers="conv5")
    m = models.create("embednet", base, models.create("netvlad", dim=base.feature_dim))
    m.load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pca_layer")})
    for layer in list(base.base.children())[:type(base)._fix_layers["conv5"]]:
        for p in layer.parameters():
            p.requires_grad_(False)
    return m.to(dev).set_precision("fp32")


def _train(mixed, state_dict, dev, folder, prefetch, capsys, iters=3):
    from ibl.trainers import Trainer
    B, N = 2, 4
    records = _write(mixed, folder, B * N * iters)
    model = _model(state_dict, dev)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    jitter = ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8", generator=torch.Generator().manual_seed(41))
    trainer = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index, prefetch=prefetch,
                      augment=Compose(DecodeJpeg(), jitter, Resize(32, 48)))
    exact, real = [], trainer._forward

    def forward(*a, **k):       # the loss tensors themselves, kept without a synchronisation
        exact.append(real(*a, **k))
        return exact[-1]
    trainer._forward = forward
    capsys.readouterr()
    trainer.train(5, 1, _loader(records, folder, B, N, iters, (32, 48)), opt, iters, print_freq=1)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch: [5-1]")]
    printed = [re.search(r"Loss (\S+) \(", ln).group(1) for ln in lines]
    losses = torch.stack([v.detach() for v in exact]).cpu()
    assert [f"{float(v):.3f}" for v in losses] == printed
    return losses, {k: v.detach().clone() for k, v in model.named_parameters()}, jitter.last_records


def test_three_steps_give_the_same_bits_with_and_without_prefetch(mixed, state_dict, dev, tmp_path, capsys):
    (tmp_path / "a").mkdir(), (tmp_path / "b").mkdir()
    losses_off, params_off, rec_off = _train(mixed, state_dict, dev, tmp_path / "a", False, capsys)
    losses_on, params_on, rec_on = _train(mixed, state_dict, dev, tmp_path / "b", True, capsys)
    print("losses without prefetch", losses_off.tolist(), "with", losses_on.tolist())
    assert losses_off.shape == (3,) and torch.equal(losses_on, losses_off) and bool(torch.isfinite(losses_off).all())
    assert torch.equal(rec_on, rec_off)                                         # the draws came in batch order
    for k, v in params_off.items():
        assert torch.equal(params_on[k], v), k
    fresh = dict(_model(state_dict, dev).named_parameters())
    assert not torch.equal(params_off["net_vlad.centroids"], fresh["net_vlad.centroids"].detach())     # it trained


@pytest.mark.parametrize("prefetch", [False, True])
def test_a_damaged_file_of_the_second_batch_is_named_behind_its_loss(mixed, state_dict, dev, tmp_path, capsys, prefetch):
    from ibl.trainers import Trainer
    B, N, iters = 2, 4, 3
    records = _write(mixed, tmp_path, B * N * iters)
    base = mixed["s_120x160_420"]
    assert records[11][4] in TRAIN_FILES
    (tmp_path / "f11.jpg").write_bytes(base[:jpeg.parse(base).scan_begin + 3000].tobytes())    # the second batch
    model = _model(state_dict, dev)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    jitter = ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8", generator=torch.Generator().manual_seed(41))
    trainer = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index, prefetch=prefetch,
                      augment=Compose(DecodeJpeg(), jitter, Resize(32, 48)))
    seen = []
    real = trainer._forward
    trainer._forward = lambda *a, **k: seen.append(1) or real(*a, **k)
    capsys.readouterr()
    with pytest.raises(RuntimeError, match=r"1 damaged JPEG file\(s\): f11.jpg \(ran out of bytes\)"):
        trainer.train(5, 1, _loader(records, tmp_path, B, N, iters, (32, 48)), opt, iters, print_freq=1)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch: [5-1]")]
    # the first iteration completed; the second one's forward ran (its loss was read), its step did not
    assert len(lines) == 1 and lines[0].startswith("Epoch: [5-1][1/3]") and len(seen) == 2
