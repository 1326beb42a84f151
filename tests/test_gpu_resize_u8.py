"""The device resize (csrc/resize.hip, ops.resize_u8, openibl_amd.augment.Resize / Compose, the `input_resize` of
extract_features) against the fixture tests/golden/resize_u8.npz — PIL's outputs (tests/helpers/make_resize_golden.py)
— and against the numpy model of PIL's arithmetic (tests/helpers/resize_u8_ref.py).  Every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import color_jitter_ref as jitter_ref
from helpers import resize_u8_ref as ref
from openibl_amd import ops
from openibl_amd.augment import ColorJitter, Compose, Resize

pytestmark = pytest.mark.gpu

CASES = ("down", "far", "from_one", "half", "one_axis", "same", "to_one", "up")
JITTERED = ("odd37x53", "parts96x128", "perm24")
TILE_H, TILE_W = 16, 64         # RS_TILE_H, RS_TILE_W of csrc/resize_tables.h


@pytest.fixture(scope="module")
def golden():
    return load_golden("resize_u8")


def _mismatch(got, want):
    bad = (got != want).nonzero()
    return f"{len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


# ---- the tables: the device's fp64 division and truncation ---------------------------------------------------------
@pytest.mark.parametrize("in_size,out_size", [(1280, 640), (640, 640), (53, 64), (64, 53), (131, 16), (817, 640),
                                              (640, 224), (3264, 640), (5, 1), (1, 7)])
def test_tables_are_the_models(dev, in_size, out_size):
    want_bounds, want_coeff = ref.tables(in_size, out_size)
    bounds, coeff = ops.resize_u8_tables(in_size, out_size, device=dev)
    assert coeff.shape == want_coeff.shape == (out_size, ref.ksize_of(in_size, out_size))
    assert np.array_equal(bounds.cpu().numpy(), want_bounds)
    assert np.array_equal(coeff.cpu().numpy(), want_coeff)


# ---- outputs against PIL's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_uint8_output_is_pils(golden, dev, name):
    x, want = torch.from_numpy(golden["x_" + name]).to(dev), torch.from_numpy(golden["y_" + name])
    got = ops.resize_u8(x, want.shape[1:3], out="uint8").cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), _mismatch(got, want)


def test_same_size_returns_the_input(golden, dev):
    x = torch.from_numpy(golden["x_same"]).to(dev)
    assert torch.equal(ops.resize_u8(x, (48, 64)), x)


@pytest.mark.parametrize("nh", [TILE_H - 1, TILE_H, TILE_H + 1])
@pytest.mark.parametrize("nw", [TILE_W - 1, TILE_W, TILE_W + 1])
def test_tile_edges(dev, nh, nw):
    h, w = int(nh * 1.37) + 1, int(nw * 1.37) + 1
    x = np.stack([ref.make_image(7 * nh + nw + i, h, w) for i in range(2)])
    want = torch.from_numpy(ref.resize(x, nh, nw))
    got = ops.resize_u8(torch.from_numpy(x).to(dev), (nh, nw)).cpu()
    assert torch.equal(got, want), _mismatch(got, want)


def test_several_tiles_and_a_deep_window(dev):
    """More than one tile on both axes at a factor past 4: every tile has its own first source row."""
    x = ref.make_image(5, 150, 331)[None]
    want = torch.from_numpy(ref.resize(x, 33, 70))
    got = ops.resize_u8(torch.from_numpy(x).to(dev), (33, 70)).cpu()
    assert torch.equal(got, want), _mismatch(got, want)


# ---- batch and layout ----------------------------------------------------------------------------------------------
def test_an_image_does_not_depend_on_its_batch_mates(golden, dev):
    x = torch.from_numpy(golden["x_down"]).to(dev)
    assert x.shape[0] == 3 and not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2])
    whole8, wholef = ops.resize_u8(x, (48, 64)), ops.resize_u8(x, (48, 64), out="float")
    for n in range(3):
        assert torch.equal(ops.resize_u8(x[n:n + 1], (48, 64)), whole8[n:n + 1]), n
        assert torch.equal(ops.resize_u8(x[n:n + 1], (48, 64), out="float"), wholef[n:n + 1]), n


def test_two_runs_give_identical_bits(golden, dev):
    for name in ("down", "far"):
        x = torch.from_numpy(golden["x_" + name]).to(dev)
        size = golden["y_" + name].shape[1:3]
        for out in ("uint8", "float"):
            assert torch.equal(ops.resize_u8(x, size, out=out), ops.resize_u8(x, size, out=out))


def test_misaligned_slices_of_a_larger_buffer(golden, dev):
    x, want = torch.from_numpy(golden["x_down"]).to(dev), torch.from_numpy(golden["y_down"])
    buf = torch.zeros(x.numel() + 3, dtype=torch.uint8, device=dev)
    for off in (1, 2, 3):
        xs = buf[off:off + x.numel()].view(x.shape)
        xs.copy_(x)
        assert xs.data_ptr() % 4 == off and torch.equal(ops.resize_u8(xs, (48, 64)).cpu(), want)
        assert torch.equal(ops.resize_u8(xs, (48, 64), out="float").cpu(), jitter_ref.host_normalize(want))


@pytest.mark.parametrize("name", ("down", "up", "far", "from_one"))
def test_float_output_is_the_normalisation_of_the_resized_bytes(golden, dev, name):
    x = torch.from_numpy(golden["x_" + name]).to(dev)
    size = golden["y_" + name].shape[1:3]
    got = ops.resize_u8(x, size, out="float")
    assert got.dtype == torch.float32 and tuple(got.shape) == (x.shape[0], 3, *size)
    assert torch.equal(got, ops.color_jitter(ops.resize_u8(x, size, out="uint8"), None, out="float"))
    assert torch.equal(got.cpu(), jitter_ref.host_normalize(torch.from_numpy(golden["y_" + name])))


# ---- argument errors (all decided on the host: nothing is launched) -------------------------------------------------
def test_argument_errors(dev):
    from openibl_amd import lib as _lib
    x = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev)
    limit = ops.RESIZE_MAX_SCALE
    assert limit >= 8
    tall = torch.zeros((1, limit * 2 + 1, 4, 3), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match=f"limit of {limit}"):
        ops.resize_u8(tall, (2, 4))
    ops.resize_u8(tall[:, :limit * 2], (2, 4))            # the limit itself is served
    # the C entry says the same, and its workspace query answers 0
    lib = _lib.load()
    assert lib.oibl_resize_u8_workspace_bytes(1, limit * 2 + 1, 4, 2, 4) == 0
    assert lib.oibl_resize_u8_workspace_bytes(1, limit * 2, 4, 2, 4) > 0
    out = torch.zeros((1, 2, 4, 3), dtype=torch.uint8, device=dev)
    ws = ops.workspace(4096, dev, slot="resize_u8")
    with pytest.raises(_lib.OpenIBLAmdError, match=f"limit of {limit}"):
        _lib.check(lib.oibl_resize_u8(tall.data_ptr(), 1, limit * 2 + 1, 4, 2, 4, 0, None, None, out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "resize_u8")
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_u8(x.float(), (4, 4))
    with pytest.raises(ValueError, match=r"\[N\]\[H\]\[W\]\[3\]"):
        ops.resize_u8(x[0], (4, 4))
    with pytest.raises(ValueError, match=r"\[N\]\[H\]\[W\]\[3\]"):
        ops.resize_u8(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=dev), (4, 4))
    for size in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError, match="positive"):
            ops.resize_u8(x, size)
    with pytest.raises(ValueError, match="size"):
        ops.resize_u8(x, 4)
    with pytest.raises(ValueError, match="out"):
        ops.resize_u8(x, (4, 4), out="half")
    with pytest.raises(ValueError, match="contiguous"):
        ops.resize_u8(torch.zeros((1, 8, 16, 3), dtype=torch.uint8, device=dev)[:, :, ::2], (4, 4))
    with pytest.raises(_lib.OpenIBLAmdError):
        ops.resize_u8(x.cpu(), (4, 4))


# ---- the reference's order: jitter, then resize ---------------------------------------------------------------------
@pytest.mark.parametrize("name", JITTERED)
def test_jitter_then_resize_is_pils(golden, dev, name):
    jg = load_golden("color_jitter")
    want = torch.from_numpy(golden["jr_" + name])
    x, rec = torch.from_numpy(jg["x_" + name]).to(dev), torch.from_numpy(jg["rec_" + name])
    chain = Compose(ColorJitter(out="uint8"), Resize(want.shape[1], want.shape[2], out="uint8"))
    got = chain(x, records=rec).cpu()
    assert torch.equal(got, want), _mismatch(got, want)
    as_float = Compose(ColorJitter(out="uint8"), Resize(want.shape[1], want.shape[2]))(x, records=rec)
    assert torch.equal(as_float.cpu(), jitter_ref.host_normalize(want))


def test_resize_keep_aspect_on_the_device(dev):
    x = ref.make_image(3, 40, 30)[None]
    r = Resize(24, 32, keep_aspect=True, out="uint8")
    assert r.target(40, 30) == (42, 32)
    assert np.array_equal(r(torch.from_numpy(x).to(dev)).cpu().numpy(), ref.resize(x, 42, 32))


# ---- the trainer ----------------------------------------------------------------------------------------------------
def test_trainer_parse_data_with_a_composed_augment(dev):
    from ibl.trainers import Trainer
    imgs = torch.from_numpy(np.stack([ref.make_image(40 + i, 61, 83) for i in range(3)]))[None]     # [1][3][61][83][3]
    batch = [(imgs[:, j].contiguous(), ["name"]) for j in range(3)]
    jit = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(3), out="uint8")
    trainer = Trainer(None, margin=0.1 ** 0.5, gpu=dev.index, augment=Compose(jit, Resize(48, 64)))
    inputs = trainer._parse_data(batch)
    assert tuple(inputs.shape) == (1, 3, 3, 48, 64) and inputs.dtype == torch.float32 and inputs.is_cuda
    rec = jit.last_records
    flat = imgs.view(3, 61, 83, 3).to(dev)
    manual = ops.color_jitter(ops.resize_u8(ops.color_jitter(flat, rec.to(dev), out="uint8"), (48, 64)), None,
                              out="float")
    assert torch.equal(inputs.view(3, 3, 48, 64), manual)
    model = ref.resize(jitter_ref.model_jitter_records(imgs.view(3, 61, 83, 3).numpy(), rec.numpy()), 48, 64)
    assert torch.equal(inputs.view(3, 3, 48, 64).cpu(), jitter_ref.host_normalize(torch.from_numpy(model)))


# ---- extraction -----------------------------------------------------------------------------------------------------
class _Records(torch.utils.data.Dataset):
    def __init__(self, images, records):
        self.images, self.records = images, records

    def __len__(self):
        return len(self.records)

    def __getitem__(self, i):
        f, pid, x, y = self.records[i]
        return self.images[i], f, pid, x, y


@pytest.fixture(scope="module")
def stored():
    """Six stored images of 96 x 128, and the numpy model's resize of them to 64 x 96."""
    raw = np.stack([ref.make_image(80 + i, 96, 128) for i in range(6)])
    return torch.from_numpy(raw), torch.from_numpy(ref.resize(raw, 64, 96))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extract_features_with_input_resize(dev, state_dict, stored, precision):
    import hubconf
    from ibl.evaluators import extract_features
    raw, resized = stored
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    model = model.to(dev).eval().set_precision(precision)
    records = [(f"g{j}.png", j, 0.0, 0.0) for j in range(6)]

    def loader(images):      # three batches of one shape: the second sight of the shape is captured
        return torch.utils.data.DataLoader(_Records(images, records), batch_size=2, num_workers=0, shuffle=False)

    want = extract_features(model, loader(resized), records, gpu=dev.index)
    got = extract_features(model, loader(raw), records, gpu=dev.index, input_resize=(64, 96))
    also = extract_features(model, loader(raw), records, gpu=dev.index, input_resize=Resize(64, 96, out="uint8"),
                            use_graphs=False)
    assert list(got) == list(want) == [r[0] for r in records]
    for f in want:
        assert torch.equal(got[f], want[f]) and torch.equal(also[f], want[f]), f
    assert len({tuple(v.tolist()) for v in want.values()}) == 6           # six images, six descriptors


def test_extract_features_refuses_float_batches_with_input_resize(dev, state_dict):
    import hubconf
    from ibl.evaluators import extract_features
    from openibl_amd import synth
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    model = model.to(dev).eval()
    records = [(f"g{j}.png", j, 0.0, 0.0) for j in range(2)]
    loader = torch.utils.data.DataLoader(_Records(synth.images(2, 64, 96, seed=5), records), batch_size=2)
    with pytest.raises(ValueError, match="uint8"):
        extract_features(model, loader, records, gpu=dev.index, input_resize=(64, 96))
