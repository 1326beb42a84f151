"""The colour jitter without a GPU: the numpy model of the kernel's arithmetic (tests/helpers/color_jitter_ref.py)
against PIL — all 2^24 colours through both HSV directions, random images through every blend — and against the
fixture (PIL's outputs); openibl_amd.augment.ColorJitter's argument checks and draws; the loader's uint8 training
transform; the trainers' `augment` hand-over; the argument checks of ops.color_jitter."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import color_jitter_ref as ref


@pytest.fixture(scope="module")
def all_colours():
    g = np.arange(256, dtype=np.uint8)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(4096, 4096, 3)


def test_model_rgb_to_hsv_is_pils_on_every_colour(all_colours):
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.fromarray(all_colours, mode="RGB").convert("HSV"))
    assert np.array_equal(ref.rgb_to_hsv(all_colours), want)


def test_model_hsv_to_rgb_is_pils_on_every_colour(all_colours):
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.fromarray(all_colours, mode="HSV").convert("RGB"))
    assert np.array_equal(ref.hsv_to_rgb(all_colours), want)


def test_model_blends_are_pils_on_random_images():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(5)
    for h, w in ((31, 45), (64, 64)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[: h // 4] //= 8         # dark rows: products near zero
        img[-h // 4:] |= 0xE0       # bright rows: the upper clip
        for factor in (0.0, 0.3, 0.999, 1.0, 1.0000001, 1.7, 2.5):
            for op in (ref.BRIGHTNESS, ref.CONTRAST, ref.SATURATION):
                factors = [1.0, 1.0, 1.0]
                factors[op] = factor
                got = ref.model_jitter(img, [op, -1, -1, -1], factors, 0)
                want = ref.pil_jitter(img, [op, -1, -1, -1], factors, 0)
                assert np.array_equal(got, want), (h, w, factor, op)
        # contrast behind other ops: the mean is the mean of the image as it stands
        for order in ([ref.BRIGHTNESS, ref.CONTRAST, -1, -1], [ref.HUE, ref.SATURATION, ref.CONTRAST, ref.BRIGHTNESS]):
            got = ref.model_jitter(img, order, [1.4, 0.6, 1.6], 200)
            assert np.array_equal(got, ref.pil_jitter(img, order, [1.4, 0.6, 1.6], 200)), order
    assert ref.hue_byte(-0.5) == 129 and ref.hue_byte(0.5) == 127 and ref.hue_byte(0.0) == 0
    assert np.array_equal(ref.luma(np.uint8([[[255, 255, 255], [0, 0, 0], [7, 7, 7]]])), [[255, 0, 7]])


def test_model_reproduces_the_fixture_and_the_fixture_has_the_cases():
    g = load_golden("color_jitter")
    names = [str(n) for n in g["names"]]
    assert sorted(names) == ["exact", "flat", "mean_half", "odd37x53", "odd5x7", "parts96x128", "perm24", "sweep64"]
    for n in names:
        x, rec, y = g["x_" + n], g["rec_" + n], g["y_" + n]
        assert x.dtype == np.uint8 and y.shape == x.shape and rec.shape == (x.shape[0], 8) and rec.dtype == np.int32
        assert np.array_equal(ref.model_jitter_records(x, rec), y), n
    # what the cases are there for
    assert sorted(map(tuple, g["rec_perm24"][:, :4].tolist())) == sorted(
        __import__("itertools").permutations(range(4)))
    assert g["x_odd5x7"][0].size % 4 == 1                                     # the second image starts misaligned
    assert (g["rec_odd5x7"][2, :4] == -1).all() and np.array_equal(g["y_odd5x7"][2], g["x_odd5x7"][2])
    assert g["x_parts96x128"].shape[1] * g["x_parts96x128"].shape[2] > 2 * 4096   # several workgroups per image
    f = g["rec_exact"][:, 4:7].view(np.float32)
    assert np.array_equal(f, np.float32([[0.3] * 3, [1.0] * 3, [1.7] * 3])) and g["rec_exact"][:, 7].tolist() == [129, 0, 127]
    means = [ref.contrast_mean(im) for im in g["x_mean_half"]]
    sums = [int(ref.luma(im).sum()) for im in g["x_mean_half"]]
    assert means == [101, 100, 101, 100] and sums[0] * 2 == 201 * 256 and sums[1] == sums[0] - 1
    hsv = ref.rgb_to_hsv(g["x_sweep64"][0])
    assert set(np.floor(hsv[..., 0].astype(np.float64) * 6 / 255).astype(int).ravel() % 6) == set(range(6))
    flat = g["x_flat"]
    assert (flat[0] == 77).all() and (flat[1] == 0).all() and (flat[2] == 255).all()


def test_color_jitter_argument_checks():
    from openibl_amd.augment import ColorJitter
    j = ColorJitter(0.7, 0.7, 0.7, 0.5)
    for got, want in ((j.brightness, (0.3, 1.7)), (j.contrast, (0.3, 1.7)), (j.saturation, (0.3, 1.7))):
        assert got == pytest.approx(want)
    assert j.hue == (-0.5, 0.5) and j.enabled
    assert ColorJitter(brightness=2.0).brightness == (0.0, 3.0)              # the lower end is clipped at 0
    assert ColorJitter(contrast=(0.5, 0.9)).contrast == (0.5, 0.9)
    assert ColorJitter(hue=(-0.1, 0.3)).hue == (-0.1, 0.3)
    off = ColorJitter()
    assert (off.brightness, off.contrast, off.saturation, off.hue) == (None,) * 4 and not off.enabled
    assert ColorJitter(brightness=(1, 1), hue=(0, 0)).enabled is False       # a degenerate range disables the op
    for kw in ({"brightness": -0.1}, {"contrast": (1.5, 0.5)}, {"saturation": (-0.2, 1.0)}, {"hue": 0.6},
               {"hue": (-0.6, 0.1)}, {"hue": -0.1}):
        with pytest.raises(ValueError):
            ColorJitter(**kw)
    for kw in ({"brightness": "big"}, {"hue": (0.1, 0.2, 0.3)}):
        with pytest.raises(TypeError):
            ColorJitter(**kw)
    with pytest.raises(ValueError, match="out"):
        ColorJitter(out="half")


def test_draws_are_deterministic_in_range_and_leave_disabled_ops_out():
    from openibl_amd.augment import ColorJitter, hue_byte
    a = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(11)).draw(64)
    b = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(11)).draw(64)
    c = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(12)).draw(64)
    assert a.dtype == torch.int32 and a.shape == (64, 8) and a.is_contiguous() and not a.is_cuda
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert (a[:, :4].sort(dim=1).values == torch.arange(4, dtype=torch.int32)).all()   # a permutation per image
    assert len({tuple(r) for r in a[:, :4].tolist()}) > 8                      # and not the same one
    f = a[:, 4:7].contiguous().view(torch.float32)
    assert (f >= 0.3 - 1e-6).all() and (f <= 1.7 + 1e-6).all() and f.std() > 0.2
    assert ((a[:, 7] >= 0) & (a[:, 7] <= 255)).all()
    assert ((a[:, 7] <= 127) | (a[:, 7] >= 129)).all() and (a[:, 7] <= 127).any() and (a[:, 7] >= 129).any()
    assert [hue_byte(h) for h in (-0.5, -0.004, 0.0, 0.004, 0.5)] == [129, 255, 0, 1, 127]
    # the order of the draws: randperm(4), then brightness, contrast, saturation, hue
    g = torch.Generator().manual_seed(3)
    one = ColorJitter(0.4, 0, (0.5, 1.5), 0.1, generator=g).draw(1)[0]
    g = torch.Generator().manual_seed(3)
    order = torch.randperm(4, generator=g).tolist()
    bri = float(torch.empty(1).uniform_(0.6, 1.4, generator=g))
    sat = float(torch.empty(1).uniform_(0.5, 1.5, generator=g))
    hue = float(torch.empty(1).uniform_(-0.1, 0.1, generator=g))
    assert one[:4].tolist() == [-1 if op == 1 else op for op in order]         # contrast is disabled: never there
    assert one[4:7].view(torch.float32).tolist() == [np.float32(bri), 1.0, np.float32(sat)]
    assert int(one[7]) == hue_byte(hue)
    only_hue = ColorJitter(hue=0.5, generator=torch.Generator().manual_seed(1)).draw(32)
    assert set(only_hue[:, :4].flatten().tolist()) == {-1, 3} and (only_hue[:, :4] == 3).sum() == 32
    assert (ColorJitter().draw(4)[:, :4] == -1).all()


def test_train_transform_hands_over_uint8_and_its_default_is_unchanged():
    Image = pytest.importorskip("PIL.Image")
    from ibl.utils.data import get_transformer_test, get_transformer_train
    rng = np.random.default_rng(2)
    img = Image.fromarray(rng.integers(0, 256, (30, 50, 3), dtype=np.uint8), mode="RGB")
    raw = get_transformer_train(24, 40, as_uint8=True)(img)
    assert raw.dtype == torch.uint8 and raw.shape == (24, 40, 3) and raw.is_contiguous()
    assert torch.equal(raw, get_transformer_test(24, 40, as_uint8=True)(img))
    dflt = get_transformer_train(24, 40)(img)
    assert dflt.dtype == torch.float32 and dflt.shape == (3, 24, 40)
    assert torch.equal(dflt, get_transformer_test(24, 40)(img))
    assert torch.equal(dflt, ref.host_normalize(raw[None])[0])                  # the float of those bytes


class _StubAugment:
    """Stands in for ColorJitter: records what the trainer hands it, answers [n][3][H][W] float32."""

    def __init__(self):
        self.seen = []

    def __call__(self, u8):
        self.seen.append(u8)
        return u8.permute(0, 3, 1, 2).float()


def _raw_batch(B, per_tuple, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (B, per_tuple, H, W, 3), dtype=torch.uint8, generator=g)
    return imgs, [(imgs[:, j].contiguous(), ["name"] * B) for j in range(per_tuple)]


def test_trainers_hand_uint8_tuples_to_augment(monkeypatch):
    from ibl.trainers import SFRSTrainer, Trainer
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)    # no device here: the move is the identity
    B, H, W = 2, 6, 10
    imgs, batch = _raw_batch(B, 4, H, W, 0)
    t = Trainer(None, augment=_StubAugment())
    out = t._parse_data(batch)
    assert out.shape == (B, 4, 3, H, W) and out.dtype == torch.float32
    seen, = t.augment.seen
    assert seen.dtype == torch.uint8 and seen.shape == (B * 4, H, W, 3) and seen.is_contiguous()
    assert torch.equal(seen.view(B, 4, H, W, 3), imgs)                        # tuple-major, every image once
    assert torch.equal(out, imgs.permute(0, 1, 4, 2, 3).float())
    neg_num, n_diff = 2, 2
    imgs, batch = _raw_batch(B, 2 + neg_num + n_diff, H, W, 1)
    s = SFRSTrainer(None, None, neg_num=neg_num)
    assert s.augment is None and Trainer(None).augment is None                # opt-in: off by default
    s.augment = _StubAugment()                                                # ... and settable as an attribute
    easy, diff = s._parse_data(batch)
    seen, = s.augment.seen                                                    # ONE call: the anchor is jittered once
    assert seen.shape == (B * 6, H, W, 3) and torch.equal(seen.view(B, 6, H, W, 3), imgs)
    want = imgs.permute(0, 1, 4, 2, 3).float()
    assert torch.equal(easy, want[:, :4]) and torch.equal(diff, torch.cat((want[:, :1], want[:, 4:]), 1))
    # float tuples with augment set are refused, and without augment nothing changed
    fl = [(torch.zeros((B, 3, H, W)), ["name"] * B) for _ in range(4)]
    with pytest.raises(ValueError, match="uint8 tuples"):
        t._parse_data(fl)
    assert Trainer(None)._parse_data(fl).shape == (B, 4, 3, H, W)


def test_ops_color_jitter_refuses_cpu_tensors_and_bad_arguments():
    from openibl_amd import ops
    from openibl_amd.lib import OpenIBLAmdError
    u8 = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    rec = torch.zeros((2, 8), dtype=torch.int32)
    for params in (None, rec):
        for out in ("float", "uint8"):
            with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
                ops.color_jitter(u8, params, out=out)
    from openibl_amd.augment import ColorJitter
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ColorJitter(0.7, 0.7, 0.7, 0.5)(u8)
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ColorJitter()(u8)
    for bad, params, match in ((u8.float(), rec, "uint8"), (u8[0], rec, r"\[N\]\[H\]\[W\]\[3\]"),
                               (torch.zeros((2, 3, 4, 6), dtype=torch.uint8), rec, r"\[N\]\[H\]\[W\]\[3\]"),
                               (torch.zeros((0, 4, 6, 3), dtype=torch.uint8), None, r"\[N\]\[H\]\[W\]\[3\]"),
                               (u8, rec.float(), "int32"), (u8, rec[:1], "params must be"),
                               (u8, torch.zeros((2, 4), dtype=torch.int32), "params must be"),
                               (u8.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), rec, "contiguous"),
                               (u8, torch.zeros((8, 2), dtype=torch.int32).t(), "contiguous")):
        with pytest.raises(ValueError, match=match):
            ops.color_jitter(bad, params)
    with pytest.raises(ValueError, match="out must be"):
        ops.color_jitter(u8, rec, out="bf16")


def test_entry_point_validates_before_any_launch():
    import ctypes
    from openibl_amd import lib
    h = lib.load()
    assert h.oibl_color_jitter_u8_workspace_bytes(12, 480, 640) == 12 * 75 * 8 + (-12 * 75 * 8) % 256
    assert h.oibl_color_jitter_u8_workspace_bytes(1, 5, 7) == 256
    assert h.oibl_color_jitter_u8_workspace_bytes(1, 1 << 14, 1 << 14) == 1024 * 8      # at most 1024 sums per image
    assert h.oibl_color_jitter_u8_workspace_bytes(0, 4, 4) == 0 == h.oibl_color_jitter_u8_workspace_bytes(1, 1 << 15, 1 << 14)
    buf = ctypes.create_string_buffer(512)       # never dereferenced: validation fails first
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    m3 = (ctypes.c_float * 3)(0, 0, 0)
    assert h.oibl_color_jitter_u8(None, 1, 4, 4, p, 0, m3, m3, p, p, 256, None) == -1 and b"null" in h.oibl_last_error()
    assert h.oibl_color_jitter_u8(p, 1, 0, 4, p, 0, m3, m3, p, p, 256, None) == -1 and b"bad shape" in h.oibl_last_error()
    assert h.oibl_color_jitter_u8(p, 1, 4, 4, p, 2, m3, m3, p, p, 256, None) == -1 and b"out_kind" in h.oibl_last_error()
    assert h.oibl_color_jitter_u8(p, 1, 4, 4, p, 1, None, m3, p, p, 256, None) == -1 and b"mean3_host" in h.oibl_last_error()
    assert h.oibl_color_jitter_u8(p, 1, 4, 4, p, 0, m3, m3, p, p + 8, 256, None) == -1 and b"aligned" in h.oibl_last_error()
    assert h.oibl_color_jitter_u8(p, 1, 4, 4, p, 0, m3, m3, p, p, 8, None) != 0 and b"workspace" in h.oibl_last_error()
