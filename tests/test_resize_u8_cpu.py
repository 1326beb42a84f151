"""The specification of the device resize, without a GPU: the numpy model of PIL's 8-bit bilinear resampling
(tests/helpers/resize_u8_ref.py — the arithmetic csrc/resize_tables.h and csrc/resize.hip repeat) against the fixture
tests/golden/resize_u8.npz, which holds PIL's own outputs, and against the installed PIL; the `resize=False` switch of
the host transforms; the sizes of `augment.Resize(keep_aspect=True)`; the argument checks of Resize and Compose."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import resize_u8_ref as ref

CASES = ("down", "far", "from_one", "half", "one_axis", "same", "to_one", "up")
JITTERED = ("odd37x53", "parts96x128", "perm24")


@pytest.fixture(scope="module")
def golden():
    return load_golden("resize_u8")


def test_fixture_holds_the_cases(golden):
    assert tuple(golden["names"]) == CASES and str(golden["pil_version"])
    for name in CASES:
        assert golden["x_" + name].dtype == np.uint8 and golden["y_" + name].dtype == np.uint8
        assert golden["x_" + name].shape[0] == golden["y_" + name].shape[0]
    # the clip is reached: saturated areas are part of the inputs
    assert (golden["x_half"] == 255).all(-1).any() and (golden["x_half"] == 0).all(-1).any()
    assert np.array_equal(golden["y_same"], golden["x_same"])


@pytest.mark.parametrize("name", CASES)
def test_model_equals_the_fixture(golden, name):
    x, want = golden["x_" + name], golden["y_" + name]
    for i in range(x.shape[0]):
        assert np.array_equal(ref.resize(x[i], want.shape[1], want.shape[2]), want[i]), i
    # a batch goes through the model as its images do
    assert np.array_equal(ref.resize(x, want.shape[1], want.shape[2]), want)


@pytest.mark.parametrize("name", JITTERED)
def test_model_equals_the_fixture_behind_the_jitter(golden, name):
    y = load_golden("color_jitter")["y_" + name]
    want = golden["jr_" + name]
    assert want.shape[0] == y.shape[0]
    assert np.array_equal(ref.resize(y, want.shape[1], want.shape[2]), want)


@pytest.mark.parametrize("src,dst", [((96, 128), (48, 64)), ((61, 83), (48, 64)), ((30, 40), (48, 64)),
                                     ((48, 83), (48, 64)), ((48, 64), (48, 64)), ((97, 131), (16, 16)),
                                     ((7, 5), (1, 1)), ((1, 1), (5, 7)), ((960, 1280), (480, 640)),
                                     ((33, 640), (480, 33))])
def test_model_equals_the_installed_pil(src, dst):
    pytest.importorskip("PIL")
    img = ref.make_image(src[0] + dst[1], *src)
    assert np.array_equal(ref.resize(img, *dst), ref.pil_resize(img, *dst))


def test_identity_tables_are_exact():
    bounds, coeff = ref.tables(640, 640)
    assert coeff.shape == (640, 3) and (coeff[:, 0] == 1 << 22).all() and (coeff[:, 1:] == 0).all()
    assert (bounds[:, 0] == np.arange(640)).all()


def test_rounded_coefficients_can_sum_above_one():
    """Why the clip is needed: somewhere the 22-bit weights of a window add up to more than 2^22."""
    assert max(int(ref.tables(i, o)[1].sum(1).max()) for i, o in ((817, 640), (131, 16), (64, 53))) > 1 << 22


# ---- the host transforms --------------------------------------------------------------------------------------------
def _pil_image(h, w, seed=0):
    Image = pytest.importorskip("PIL.Image")
    return Image.fromarray(ref.make_image(seed, h, w), "RGB")


def test_resize_false_hands_over_the_stored_bytes():
    from ibl.utils.data import get_transformer_test, get_transformer_train
    img = _pil_image(61, 83)
    for make in (get_transformer_train, get_transformer_test):
        raw = make(48, 64, as_uint8=True, resize=False)(img)
        assert raw.dtype == torch.uint8 and tuple(raw.shape) == (61, 83, 3)
        assert np.array_equal(raw.numpy(), np.asarray(img))
        # the default is what it was: the host resizes
        assert tuple(make(48, 64, as_uint8=True)(img).shape) == (48, 64, 3)
        assert tuple(make(48, 64)(img).shape) == (3, 48, 64)
    # and the host's resize of those bytes is the model's
    assert np.array_equal(get_transformer_train(48, 64, as_uint8=True)(img).numpy(), ref.resize(np.asarray(img), 48, 64))


def test_resize_false_needs_as_uint8():
    from ibl.utils.data import get_transformer_test, get_transformer_train
    for make in (get_transformer_train, get_transformer_test):
        with pytest.raises(ValueError, match="as_uint8"):
            make(48, 64, resize=False)
    with pytest.raises(ValueError, match="as_uint8"):
        get_transformer_test(48, 64, tokyo=True, as_uint8=False, resize=False)


@pytest.mark.parametrize("w,h", [(853, 640), (640, 853), (3264, 2448), (500, 500)])
def test_keep_aspect_sizes_are_the_test_transforms(w, h):
    from ibl.utils.data import get_transformer_test
    from openibl_amd.augment import Resize
    Image = pytest.importorskip("PIL.Image")
    got = get_transformer_test(480, 640, tokyo=True, as_uint8=True)(Image.new("RGB", (w, h)))
    assert Resize(480, 640, keep_aspect=True).target(h, w) == (got.shape[0], got.shape[1])
    assert Resize(480, 640).target(h, w) == (480, 640)


def test_resize_argument_errors():
    from openibl_amd.augment import Resize
    for bad in ((0, 64), (48, 0), (-1, 64)):
        with pytest.raises(ValueError, match="positive"):
            Resize(*bad)
    with pytest.raises(TypeError):
        Resize(48.0, 64)
    with pytest.raises(ValueError, match="out"):
        Resize(48, 64, out="half")
    assert Resize(48, 64).out == "float" and Resize(48, 64, out="uint8").out == "uint8"


def test_compose_argument_errors_and_order():
    from openibl_amd.augment import ColorJitter, Compose, Resize
    with pytest.raises(ValueError, match="at least one"):
        Compose()
    with pytest.raises(TypeError):
        Compose(Resize(4, 4, out="uint8"), 5)
    with pytest.raises(ValueError, match="uint8"):
        Compose(ColorJitter(0.7, 0.7, 0.7, 0.5), Resize(48, 64))          # the jitter would hand float on
    Compose(ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8"), Resize(48, 64))
    seen = []
    chain = Compose(lambda x, records=None: seen.append(("a", records)) or x + 1, lambda x: seen.append("b") or x * 2)
    assert chain(1, records="r") == 4 and seen == [("a", "r"), "b"]


def test_input_resize_argument():
    from openibl_amd.augment import Resize
    from openibl_amd.extract import input_resizer
    assert input_resizer(None) is None
    r = input_resizer((64, 96))
    assert isinstance(r, Resize) and r.target(96, 128) == (64, 96) and r.out == "uint8"
    keep = Resize(480, 640, keep_aspect=True, out="uint8")
    assert input_resizer(keep) is keep
    with pytest.raises(ValueError, match="uint8"):
        input_resizer(Resize(64, 96))
    with pytest.raises(TypeError):
        input_resizer(64)
