"""The device JPEG decoder (csrc/jpeg.hip, ops.decode_jpeg, openibl_amd.jpeg, the `input_decode` of extract_features
and TrunkCache.fill) against the fixture tests/golden/jpeg_decode.npz — Pillow's own outputs
(tests/helpers/make_jpeg_golden.py).  Every comparison is exact: the decoder is integer arithmetic."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from openibl_amd import jpeg, ops

pytestmark = pytest.mark.gpu

CASES = ("8x8_444", "16x16_420", "9x17_422", "17x31_420", "37x53_444", "37x53_422", "37x53_420", "48x64_420_q30",
         "48x64_420_q75", "48x64_420_q95", "48x64_420_rst1", "48x64_420_rst3", "48x64_420_rstrow", "48x64_422_opt",
         "37x53_grey", "48x64_444_flat", "48x64_444_noise", "40x104_444_rst65")


@pytest.fixture(scope="module")
def golden():
    return load_golden("jpeg_decode")


def _decode(files, dev, **kw):
    return ops.decode_jpeg(jpeg.JpegBatch.from_files(files).to(dev), **kw)


def _mismatch(got, want):
    bad = (got != want).nonzero()
    return f"{len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _same(got, want):
    want = torch.as_tensor(np.asarray(want))
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want), _mismatch(got, want)


@pytest.mark.parametrize("name", CASES)
def test_output_is_pils(golden, dev, name):
    _same(_decode([golden["s_" + name]], dev)[0], golden["y_" + name])


def test_the_mixed_batch(golden, dev):
    names = list(golden["mixed4"])
    got = _decode([golden["s_" + n] for n in names], dev)
    assert got.shape == (4, 48, 64, 3)
    for i, n in enumerate(names):
        _same(got[i], golden["y_" + n])


def _many(golden):
    o = golden["many_offsets"]
    return [golden["many_bytes"][o[i]:o[i + 1]] for i in range(len(o) - 1)]


def test_seventy_images_in_one_call(golden, dev):
    _same(_decode(_many(golden), dev), golden["many_y"])


def test_sixty_five_segments_of_one_image(golden, dev):
    batch = jpeg.JpegBatch.from_files([golden["s_40x104_444_rst65"]] * 2)
    assert batch.max_segments == 65 and batch.segments.shape[0] == 130
    got = ops.decode_jpeg(batch.to(dev))
    _same(got[0], golden["y_40x104_444_rst65"])
    _same(got[1], golden["y_40x104_444_rst65"])


def test_two_runs_give_identical_bits(golden, dev):
    files = _many(golden)
    a, sa = _decode(files, dev, check=False)
    b, sb = _decode(files, dev, check=False)
    assert torch.equal(a, b) and torch.equal(sa, sb) and int(sa.abs().sum()) == 0 and sa.dtype == torch.int32


def test_an_image_does_not_depend_on_its_batch_mates(golden, dev):
    names = list(golden["mixed4"])
    batch = _decode([golden["s_" + n] for n in names], dev)
    for i, n in enumerate(names):
        assert torch.equal(_decode([golden["s_" + n]], dev)[0], batch[i]), n
    back = _decode([golden["s_" + n] for n in names[::-1]], dev)
    assert torch.equal(back.flip(0), batch)


def test_a_batch_with_host_decoded_files(golden, dev):
    pytest.importorskip("PIL")
    files = [golden["s_37x53_420"], golden["f_progressive"], golden["s_37x53_grey"], golden["f_png"],
             golden["f_cmyk"]]
    batch = jpeg.JpegBatch.from_files(files)
    assert batch.host_index.tolist() == [1, 3, 4] and batch.reasons[1] == "progressive"
    got, status = ops.decode_jpeg(batch.to(dev), check=False)
    assert status.tolist() == [0] * 5
    for i, key in enumerate(("y_37x53_420", "fy_progressive", "y_37x53_grey", "fy_png", "fy_cmyk")):
        _same(got[i], golden[key])
    # only host-decoded files: nothing is launched, the pixels arrive
    _same(_decode([golden["f_9x4_420"]], dev)[0], golden["fy_9x4_420"])


def test_damaged_streams_are_reported_and_leave_their_batch_mates_alone(golden, dev):
    mates = ("48x64_420_q30", "48x64_420_rst3")
    files = [golden["s_" + mates[0]], golden["s_truncated"], golden["s_" + mates[1]], golden["s_xor"]]
    got, status = _decode(files, dev, check=False)
    status = status.tolist()
    assert status[0] == 0 and status[2] == 0 and status[1] == jpeg.ST_OUT_OF_BYTES and status[3] != 0
    _same(got[0], golden["y_" + mates[0]])
    _same(got[2], golden["y_" + mates[1]])
    # what was decoded in front of the cut is still there: the first MCU row of the truncated file (its last pixel
    # row blends in the chroma row below, which the cut took)
    _same(got[1, :15], golden["y_48x64_420_q75"][:15])
    with pytest.raises(ValueError, match=r"image 1 \(ran out of bytes\).*image 3"):
        _decode(files, dev)
    # a restart stream that ends in front of one of its markers: the parser's finding is the status
    data = golden["s_48x64_420_rst1"]
    p = jpeg.parse(data)
    cut = data[:p.scan_begin + int(p.segments[5, 1])]
    got, status = _decode([cut, data], dev, check=False)
    assert status.tolist() == [jpeg.ST_BAD_RESTART, 0]
    _same(got[1], golden["y_48x64_420_rst1"])


# ---- the loader and the extraction loops ---------------------------------------------------------------------------
def _write_files(golden, tmp_path):
    """Six files of 48 x 64 in tmp_path — one of them progressive, which the loader's worker decodes — and their
    records."""
    from PIL import Image          # the comparison loader decodes with Pillow: these tests need it
    from helpers import jpeg_ref as ref
    names = ["48x64_420_q30", "48x64_420_q75", "48x64_422_opt", "48x64_420_rst3", "48x64_444_noise"]
    records = []
    for j, n in enumerate(names):
        (tmp_path / f"g{j}.jpg").write_bytes(golden["s_" + n].tobytes())
        records.append((f"g{j}.jpg", j, 0.0, 0.0))
    Image.fromarray(ref.make_image(3, 48, 64)).save(tmp_path / "g5.jpg", "JPEG", progressive=True)
    records.append(("g5.jpg", 5, 0.0, 0.0))
    return records


def _loaders(records, root):
    from ibl.utils.data import get_transformer_test
    from ibl.utils.data.preprocessor import Preprocessor
    files = torch.utils.data.DataLoader(Preprocessor(records, root=str(root), raw=True), batch_size=2, num_workers=0,
                                        shuffle=False, collate_fn=jpeg.collate)
    pixels = torch.utils.data.DataLoader(
        Preprocessor(records, root=str(root), transform=get_transformer_test(32, 48, as_uint8=True, resize=False)),
        batch_size=2, num_workers=0, shuffle=False)
    return files, pixels


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_extract_features_with_input_decode(golden, dev, state_dict, tmp_path, precision):
    import hubconf
    from ibl.evaluators import extract_features
    records = _write_files(golden, tmp_path)
    files, pixels = _loaders(records, tmp_path)
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    model = model.to(dev).eval().set_precision(precision)
    want = extract_features(model, pixels, records, gpu=dev.index, input_resize=(32, 48))
    got = extract_features(model, files, records, gpu=dev.index, input_decode=True, input_resize=(32, 48))
    also = extract_features(model, files, records, gpu=dev.index, input_decode=True, input_resize=(32, 48),
                            use_graphs=False)
    assert list(got) == list(want) == [r[0] for r in records]
    for f in want:
        assert torch.equal(got[f], want[f]) and torch.equal(also[f], want[f]), f
    assert len({tuple(v.tolist()) for v in want.values()}) == 6
    with pytest.raises(ValueError, match="JpegBatch"):
        extract_features(model, pixels, records, gpu=dev.index, input_decode=True, input_resize=(32, 48))


def test_extract_features_lists_the_damaged_files(golden, dev, state_dict, tmp_path):
    import hubconf
    from ibl.evaluators import extract_features
    records = _write_files(golden, tmp_path)[:4]
    (tmp_path / "g2.jpg").write_bytes(golden["s_truncated"].tobytes())
    files, _ = _loaders(records, tmp_path)
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    model = model.to(dev).eval()
    with pytest.raises(RuntimeError, match=r"1 damaged JPEG file\(s\): g2.jpg \(ran out of bytes\)"):
        extract_features(model, files, records, gpu=dev.index, input_decode=True, input_resize=(32, 48))


def test_trunk_cache_fill_with_input_decode(golden, dev, state_dict, tmp_path):
    import hubconf
    from openibl_amd.trunk_cache import TrunkCache
    records = _write_files(golden, tmp_path)
    files, pixels = _loaders(records, tmp_path)
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    for layer in list(model.base_model.base.children())[:24]:
        for p in layer.parameters():
            p.requires_grad_(False)
    model = model.to(dev).eval()
    want = TrunkCache.fill(model, pixels, records, gpu=dev.index, input_resize=(32, 48))
    got = TrunkCache.fill(model, files, records, gpu=dev.index, input_decode=True, input_resize=(32, 48))
    assert got.n_items == want.n_items == 6 and torch.equal(got.lines, want.lines)
    assert torch.equal(got.descriptors(model), want.descriptors(model))
