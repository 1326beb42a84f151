"""The chunked route of the device JPEG decoder (csrc/jpeg.hip, `ops.decode_jpeg(scan="chunked")`, the route
names of `input_decode`) against Pillow's own outputs in tests/golden/jpeg_decode.npz and tests/golden/jpeg_chunked.npz
and against the serial route.  Every comparison is exact: the decoder is integer arithmetic."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from openibl_amd import jpeg, ops

pytestmark = pytest.mark.gpu

FREE = ("8x8_444", "16x16_420", "9x17_422", "17x31_420", "37x53_444", "37x53_422", "37x53_420", "48x64_420_q30",
        "48x64_420_q75", "48x64_420_q95", "48x64_422_opt", "37x53_grey", "48x64_444_flat", "48x64_444_noise")
RESTARTS = ("48x64_420_rst1", "48x64_420_rst3", "48x64_420_rstrow", "40x104_444_rst65")
LONG = ("420_q75_smooth", "444_q95_noise", "422_opt", "grey", "420_rst2rows")


@pytest.fixture(scope="module")
def golden():
    both = load_golden("jpeg_decode")
    long_files = load_golden("jpeg_chunked")
    assert tuple(long_files["names"]) == LONG
    for n in LONG:
        both["s_" + n], both["y_" + n] = long_files["s_" + n], long_files["y_" + n]
    return both


def _decode(files, dev, **kw):
    return ops.decode_jpeg(jpeg.JpegBatch.from_files(files).to(dev), **kw)


def _same(got, want):
    want = torch.as_tensor(np.asarray(want))
    got = got.cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}")


def _many(golden):
    o = golden["many_offsets"]
    return [golden["many_bytes"][o[i]:o[i + 1]] for i in range(len(o) - 1)]


@pytest.fixture(scope="module")
def serial(golden, dev):
    """The serial route's pixels and status of every single file, computed once."""
    out = {}
    for n in FREE + RESTARTS + LONG:
        px, st = _decode([golden["s_" + n]], dev, check=False, scan="serial")
        out[n] = (px.cpu(), st.cpu())
    return out


# ---- 1. restart-free files: one segment of many lanes ---------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [4, 16, 64, 128])
def test_chunked_output_is_pils_and_the_serial_routes(golden, dev, serial, chunk_bytes):
    for n in FREE + LONG[:4]:
        got, status = _decode([golden["s_" + n]], dev, check=False, scan="chunked", chunk_bytes=chunk_bytes)
        assert ops.last_jpeg_route == "chunked"
        assert status.tolist() == [0] and torch.equal(status.cpu(), serial[n][1]), n
        _same(got[0], golden["y_" + n])
        assert torch.equal(got.cpu(), serial[n][0]), n
    if chunk_bytes == 4:          # more chunks than lanes: the last lane took the remainder
        assert jpeg.JpegBatch.from_files([golden["s_48x64_444_noise"]]).max_segment_bytes > 4 * 1024


def test_the_settle_loop_iterates_on_the_device(golden, dev):
    _decode([golden["s_48x64_444_noise"]], dev, scan="chunked", chunk_bytes=16)
    rounds = ops.last_jpeg_rounds.cpu().tolist()
    assert len(rounds) == 1 and 20 <= rounds[0] <= 1024, rounds


# ---- 2. restart files: segments of one lane beside segments of many -------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [16, 64])
def test_restart_files(golden, dev, serial, chunk_bytes):
    for n in RESTARTS + LONG[4:]:
        got, status = _decode([golden["s_" + n]], dev, check=False, scan="chunked", chunk_bytes=chunk_bytes)
        assert status.tolist() == [0], n
        _same(got[0], golden["y_" + n])
        assert torch.equal(got.cpu(), serial[n][0]), n
    batch = jpeg.JpegBatch.from_files([golden["s_40x104_444_rst65"]] * 2)
    assert batch.max_segments == 65 and batch.segments.shape[0] == 130
    got = ops.decode_jpeg(batch.to(dev), scan="chunked", chunk_bytes=chunk_bytes)
    _same(got[0], golden["y_40x104_444_rst65"])
    _same(got[1], golden["y_40x104_444_rst65"])


# ---- 3. batches -----------------------------------------------------------------------------------------------------
def test_the_mixed_batch_and_the_seventy(golden, dev):
    names = list(golden["mixed4"])
    for cb in (16, 128):
        got = _decode([golden["s_" + n] for n in names], dev, scan="chunked", chunk_bytes=cb)
        assert got.shape == (4, 48, 64, 3)
        for i, n in enumerate(names):
            _same(got[i], golden["y_" + n])
    _same(_decode(_many(golden), dev, scan="chunked", chunk_bytes=16), golden["many_y"])
    _same(_decode(_many(golden), dev, scan="chunked"), golden["many_y"])
    _same(_decode([golden["s_" + n] for n in LONG], dev, scan="chunked"), np.stack([golden["y_" + n] for n in LONG]))


def test_two_runs_give_identical_bits(golden, dev):
    files = _many(golden)
    a, sa = _decode(files, dev, check=False, scan="chunked", chunk_bytes=16)
    b, sb = _decode(files, dev, check=False, scan="chunked", chunk_bytes=16)
    assert torch.equal(a, b) and torch.equal(sa, sb) and int(sa.abs().sum()) == 0 and sa.dtype == torch.int32
    files = [golden["s_" + n] for n in LONG]
    a, sa = _decode(files, dev, check=False, scan="chunked", chunk_bytes=64)
    b, sb = _decode(files, dev, check=False, scan="chunked", chunk_bytes=64)
    assert torch.equal(a, b) and torch.equal(sa, sb) and int(sa.abs().sum()) == 0


def test_an_image_does_not_depend_on_its_batch_mates(golden, dev):
    names = list(golden["mixed4"])
    batch = _decode([golden["s_" + n] for n in names], dev, scan="chunked", chunk_bytes=16)
    for i, n in enumerate(names):
        assert torch.equal(_decode([golden["s_" + n]], dev, scan="chunked", chunk_bytes=16)[0], batch[i]), n
    back = _decode([golden["s_" + n] for n in names[::-1]], dev, scan="chunked", chunk_bytes=16)
    assert torch.equal(back.flip(0), batch)


# ---- 4. the route "auto" takes ----------------------------------------------------------------------------------------
def test_auto_takes_the_chunked_route_for_long_segments_only(golden, dev, serial):
    long_file, short_file = golden["s_444_q95_noise"], golden["s_8x8_444"]
    assert jpeg.JpegBatch.from_files([long_file]).max_segment_bytes >= jpeg.CHUNKED_MIN_BYTES
    assert jpeg.JpegBatch.from_files([short_file]).max_segment_bytes < jpeg.CHUNKED_MIN_BYTES
    got = _decode([long_file], dev, scan="auto")
    assert ops.last_jpeg_route == "chunked"
    also = _decode([long_file], dev)                       # the default is "auto"
    assert ops.last_jpeg_route == "chunked" and torch.equal(got, also)
    assert torch.equal(got.cpu(), serial["444_q95_noise"][0])
    _same(got[0], golden["y_444_q95_noise"])
    got = _decode([short_file], dev, scan="auto")
    assert ops.last_jpeg_route == "serial" and ops.last_jpeg_rounds is None
    assert torch.equal(got.cpu(), serial["8x8_444"][0])
    assert torch.equal(_decode([short_file], dev, scan="chunked").cpu(), serial["8x8_444"][0])
    assert ops.last_jpeg_route == "chunked"


# ---- 5. damaged streams -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [16, 64])
def test_damaged_streams_are_reported_as_the_serial_route_reports_them(golden, dev, chunk_bytes):
    mates = ("48x64_420_q30", "48x64_420_rst3")
    files = [golden["s_" + mates[0]], golden["s_truncated"], golden["s_" + mates[1]], golden["s_xor"]]
    want, want_status = _decode(files, dev, check=False, scan="serial")
    got, status = _decode(files, dev, check=False, scan="chunked", chunk_bytes=chunk_bytes)
    assert status.tolist() == want_status.tolist()
    assert status[0] == 0 and status[2] == 0 and status[1] == jpeg.ST_OUT_OF_BYTES and status[3] != 0
    _same(got[0], golden["y_" + mates[0]])
    _same(got[2], golden["y_" + mates[1]])
    assert torch.equal(got[1, :15], want[1, :15])
    _same(got[1, :15], golden["y_48x64_420_q75"][:15])
    with pytest.raises(ValueError, match=r"image 1 \(ran out of bytes\).*image 3") as chunked:
        _decode(files, dev, scan="chunked", chunk_bytes=chunk_bytes)
    with pytest.raises(ValueError) as plain:
        _decode(files, dev, scan="serial")
    assert str(chunked.value) == str(plain.value)


# ---- 6. the extraction loop -------------------------------------------------------------------------------------------
def _write_files(golden, tmp_path):
    """The six files of 48 x 64 of the loader test of tests/test_gpu_jpeg_decode.py — one of them progressive, which
    the loader's worker decodes — and their records."""
    from PIL import Image          # the comparison loader decodes with Pillow
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


def test_extract_features_with_the_route_named(golden, dev, state_dict, tmp_path):
    import hubconf
    from ibl.evaluators import extract_features
    records = _write_files(golden, tmp_path)
    files, pixels = _loaders(records, tmp_path)
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    model = model.to(dev).eval()
    want = extract_features(model, pixels, records, gpu=dev.index, input_resize=(32, 48))
    plain = extract_features(model, files, records, gpu=dev.index, input_decode="serial", input_resize=(32, 48))
    assert ops.last_jpeg_route == "serial"
    got = extract_features(model, files, records, gpu=dev.index, input_decode="chunked", input_resize=(32, 48))
    assert ops.last_jpeg_route == "chunked"
    assert list(got) == list(want) == [r[0] for r in records]
    for f in want:
        assert torch.equal(got[f], want[f]) and torch.equal(plain[f], want[f]), f
    assert len({tuple(v.tolist()) for v in want.values()}) == 6
    with pytest.raises(ValueError, match="JpegBatch"):
        extract_features(model, pixels, records, gpu=dev.index, input_decode="chunked", input_resize=(32, 48))
    with pytest.raises(ValueError, match="input_decode"):
        extract_features(model, files, records, gpu=dev.index, input_decode="nope", input_resize=(32, 48))
