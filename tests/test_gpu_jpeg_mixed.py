"""JPEG batches of mixed stored sizes on the device (csrc/jpeg.hip, oibl_resize_u8_mixed of csrc/resize.hip,
ops.decode_jpeg_mixed / resize_u8_mixed / decode_resize_jpeg, jpeg.MixedJpegBatch, the `input_decode` of
extract_features) against the fixture tests/golden/jpeg_mixed.npz — Pillow's own outputs
(tests/helpers/make_jpeg_mixed_golden.py) — and against the uniform calls on every file alone.  Every comparison is
exact: the decoder and the resize are integer arithmetic."""
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden
from openibl_amd import jpeg, ops

pytestmark = pytest.mark.gpu

NAMES = ("37x53_420", "48x64_grey", "64x48_422", "9x8_444", "120x160_420", "120x160_420_rstrow", "640x16_420",
         "40x56_progressive", "24x30_png")
DEVICE = NAMES[:7]
TARGETS = ((40, 72), (48, 64), (16, 16))
ROUTES = (("serial", None), ("chunked", 4), ("chunked", 16), ("chunked", 64))
ORDERS = ((8, 7, 6, 5, 4, 3, 2, 1, 0), (4, 0, 8, 6, 2, 7, 5, 1, 3), (3, 6, 1, 8, 0, 5, 7, 2, 4))
MEAN, STD = (0.48501961, 0.45795686, 0.40760392), (0.00392157, 0.00392157, 0.00392157)


@pytest.fixture(scope="module")
def golden():
    return load_golden("jpeg_mixed")


def names_for(target):
    """The fixture files a resize to `target` takes: 640 x 16 is beyond the shrink limit of 16 for a height of 16."""
    return tuple(n for n in NAMES if not (n == "640x16_420" and target[0] * 16 < 640))


def files(golden, names=NAMES):
    return [golden["s_" + n] for n in names]


def mixed(golden, dev, names=NAMES, **kw):
    return jpeg.MixedJpegBatch.from_files(files(golden, names), **kw).to(dev)


@pytest.fixture(scope="module")
def alone(golden, dev):
    """Every fixture file through the EXISTING uniform calls in a batch of one: {name: pixels [H][W][3]} and
    {(name, target): resized [H2][W2][3]} on the host, computed once."""
    px, rs = {}, {}
    for n in NAMES:
        one = ops.decode_jpeg(jpeg.JpegBatch.from_files([golden["s_" + n]]).to(dev), scan="serial")
        px[n] = one[0].cpu()
        for t in TARGETS:
            if n in names_for(t):
                rs[n, t] = ops.resize_u8(one, t)[0].cpu()
    return px, rs


def _same(got, want, what=""):
    want = torch.as_tensor(np.asarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {want.numel()} differ, first at {bad[0].tolist()}: got "
                             f"{got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


# ---- the decoder ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan,chunk_bytes", ROUTES)
def test_decode_is_pils_and_the_uniform_decoders(golden, dev, alone, scan, chunk_bytes):
    views, status = ops.decode_jpeg_mixed(mixed(golden, dev), check=False, scan=scan, chunk_bytes=chunk_bytes)
    assert status.dtype == torch.int32 and status.tolist() == [0] * 9 and ops.last_jpeg_route == scan
    assert len(views) == 9
    base = views[0].untyped_storage().data_ptr()
    for n, v in zip(NAMES, views):
        assert v.is_contiguous() and v.untyped_storage().data_ptr() == base        # views into ONE packed buffer
        _same(v, golden["y_" + n], n)
        _same(v, alone[0][n], n)
    again = ops.decode_jpeg_mixed(mixed(golden, dev), scan=scan, chunk_bytes=chunk_bytes)        # check=True
    assert all(torch.equal(a, b) for a, b in zip(again, views))


def test_auto_takes_the_chunked_route_by_the_longest_segment(golden, dev, alone):
    b = mixed(golden, dev)
    assert b.max_segment_bytes >= jpeg.CHUNKED_MIN_BYTES
    ops.decode_jpeg_mixed(b)
    assert ops.last_jpeg_route == "chunked" and ops.last_jpeg_rounds.numel() == b.segments.shape[0]
    assert int(ops.last_jpeg_rounds.max()) >= 2 and int(ops.last_jpeg_rounds.min()) >= 1
    small = mixed(golden, dev, NAMES[:4])
    assert small.max_segment_bytes < jpeg.CHUNKED_MIN_BYTES
    views = ops.decode_jpeg_mixed(small)
    assert ops.last_jpeg_route == "serial" and ops.last_jpeg_rounds is None
    for n, v in zip(NAMES[:4], views):
        _same(v, alone[0][n], n)


# ---- decode + resize ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", TARGETS)
def test_decode_resize_is_pils_resize_of_pils_decode(golden, dev, alone, target):
    names = names_for(target)
    t = TARGETS.index(target)
    u8, status = ops.decode_resize_jpeg(mixed(golden, dev, names, target=target), target, check=False)
    assert u8.shape == (len(names), *target, 3) and u8.dtype == torch.uint8 and status.tolist() == [0] * len(names)
    for i, n in enumerate(names):
        _same(u8[i], golden[f"r{t}_{n}"], n)
        _same(u8[i], alone[1][n, target], n)
    if target == (48, 64):
        _same(u8[1], golden["y_48x64_grey"], "the identity")
    f32 = ops.decode_resize_jpeg(mixed(golden, dev, names), target, out="float", mean=MEAN, std=STD)
    assert f32.shape == (len(names), 3, *target) and f32.dtype == torch.float32
    want = ((u8.cpu().float() / 255.0 - torch.tensor(MEAN)) / torch.tensor(STD)).permute(0, 3, 1, 2)   # on the host
    assert torch.equal(f32.cpu(), want.contiguous())
    # the default normalisation is the loader's, as for resize_u8
    dflt = ops.decode_resize_jpeg(mixed(golden, dev, names), target, out="float")
    assert torch.equal(dflt, ops.resize_u8(u8, target, out="float"))
    for scan, cb in ROUTES:
        other = ops.decode_resize_jpeg(mixed(golden, dev, names), target, scan=scan, chunk_bytes=cb)
        assert torch.equal(other, u8), (scan, cb)


def test_the_shrink_limit_holds_per_image(golden, dev):
    with pytest.raises(ValueError, match=r"image 6 is 640 x 16.*limit of 16"):
        ops.decode_resize_jpeg(mixed(golden, dev), (16, 16))
    with pytest.raises(ValueError, match=r"image 6 is 640 x 16.*limit of 16"):
        jpeg.MixedJpegBatch.from_files(files(golden), target=(39, 72))
    assert ops.decode_resize_jpeg(mixed(golden, dev), (40, 10)).shape == (9, 40, 10, 3)     # 640 = 16 * 40, 160 = 160


def test_resize_u8_mixed_alone(golden, dev, alone):
    """The mixed resize on a packed buffer that did not come from the decoder: Pillow's pixels, packed by hand."""
    sizes = [golden["y_" + n].shape[:2] for n in NAMES]
    geom, totals = jpeg.mixed_layout(sizes)
    packed = np.full(totals[2] + 100, 255, np.uint8)          # a longer buffer, and 255 in the gaps
    for off, n in zip(jpeg.geom_pixel_offsets(geom), NAMES):
        packed[off:off + golden["y_" + n].size] = golden["y_" + n].reshape(-1)
    got = ops.resize_u8_mixed(torch.from_numpy(packed).to(dev), sizes, (40, 72))
    for i, n in enumerate(NAMES):
        _same(got[i], golden[f"r0_{n}"], n)
    up = ops.resize_u8_mixed(torch.from_numpy(packed).to(dev), torch.tensor(sizes), (700, 130))      # upscaling
    for i, n in enumerate(NAMES):
        one = ops.resize_u8(torch.from_numpy(golden["y_" + n]).to(dev)[None], (700, 130))
        assert torch.equal(up[i], one[0]), n


# ---- position independence, determinism -----------------------------------------------------------------------------
def test_a_file_gives_the_same_bytes_wherever_it_stands(golden, dev, alone):
    target = (40, 72)
    for order in ORDERS:
        names = [NAMES[i] for i in order]
        b = mixed(golden, dev, names)
        views = ops.decode_jpeg_mixed(b)
        dense = ops.decode_resize_jpeg(b, target)
        for i, n in enumerate(names):
            _same(views[i], alone[0][n], (order, n))
            _same(dense[i], alone[1][n, target], (order, n))
    for n in NAMES:        # a batch of one, through the mixed entry
        b = mixed(golden, dev, [n])
        _same(ops.decode_jpeg_mixed(b)[0], alone[0][n], n)
        _same(ops.decode_resize_jpeg(b, target)[0], alone[1][n, target], n)


def test_two_runs_give_identical_bits(golden, dev):
    runs = []
    for _ in range(2):
        b = mixed(golden, dev)
        views, st = ops.decode_jpeg_mixed(b, check=False)
        runs.append((torch.cat([v.reshape(-1) for v in views]).clone(), st.clone(),
                     ops.decode_resize_jpeg(b, (40, 72), out="float")))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- damage ---------------------------------------------------------------------------------------------------------
def test_a_damaged_stream_in_the_middle_is_reported_and_hurts_nobody(golden, dev, alone):
    base = golden["s_120x160_420"]
    p = jpeg.parse(base)
    cut = base[:p.scan_begin + 3000]
    xor = golden["s_120x160_420_rstrow"].copy()
    xor[jpeg.parse(xor).scan_begin + 3000] ^= 0x5A       # (the numpy model reports a coefficient overrun for it)
    assert jpeg.parse(cut).device and jpeg.parse(xor).device
    names = list(NAMES)
    batch = files(golden)
    batch[4:4] = [cut, xor]                      # positions 4 and 5, between good files
    names[4:4] = [None, None]
    for scan, cb in ROUTES:
        b = jpeg.MixedJpegBatch.from_files(batch).to(dev)
        views, status = ops.decode_jpeg_mixed(b, check=False, scan=scan, chunk_bytes=cb)
        status = status.tolist()
        assert status[4] == jpeg.ST_OUT_OF_BYTES and status[5] == jpeg.ST_OVERRUN, (scan, cb, status)
        assert [s for i, s in enumerate(status) if i not in (4, 5)] == [0] * 9
        for n, v in zip(names, views):
            if n is not None:
                _same(v, alone[0][n], (scan, cb, n))
        # what was decoded in front of the cut is still there
        _same(views[4][:8], alone[0]["120x160_420"][:8], "in front of the cut")
        dense, st2 = ops.decode_resize_jpeg(b, (40, 72), check=False, scan=scan, chunk_bytes=cb)
        assert st2.tolist() == status
        for i, n in enumerate(names):
            if n is not None:
                _same(dense[i], alone[1][n, (40, 72)], (scan, cb, n))
    with pytest.raises(ValueError, match=r"image 4 \(ran out of bytes\).*image 5"):
        ops.decode_jpeg_mixed(jpeg.MixedJpegBatch.from_files(batch).to(dev))
    with pytest.raises(ValueError, match=r"decode_resize_jpeg: damaged JPEG streams: image 4 \(ran out of bytes\)"):
        ops.decode_resize_jpeg(jpeg.MixedJpegBatch.from_files(batch).to(dev), (40, 72))


def test_an_inconsistent_table_row_is_status_5_and_hurts_nobody(golden, dev, alone):
    """Rows of the device's geometry table overwritten before the call: the kernels skip those images (status 5) and
    decode the others as ever (every such row fails the kernels' check before any access: the host program of
    tests/test_jpeg_mixed_cpu.py runs the same rows under the sanitizers)."""
    b = mixed(golden, dev, DEVICE)
    hurt = b.dev_geom.clone()
    hurt[1, 0] = 70000                   # a height outside its range
    hurt[3, 2] = 1 << 30                 # a coefficient base behind the workspace
    hurt[5, 4] = b.totals[2] - 100       # a pixel offset whose image passes the end of the packed buffer
    b.dev_geom = hurt
    views, status = ops.decode_jpeg_mixed(b, check=False, scan="serial")
    assert status.tolist() == [0, 5, 0, 5, 0, 5, 0]
    for i in (0, 2, 4, 6):
        _same(views[i], alone[0][DEVICE[i]], DEVICE[i])
    _, status = ops.decode_jpeg_mixed(b, check=False, scan="chunked", chunk_bytes=16)
    assert status.tolist() == [0, 5, 0, 5, 0, 5, 0]
    with pytest.raises(ValueError, match=r"image 1 \(geometry table inconsistent\)"):
        ops.decode_jpeg_mixed(b)
    # the resize: an image whose row disagrees with the host's sizes reads nothing and comes out as zero bytes
    good = mixed(golden, dev, DEVICE)
    packed, _ = ops._decode_jpeg_mixed_packed(good, "serial", None)
    geom = good.geom.clone()
    geom[2, 1] = 9999                                            # wider than any image of the host's sizes
    geom[4, 5] = 3                                               # an offset of 12 GiB
    out = ops._resize_u8_mixed(packed, geom, good.sizes.numpy(), 40, 72, "uint8", MEAN, STD, dev)
    assert int(out[2].max()) == 0 and int(out[4].max()) == 0
    for i in (0, 1, 3, 5, 6):
        _same(out[i], alone[1][DEVICE[i], (40, 72)], DEVICE[i])


# ---- the kinds of batches -------------------------------------------------------------------------------------------
def test_batches_all_on_the_host_all_on_the_device_and_of_one_image(golden, dev, alone):
    for names in (NAMES[7:], DEVICE, ("9x8_444",), ("24x30_png",)):
        b = mixed(golden, dev, names)
        views, status = ops.decode_jpeg_mixed(b, check=False)
        assert status.tolist() == [0] * len(names)
        dense = ops.decode_resize_jpeg(b, (48, 64))
        for i, n in enumerate(names):
            _same(views[i], golden["y_" + n], n)
            _same(dense[i], golden[f"r1_{n}"], n)


def test_a_uniform_batch_equals_the_uniform_calls(golden, dev):
    same = ["120x160_420", "120x160_420_rstrow", "120x160_420"]
    b = mixed(golden, dev, same)
    assert b.uniform
    u = jpeg.JpegBatch.from_files(files(golden, same)).to(dev)
    for scan, cb in ROUTES:
        want = ops.decode_jpeg(u, scan=scan, chunk_bytes=cb)
        views = ops.decode_jpeg_mixed(b, scan=scan, chunk_bytes=cb)
        for i in range(3):
            assert torch.equal(views[i], want[i]), (scan, cb, i)
        for target in TARGETS:
            for out in ("uint8", "float"):
                got = ops.decode_resize_jpeg(b, target, out=out, scan=scan, chunk_bytes=cb)
                assert torch.equal(got, ops.resize_u8(want, target, out=out)), (scan, cb, target, out)
                # a plain JpegBatch takes the uniform calls
                assert torch.equal(ops.decode_resize_jpeg(u, target, out=out, scan=scan, chunk_bytes=cb), got)


# ---- the loader and the extraction loop -----------------------------------------------------------------------------
def _write_files(golden, tmp_path):
    """Six files of four sizes in tmp_path, one of them progressive (a size of its own), and their records."""
    names = ["48x64_grey", "64x48_422", "120x160_420", "40x56_progressive", "120x160_420_rstrow", "64x48_422"]
    records = []
    for j, n in enumerate(names):
        (tmp_path / f"m{j}.jpg").write_bytes(golden["s_" + n].tobytes())
        records.append((f"m{j}.jpg", j, 0.0, 0.0))
    return records


def _loaders(records, root):
    from ibl.utils.data import get_transformer_test
    from ibl.utils.data.preprocessor import Preprocessor
    mixed_files = torch.utils.data.DataLoader(
        Preprocessor(records, root=str(root), raw=True), batch_size=6, num_workers=0, shuffle=False,
        collate_fn=functools.partial(jpeg.collate_mixed, target=(48, 64)))
    pillow = torch.utils.data.DataLoader(
        Preprocessor(records, root=str(root), transform=get_transformer_test(48, 64, as_uint8=True)),
        batch_size=6, num_workers=0, shuffle=False)
    return mixed_files, pillow


def _model(state_dict, dev):
    import hubconf
    model = hubconf.vgg16_netvlad()
    model.load_state_dict(state_dict)
    return model.to(dev).eval()


def test_extract_features_from_a_folder_of_mixed_sizes(golden, dev, state_dict, tmp_path):
    from ibl.evaluators import extract_features
    records = _write_files(golden, tmp_path)
    mixed_files, pillow = _loaders(records, tmp_path)
    model = _model(state_dict, dev)
    want = extract_features(model, pillow, records, gpu=dev.index)
    got = extract_features(model, mixed_files, records, gpu=dev.index, input_decode=True, input_resize=(48, 64))
    assert list(got) == list(want) == [r[0] for r in records]
    for f in want:
        assert torch.equal(got[f], want[f]), f
    assert torch.equal(want["m1.jpg"], want["m5.jpg"]) and len({tuple(v.tolist()) for v in want.values()}) == 5
    with pytest.raises(ValueError, match="needs input_resize"):
        extract_features(model, mixed_files, records, gpu=dev.index, input_decode=True)
    from openibl_amd.augment import Resize
    with pytest.raises(ValueError, match="keep_aspect"):
        extract_features(model, mixed_files, records, gpu=dev.index, input_decode=True,
                         input_resize=Resize(48, 64, keep_aspect=True, out="uint8"))


def test_extract_features_lists_the_damaged_file_of_a_mixed_folder(golden, dev, state_dict, tmp_path):
    from ibl.evaluators import extract_features
    records = _write_files(golden, tmp_path)
    base = golden["s_120x160_420"]
    (tmp_path / "m2.jpg").write_bytes(base[:jpeg.parse(base).scan_begin + 3000].tobytes())
    mixed_files, _ = _loaders(records, tmp_path)
    with pytest.raises(RuntimeError, match=r"1 damaged JPEG file\(s\): m2.jpg \(ran out of bytes\)"):
        extract_features(_model(state_dict, dev), mixed_files, records, gpu=dev.index, input_decode=True,
                         input_resize=(48, 64))
