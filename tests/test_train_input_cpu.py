"""Training tuples from the files' bytes, without a GPU: the fixture tests/golden/train_input.npz against the chained
numpy models (decode -> jitter -> resize), jpeg.collate_tuples, and the refusals of ops.decode_jitter_resize_jpeg,
augment.DecodeJpeg / ColorJitter / Resize / Compose on packed batches and the trainers' branch for file bytes."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import color_jitter_ref as cj
from helpers import jpeg_ref
from helpers import resize_u8_ref as rs

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("37x53_420", "48x64_grey", "64x48_422", "9x8_444", "120x160_420", "120x160_420_rstrow", "640x16_420",
         "40x56_progressive", "24x30_png")
DEVICE = NAMES[:7]
TARGETS = {"t": (32, 48), "u": (48, 32)}


@pytest.fixture(scope="module")
def mixed():
    return load_golden("jpeg_mixed")


@pytest.fixture(scope="module")
def golden():
    return load_golden("train_input")


def items_of(mixed, names):
    return [(torch.from_numpy(mixed["s_" + n]), n, i, 0.5 * i, 1.5) for i, n in enumerate(names)]


# ---- 1. the fixture -------------------------------------------------------------------------------------------------
def test_fixture_has_the_records_it_is_there_for(golden, mixed):
    assert tuple(str(n) for n in golden["names"]) == NAMES == tuple(str(n) for n in mixed["names"])
    assert str(golden["pil_version"]) and (ROOT / "tests" / "golden" / "train_input.npz").stat().st_size < 100 << 10
    rec = golden["records"]
    assert rec.shape == (9, 8) and rec.dtype == np.int32
    orders = rec[:, :4].tolist()
    assert {o.index(cj.CONTRAST) for o in orders if cj.CONTRAST in o} == {0, 1, 2, 3}     # contrast at every place
    assert any(cj.CONTRAST not in o and any(c >= 0 for c in o) for o in orders)           # one without contrast
    assert [-1, -1, -1, -1] in orders                                                     # one with every op skipped
    f = rec[:, 4:7].view(np.float32)
    assert (f >= 0.3).all() and (f <= 1.7).all() and ((rec[:, 7] >= 0) & (rec[:, 7] <= 255)).all()
    for key, (h, w) in TARGETS.items():
        for n in NAMES:
            assert golden[f"{key}_{n}"].shape == (h, w, 3) and golden[f"{key}_{n}"].dtype == np.uint8
    # the record with every op skipped is the plain resize of the decoded bytes
    skipped = NAMES[orders.index([-1, -1, -1, -1])]
    assert np.array_equal(golden["t_" + skipped], rs.pil_resize(mixed["y_" + skipped], 32, 48))


def test_chained_numpy_models_reproduce_the_fixture(golden, mixed):
    """decode (jpeg_ref, the files the device decodes; Pillow's bytes for the two of the host route) -> jitter
    (color_jitter_ref) -> resize (resize_u8_ref): the models the kernels are held to, chained, give Pillow's bytes."""
    for n, name in enumerate(NAMES):
        rgb = jpeg_ref.decode(mixed["s_" + name]).rgb if name in DEVICE else mixed["y_" + name]
        assert np.array_equal(rgb, mixed["y_" + name]), name
        jittered = cj.model_jitter(rgb, *cj.unpack_record(golden["records"][n]))
        for key, (h, w) in TARGETS.items():
            assert np.array_equal(rs.resize(jittered, h, w), golden[f"{key}_{name}"]), (name, key)


# ---- 2. collate_tuples ----------------------------------------------------------------------------------------------
def tuples_of(mixed, B, N, names=NAMES):
    """B tuples of N items over the fixture's files, file k = names[k % len(names)]."""
    flat = [(torch.from_numpy(mixed["s_" + names[k % len(names)]]), f"{names[k % len(names)]}#{k}", k, 0.5 * k, 1.5)
            for k in range(B * N)]
    return [flat[b * N:(b + 1) * N] for b in range(B)]


def test_collate_tuples_is_one_mixed_batch_in_tuple_major_order(mixed):
    from torch.utils.data import default_collate
    from openibl_amd import jpeg
    B, N = 3, 4
    items = tuples_of(mixed, B, N)
    out = jpeg.collate_tuples(items)
    batch = out[0]
    assert isinstance(out, list) and isinstance(batch, jpeg.MixedJpegBatch) and batch.tuples == (B, N)
    assert batch.n == len(batch) == B * N and not batch.uniform
    order = [NAMES[k % 9] for k in range(B * N)]
    want = jpeg.MixedJpegBatch.from_files([mixed["s_" + n] for n in order])
    for name in jpeg.MixedJpegBatch._TENSORS:
        assert torch.equal(getattr(batch, name), getattr(want, name)), name
    assert torch.equal(batch.sizes, want.sizes) and batch.totals == want.totals and batch.reasons == want.reasons
    # the host-route slots: the progressive file and the PNG, at their tuple-major positions
    assert batch.host_index.tolist() == [7, 8] and batch.reasons[7] == "progressive" and batch.reasons[9] == ""
    assert batch.dev_index.tolist() == [0, 1, 2, 3, 4, 5, 6, 9, 10, 11]
    # the other fields as default_collate collates a tuple loader's batch: one entry per tuple position
    rest = out[1:]
    ref = default_collate([[tuple(it[1:]) for it in t] for t in items])
    assert len(rest) == N == len(ref)
    for n in range(N):
        fnames, pids, x, y = rest[n]
        assert list(fnames) == [f"{NAMES[(b * N + n) % 9]}#{b * N + n}" for b in range(B)] == list(ref[n][0])
        assert pids.tolist() == [b * N + n for b in range(B)] and torch.equal(x, ref[n][2]) and y.shape == (B,)
    assert jpeg.tuple_names(out) == [f"{NAMES[k % 9]}#{k}" for k in range(B * N)]
    # always mixed, also when every size agrees
    same = jpeg.collate_tuples(tuples_of(mixed, 2, 2, names=("120x160_420", "120x160_420_rstrow")))[0]
    assert isinstance(same, jpeg.MixedJpegBatch) and same.uniform and same.tuples == (2, 2)
    # bare byte items (no other fields)
    bare = jpeg.collate_tuples([[(it[0],) for it in t] for t in items])
    assert len(bare) == 1 and bare[0].tuples == (B, N)


def test_collate_tuples_checks_the_shrink_limit_and_the_tuple_lengths(mixed):
    from openibl_amd import jpeg
    items = tuples_of(mixed, 2, 4)                    # file 6 is 640 x 16
    with pytest.raises(ValueError, match=r"image 6 is 640 x 16.*32 x 48.*limit of 16"):
        functools.partial(jpeg.collate_tuples, target=(32, 48))(items)
    assert jpeg.collate_tuples(items, target=(40, 48))[0].n == 8          # 640 = 16 * 40
    assert jpeg.collate_tuples(items)[0].n == 8                           # without a target the device call raises
    with pytest.raises(ValueError, match="tuple 1 has 3 images, tuple 0 has 4"):
        jpeg.collate_tuples([items[0], items[1][:3]])
    with pytest.raises(ValueError, match="empty"):
        jpeg.collate_tuples([])
    with pytest.raises(ValueError, match="empty"):
        jpeg.collate_tuples([[], []])


def test_collated_tuples_move_and_pin_like_any_batch(mixed):
    from openibl_amd import jpeg
    b = jpeg.collate_tuples(tuples_of(mixed, 2, 3))[0]
    c = b.to("cpu")
    assert c is not b and c.tuples == (2, 3) and c.n == 6 and torch.equal(c.scan, b.scan)
    if torch.cuda.is_available():
        p = b.pin_memory()
        assert p.is_pinned() and p.tuples == (2, 3)


# ---- 3. ops and augment ---------------------------------------------------------------------------------------------
def test_decode_jitter_resize_checks_its_arguments_and_has_no_cpu_fallback(mixed):
    from openibl_amd import jpeg, ops
    from openibl_amd.lib import OpenIBLAmdError
    b = jpeg.MixedJpegBatch.from_files([mixed["s_" + n] for n in NAMES])
    one = jpeg.JpegBatch.from_files([mixed["s_9x8_444"]])
    rec = torch.zeros((9, 8), dtype=torch.int32)
    for call in (lambda: ops.decode_jitter_resize_jpeg(b, None, (48, 32)),
                 lambda: ops.decode_jitter_resize_jpeg(b, rec, (48, 32), out="uint8", check=False),
                 lambda: ops.decode_jitter_resize_jpeg(one, rec[:1], (16, 16))):
        with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="MixedJpegBatch or a JpegBatch"):
        ops.decode_jitter_resize_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), None, (16, 16))
    with pytest.raises(ValueError, match="size must be"):
        ops.decode_jitter_resize_jpeg(b, rec, 48)
    with pytest.raises(ValueError, match="out must be"):
        ops.decode_jitter_resize_jpeg(b, rec, (48, 32), out="half")
    with pytest.raises(ValueError, match=r"image 6 is 640 x 16.*32 x 48.*limit of 16"):
        ops.decode_jitter_resize_jpeg(b, rec, (32, 48))
    with pytest.raises(ValueError, match=r"params must be \[9\]\[8\]"):
        ops.decode_jitter_resize_jpeg(b, rec[:4], (48, 32))
    with pytest.raises(ValueError, match="int32"):
        ops.decode_jitter_resize_jpeg(b, rec.float(), (48, 32))
    with pytest.raises(ValueError, match=r"params must be \[1\]\[8\]"):
        ops.decode_jitter_resize_jpeg(one, rec, (16, 16))
    with pytest.raises(ValueError, match="scan must be one of"):
        ops.decode_jitter_resize_jpeg(b, rec, (48, 32), scan="nope")


def packed_images(sizes=((8, 8), (5, 7))):
    from openibl_amd import jpeg, ops
    geom, totals = jpeg.mixed_layout(sizes)
    return ops.PackedImages(torch.zeros(totals[2], dtype=torch.uint8), np.asarray(sizes, np.int32),
                            torch.from_numpy(geom), torch.zeros(len(sizes), dtype=torch.int32))


def test_augment_stages_take_a_packed_batch_and_keep_their_errors(mixed):
    from openibl_amd import jpeg
    from openibl_amd.augment import ColorJitter, Compose, DecodeJpeg, Resize
    from openibl_amd.lib import OpenIBLAmdError
    with pytest.raises(ValueError, match="scan must be one of"):
        DecodeJpeg(scan="fast")
    d = DecodeJpeg()
    assert d.out == "uint8" and d.scan == "auto" and d.last_status is None and "auto" in repr(d)
    with pytest.raises(ValueError, match="MixedJpegBatch or a JpegBatch"):
        d(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    b = jpeg.MixedJpegBatch.from_files([mixed["s_" + n] for n in NAMES])
    for batch in (b, jpeg.JpegBatch.from_files([mixed["s_9x8_444"]])):
        with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
            d(batch)
    p = packed_images()
    assert len(p) == 2
    # the jitter works in place and needs out='uint8'; with every op disabled the object passes through untouched
    with pytest.raises(ValueError, match="in place and needs out='uint8'"):
        ColorJitter(0.7, 0.7, 0.7, 0.5)(p)
    off = ColorJitter(out="uint8")
    assert off(p) is p and off.last_records is None
    j = ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8", generator=torch.Generator().manual_seed(4))
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        j(p)
    assert j.last_records.shape == (2, 8)                         # one record per image of the packed batch
    with pytest.raises(ValueError, match=r"params must be \[2\]\[8\]"):
        j(p, records=torch.zeros((3, 8), dtype=torch.int32))
    # the resize: a fixed target only
    with pytest.raises(ValueError, match="keep_aspect"):
        Resize(32, 48, keep_aspect=True)(p)
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        Resize(32, 48)(p)
    with pytest.raises(ValueError, match=r"image 0 is 8 x 17.*1 x 1.*limit of 16"):
        Resize(1, 1, out="uint8")(packed_images(((8, 17),)))
    # every existing call pattern keeps its behaviour and its errors
    with pytest.raises(ValueError, match=r"\[N\]\[H\]\[W\]\[3\]"):
        Resize(32, 48)(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ColorJitter(0.7, 0.7, 0.7, 0.5)(torch.zeros(2, 4, 6, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="hands float on"):
        Compose(DecodeJpeg(), ColorJitter(0.7, 0.7, 0.7, 0.5), Resize(32, 48))


def test_compose_sends_records_to_the_jitter_wherever_it_stands():
    from openibl_amd.augment import ColorJitter, Compose

    class Spy(ColorJitter):
        def __call__(self, x, **kw):
            self.seen = kw
            return x + ["jitter"]

    def stage(name):
        def run(x, **kw):
            assert not kw, (name, kw)
            return x + [name]
        run.out = "uint8"
        return run
    rec = torch.zeros((1, 8), dtype=torch.int32)
    spy = Spy(out="uint8")
    assert Compose(stage("decode"), spy, stage("resize"))([], records=rec) == ["decode", "jitter", "resize"]
    assert spy.seen == {"records": rec}
    spy = Spy(out="uint8")
    assert Compose(spy, stage("resize"))([], records=rec) == ["jitter", "resize"] and spy.seen == {"records": rec}
    spy = Spy(out="uint8")
    assert Compose(stage("decode"), spy)([]) == ["decode", "jitter"] and spy.seen == {}
    # as before: without a jitter stage, and for any other keyword, the first stage gets the arguments

    def first(x, **kw):
        return x + [sorted(kw)]
    first.out = "uint8"
    assert Compose(first, stage("resize"))([], records=rec) == [["records"], "resize"]
    assert Compose(first, spy)([], other=1) == [["other"], "jitter"]


# ---- 4. the trainers ------------------------------------------------------------------------------------------------
def test_trainers_refuse_file_bytes_without_the_chain_that_decodes_them(mixed):
    from ibl.trainers import SFRSTrainer, Trainer, _file_chain, _is_file_tuples
    from openibl_amd import jpeg
    from openibl_amd.augment import ColorJitter, Compose, DecodeJpeg, Resize
    batch = jpeg.collate_tuples(tuples_of(mixed, 2, 4), target=(48, 32))
    assert _is_file_tuples(batch)
    plain = jpeg.collate_mixed(items_of(mixed, NAMES[:3]))
    assert not _is_file_tuples(plain) and not _is_file_tuples([(torch.zeros(2, 3, 4, 4), ["a", "b"])])
    jit = ColorJitter(0.7, 0.7, 0.7, 0.5, out="uint8")
    wrong = (None, ColorJitter(0.7, 0.7, 0.7, 0.5), Compose(jit, Resize(48, 32)), Compose(DecodeJpeg(), jit),
             Compose(DecodeJpeg(), jit, Resize(48, 32, keep_aspect=True)),
             Compose(DecodeJpeg(), jit, Resize(48, 32, out="uint8")))
    for augment in wrong:
        for trainer in (Trainer(None, augment=augment), SFRSTrainer(None, None, neg_num=1, augment=augment)):
            with pytest.raises(ValueError, match="starts with DecodeJpeg and ends with a Resize without keep_aspect"):
                trainer._parse_data(batch)
    # the right chain passes (the move to the device comes next; there is none here)
    chain = Compose(DecodeJpeg(), jit, Resize(48, 32))
    assert _file_chain(chain) is chain
    # opt-in and off by default; every other input takes the path it took
    assert Trainer(None).prefetch is False and SFRSTrainer(None, None).prefetch is False
    assert Trainer(None, prefetch=True).prefetch is True
    fl = [(torch.zeros((2, 3, 4, 6)), ["name"] * 2) for _ in range(4)]
    with pytest.raises(ValueError, match="uint8 tuples"):
        Trainer(None, augment=chain)._parse_data(fl)


def test_damaged_files_are_named_from_the_pinned_statuses():
    import collections
    from ibl.trainers import _check_files
    pending = collections.deque()
    _check_files(pending)                                                        # nothing pending: nothing to do
    pending.append((torch.zeros(3, dtype=torch.int32), ["a", "b", "c"]))
    pending.append((torch.tensor([0, 3, 0, 1], dtype=torch.int32), ["p.jpg", "q.jpg", "r.jpg", "s.jpg"]))
    pending.append((torch.tensor([5], dtype=torch.int32), None))
    _check_files(pending)                                                        # the oldest batch: clean
    assert len(pending) == 2
    with pytest.raises(RuntimeError, match=r"2 damaged JPEG file\(s\): q.jpg \(ran out of bytes\), s.jpg \(bad Huffman"):
        _check_files(pending)
    assert not pending
    pending.append((torch.tensor([5], dtype=torch.int32), None))
    with pytest.raises(RuntimeError, match=r"item 0 \(geometry table inconsistent\)"):
        _check_files(pending)
