"""JPEG batches of mixed stored sizes (csrc/jpeg_mixed.h, csrc/jpeg.hip, oibl_resize_u8_mixed), without a GPU:
the layout function through the C ABI and its numpy twin, the geometry table's device-side check and the mixed entropy
stage as a host program under the address and undefined-behaviour sanitizers, the C ABI's validation, MixedJpegBatch
and collate_mixed, and the refusals of the Python layers."""
import ctypes
import functools
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("37x53_420", "48x64_grey", "64x48_422", "9x8_444", "120x160_420", "120x160_420_rstrow", "640x16_420",
         "40x56_progressive", "24x30_png")
SIZES = ((37, 53), (48, 64), (64, 48), (9, 8), (120, 160), (120, 160), (640, 16), (40, 56), (24, 30))
DEVICE = NAMES[:7]
NEW = ("oibl_jpeg_mixed_layout", "oibl_jpeg_decode_mixed_workspace_bytes", "oibl_jpeg_decode_mixed",
       "oibl_resize_u8_mixed_workspace_bytes", "oibl_resize_u8_mixed")


@pytest.fixture(scope="module")
def golden():
    return load_golden("jpeg_mixed")


def files(golden, names=NAMES):
    return [golden["s_" + n] for n in names]


def test_fixture_is_the_set_the_index_computations_need(golden):
    from openibl_amd import jpeg
    assert tuple(golden["names"]) == NAMES and str(golden["pil_version"])
    assert golden["targets"].tolist() == [[40, 72], [48, 64], [16, 16]]
    assert (ROOT / "tests" / "golden" / "jpeg_mixed.npz").stat().st_size < 512 << 10
    for n, (h, w) in zip(NAMES, SIZES):
        assert golden["y_" + n].shape == (h, w, 3)
        p = jpeg.parse(golden["s_" + n])
        assert p.device == (n in DEVICE), (n, p.reason)
        for t, (h2, w2) in enumerate(golden["targets"].tolist()):
            assert (f"r{t}_{n}" in golden) == (h <= 16 * h2 and w <= 16 * w2)
    assert "r2_640x16_420" not in golden and sum(k.startswith("r2_") for k in golden) == 8
    free, rst = jpeg.parse(golden["s_120x160_420"]), jpeg.parse(golden["s_120x160_420_rstrow"])
    assert free.segments.shape[0] == 1 and free.scan.size > 6000           # several kB in one segment: many chunks
    assert rst.segments.shape[0] == 8 and rst.restart_interval == 10       # one restart per MCU row
    assert len(set(SIZES)) == 8                                        # a size of its own, but for the two 120 x 160


# ---- 1. the layout function -----------------------------------------------------------------------------------------
def c_layout(sizes):
    """oibl_jpeg_mixed_layout through ctypes -> (rc, geom [N][8], totals [6])."""
    from openibl_amd import lib
    h = lib.load()
    sizes = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = sizes.shape[0]
    geom = np.full((max(n, 1), 8), -7, np.int32)
    totals = (ctypes.c_size_t * 6)()
    rc = h.oibl_jpeg_mixed_layout(sizes.ctypes.data_as(ctypes.c_void_p), n, geom.ctypes.data_as(ctypes.c_void_p),
                                  totals)
    return rc, geom, [int(v) for v in totals]


def uniform_bytes(h, w):
    """(coefficient bytes, plane bytes) of one image in the uniform decoder: 6 + 3 bytes per MCU-padded pixel."""
    padded = (16 * ((h + 15) // 16)) * (16 * ((w + 15) // 16))
    return 6 * padded, 3 * padded


def test_layout_offsets_are_disjoint_ascending_and_aligned():
    from openibl_amd import jpeg
    rng = np.random.RandomState(5)
    for sizes in (SIZES, [(1, 1)], [(32768, 32768)], [(480, 640), (640, 480), (960, 1280), (1280, 960)] * 8,
                  rng.randint(1, 300, (200, 2)).tolist()):
        rc, geom, totals = c_layout(sizes)
        assert rc == 0
        pix = jpeg.geom_pixel_offsets(geom)
        end_blocks = end_pix = 0
        for (h, w), row, p in zip(sizes, geom.tolist(), pix.tolist()):
            cb, pb = uniform_bytes(h, w)
            assert row[:2] == [h, w] and row[6:] == [0, 0]
            assert row[2] == row[3] == end_blocks                 # back to back: ascending and disjoint
            assert row[2] * 128 % 512 == 0 and row[3] * 64 % 256 == 0     # a whole number of 16 x 16 MCU cells
            end_blocks += cb // 128
            assert end_blocks * 64 == row[3] * 64 + pb
            assert p % 64 == 0 and end_pix <= p < end_pix + 64    # the next multiple of 64 behind the last image
            end_pix = p + 3 * h * w
        assert totals[0] == sum(uniform_bytes(h, w)[0] for h, w in sizes)
        assert totals[1] == sum(uniform_bytes(h, w)[1] for h, w in sizes)
        assert totals[0] + totals[1] == sum(9 * (16 * ((h + 15) // 16)) * (16 * ((w + 15) // 16)) for h, w in sizes)
        assert totals[2] == end_pix
        assert totals[3] == max(4 * ((h + 15) // 16) * ((w + 15) // 16) for h, w in sizes)
        assert totals[4] == max(h for h, _ in sizes) and totals[5] == max(w for _, w in sizes)
        # the numpy twin the loader's workers use
        g2, t2 = jpeg.mixed_layout(sizes)
        assert np.array_equal(g2, geom) and list(t2) == totals


def test_layout_of_one_image_is_the_uniform_layout():
    from openibl_amd import lib
    h = lib.load()
    for H, W in ((48, 64), (37, 53), (9, 8), (480, 640), (1, 8)):
        rc, geom, totals = c_layout([(H, W)])
        assert rc == 0 and geom[0].tolist() == [H, W, 0, 0, 0, 0, 0, 0]
        assert totals[2] == 3 * H * W
        t = (ctypes.c_size_t * 6)(*totals)
        # the uniform chunked workspace: the same coefficients, statuses, rounds and planes
        assert h.oibl_jpeg_decode_mixed_workspace_bytes(t, 1, 3) == \
            h.oibl_jpeg_decode_chunked_workspace_bytes(1, H, W, 3, 64)


def test_layout_rejects_every_limit_with_a_message():
    from openibl_amd import jpeg, lib
    h = lib.load()
    for bad, word in (([(0, 8)], b"image 0 is 0 x 8"), ([(8, 8), (8, 32769)], b"image 1 is 8 x 32769"),
                      ([(8, 8), (-1, 8)], b"image 1 is -1 x 8"), ([(32768, 32768)] * 43, b"coefficient blocks")):
        rc, _, _ = c_layout(bad)
        assert rc == -1 and word in h.oibl_last_error(), (bad[:2], h.oibl_last_error())
        with pytest.raises(ValueError, match="image|blocks"):
            jpeg.mixed_layout(bad)
    # 42 of the largest images are fewer than 2^31 blocks.  (A block of 64 coefficients stands for at most 192 pixel
    # bytes, so fewer than 2^31 blocks are fewer than 2^39 pixel bytes: the limit of 2^40 packed pixel bytes holds
    # with them, and every pixel offset is 64-bit all the same.)
    rc, geom, totals = c_layout([(32768, 32768)] * 42)
    assert rc == 0 and totals[2] == 42 * 3 * 32768 * 32768 < 1 << 40
    assert int(jpeg.geom_pixel_offsets(geom)[41]) == 41 * 3 * 32768 * 32768 > 1 << 36 and geom[41, 5] == 30
    sizes = np.array([(0, 0)], np.int32)
    assert h.oibl_jpeg_mixed_layout(None, 1, sizes.ctypes.data_as(ctypes.c_void_p), (ctypes.c_size_t * 6)()) == -1
    assert b"null" in h.oibl_last_error()
    for n in (0, 65536, -3):
        assert h.oibl_jpeg_mixed_layout(sizes.ctypes.data_as(ctypes.c_void_p), n,
                                        sizes.ctypes.data_as(ctypes.c_void_p), (ctypes.c_size_t * 6)()) == -1
        assert b"N = " in h.oibl_last_error()


# ---- 2. the host program --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/helpers/jpeg_mixed_harness.cpp + csrc/jpeg_mixed.h + csrc/jpeg_chunked.h as a program of its own under
    -fsanitize=address,undefined; nothing is preloaded and no Python binding is involved."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert shutil.which(cxx) is not None or Path(cxx).exists(), "no host C++ compiler (g++ or the ROCm clang++)"
    exe = tmp_path_factory.mktemp("jpeg_mixed_harness") / "jpeg_mixed_harness"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "openibl_amd" / "csrc"),
                    str(ROOT / "tests" / "helpers" / "jpeg_mixed_harness.cpp"), "-o", str(exe)], check=True)

    def run(streams, chunk_bytes, overrides=()):
        """streams: files the parser sends to the device, as ONE batch -> (geom, totals, rows) with a row per image:
        (status serial, status chunked, status alone, ok, coef alone, coef serial, coef chunked)."""
        from openibl_amd import jpeg
        b = jpeg.MixedJpegBatch.from_files(streams)
        assert not b.host_index.numel(), b.reasons
        n, S = b.n, int(b.segments.shape[0])
        blob = [struct.pack("<5i", n, S, b.scan.numel(), chunk_bytes, len(overrides)),
                b.sizes.numpy().astype("<i4").tobytes(), b.records.numpy().tobytes(),
                b.segments.numpy().astype("<i4").tobytes(), b.scan.numpy().tobytes(),
                np.asarray(overrides, "<i4").reshape(-1, 3).tobytes()]
        fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
        fin.write_bytes(b"".join(blob))
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True,
                           env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
        assert r.returncode == 0, r.stderr[-3000:]
        raw = fout.read_bytes()
        geom = np.frombuffer(raw, "<i4", 8 * n).reshape(n, 8)
        totals = np.frombuffer(raw, "<i8", 6, 32 * n).tolist()
        assert np.array_equal(geom, b.geom.numpy()) and totals == list(b.totals)      # the numpy twin again
        at, rows = 32 * n + 48, []
        for _ in range(n):
            ss, sc, sa, ok, m = struct.unpack_from("<5i", raw, at)
            coefs = [np.frombuffer(raw, "<i2", m, at + 20 + 2 * m * k) for k in range(3)]
            at += 20 + 6 * m
            rows.append((ss, sc, sa, ok, *coefs))
        assert at == len(raw)
        return geom, totals, rows
    return run


ORDERS = (tuple(range(7)), (6, 5, 4, 3, 2, 1, 0), (4, 0, 6, 2, 5, 1, 3), (3, 3, 0, 4, 4, 6))


@pytest.mark.parametrize("chunk_bytes", [4, 16, 64])
def test_mixed_entropy_equals_every_image_alone_in_several_orders(golden, harness, chunk_bytes):
    seen = {}
    for order in ORDERS:
        names = [DEVICE[i] for i in order]
        _, _, rows = harness(files(golden, names), chunk_bytes)
        for name, (ss, sc, sa, ok, alone, serial, chunked) in zip(names, rows):
            assert (ss, sc, sa, ok) == (0, 0, 0, 1), (order, name)
            assert alone.size and np.array_equal(serial, alone) and np.array_equal(chunked, alone), (order, name)
            assert np.array_equal(seen.setdefault(name, alone), alone)                 # whatever the position


def damaged_streams(golden):
    """Truncations and single-byte corruptions of the fixture's device files that the parser still sends to the
    device (seeded: the same every run)."""
    from openibl_amd import jpeg
    rng = np.random.RandomState(77)
    out = []
    for i in range(60):
        base = golden["s_" + DEVICE[i % 7]]
        s0 = jpeg.parse(base).scan_begin
        hurt = base.copy()
        if i % 2:
            hurt = hurt[:rng.randint(s0 + 1, base.size - 2)]
        else:
            hurt[rng.randint(s0, base.size - 2)] ^= rng.randint(1, 256)
        if jpeg.parse(hurt).device:
            out.append(hurt)
    assert len(out) > 45
    return out


@pytest.mark.parametrize("chunk_bytes", [4, 64])
def test_damaged_streams_between_good_ones_run_clean_and_hurt_nobody(golden, harness, chunk_bytes):
    """Every third image of the batch is damaged: the program ends clean under the sanitizers, every image has the
    status of the image alone on both routes, the serial route its coefficients, and the good images both."""
    good, hurt = files(golden, DEVICE), damaged_streams(golden)
    batch, is_hurt = [], []
    for i, h in enumerate(hurt):
        batch += [good[i % 7], h, good[(i + 3) % 7]]
        is_hurt += [False, True, False]
    _, _, rows = harness(batch, chunk_bytes)
    n_damaged = 0
    for hurt_one, (ss, sc, sa, ok, alone, serial, chunked) in zip(is_hurt, rows):
        assert ok == 1 and ss == sa and sc == sa
        assert np.array_equal(serial, alone)
        if not hurt_one:
            assert sa == 0
        if sa == 0:
            assert np.array_equal(chunked, alone)
        n_damaged += sa != 0
    assert n_damaged > 35


def test_an_inconsistent_table_gives_status_5_and_touches_nothing_outside(golden, harness):
    """Rows of the geometry table overwritten behind the layout function: sides outside their range or beyond the
    batch's largest, bases and offsets that are negative or pass the end of their space.  The program ends clean under
    the sanitizers (its buffers have exactly the layout's sizes); every refused image has status 5 on both routes,
    and every image whose row was left alone decodes as it does alone."""
    names = list(DEVICE)
    _, totals, _ = harness(files(golden, names), 16)
    blocks = totals[1] // 64
    H, W, COEF, PLANE, LO, HI = range(6)
    cases = [(0, H, 0), (0, H, -5), (0, H, 32769), (0, H, 641), (1, W, 7), (1, W, 161), (1, W, 1 << 30),
             (2, COEF, -1), (2, COEF, blocks), (2, COEF, blocks - 3 * 16 + 1), (2, COEF, 0x7FFFFFFF),
             (3, PLANE, -1), (3, PLANE, blocks - 3 * 4 + 1), (4, LO, totals[2] - 3 * 120 * 160 + 1), (4, LO, -1),
             (4, HI, 1), (4, HI, -1), (4, HI, 256), (5, H, 136), (5, W, 176), (6, W, 32), (6, H, 33), (4, H, 100)]
    accepted = ((6, H, 33), (4, H, 100))
    for image, entry, value in cases:
        _, _, rows = harness(files(golden, names), 16, overrides=[(image, entry, value)])
        for i, (ss, sc, sa, ok, alone, serial, chunked) in enumerate(rows):
            if i == image and (image, entry, value) not in accepted:
                assert (ss, sc, ok, alone.size) == (5, 5, 0, 0), (image, entry, value)
            elif i == image:
                # a row that stays inside every space (a smaller image at the same place) is accepted: it decodes
                # something else, inside its own extent
                assert ok == 1
            else:
                assert (ss, sc, sa, ok) == (0, 0, 0, 1)
                assert np.array_equal(serial, alone) and np.array_equal(chunked, alone), (image, entry, value, i)
    # every row wrong at once, and a table whose rows all point at the first image's place
    _, _, rows = harness(files(golden, names), 64, overrides=[(i, COEF, blocks) for i in range(7)])
    assert all(r[:2] == (5, 5) for r in rows)
    _, _, rows = harness(files(golden, names), 64,
                         overrides=[(i, e, 0) for i in range(1, 7) for e in (COEF, PLANE, LO)])
    assert all(r[3] == 1 for r in rows)         # inside the spaces: accepted, overlapping, bounded


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------
def test_abi_declared_exported_bound_documented():
    from openibl_amd import lib
    header = (ROOT / "include" / "openibl_amd.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in NEW:
        assert name + "(" in header and name in lib.SIGNATURES and name in doc and hasattr(raw, name)


def test_decode_mixed_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(1024)           # never dereferenced: validation fails first
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    _, _, totals = c_layout([(48, 64), (37, 53), (64, 48), (9, 8)])
    good = dict(scan=p, n=100, rec=p, seg=p, S=4, mx=1, N=4, geom=p, totals=totals, cb=0, out=p, st=p, ws=p,
                wsb=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        t = None if a["totals"] is None else (ctypes.c_size_t * 6)(*a["totals"])
        return h.oibl_jpeg_decode_mixed(a["scan"], a["n"], a["rec"], a["seg"], a["S"], a["mx"], a["N"], a["geom"], t,
                                        a["cb"], a["out"], a["st"], a["ws"], a["wsb"], None)
    for key in ("scan", "rec", "seg", "geom", "totals", "out", "st"):
        assert call(**{key: None}) == -1 and b"null" in h.oibl_last_error(), key
    for cb in (3, 65537, -1, 1):
        assert call(cb=cb) == -1 and b"chunk_bytes" in h.oibl_last_error(), cb
    for kw in (dict(N=0), dict(N=65536), dict(S=3), dict(S=(1 << 28) + 1)):
        assert call(**kw) == -1 and b"bad shape" in h.oibl_last_error(), kw
    t = list(totals)
    for i, v in ((0, t[0] + 128), (1, t[1] + 64), (1, 0), (2, 0), (2, 1 << 40), (3, 0), (3, t[1]), (4, 0),
                 (4, 32769), (5, 0), (5, 32769)):
        wrong = list(t)
        wrong[i] = v
        assert call(totals=wrong) == -1 and b"totals" in h.oibl_last_error(), (i, v)
        assert h.oibl_jpeg_decode_mixed_workspace_bytes((ctypes.c_size_t * 6)(*wrong), 4, 4) == 0
    assert call(n=0) == -1 and call(n=1 << 31) == -1 and b"scan_len" in h.oibl_last_error()
    assert call(mx=0) == -1 and call(mx=5) == -1 and b"max_segments" in h.oibl_last_error()
    assert call(rec=p + 2) == -1 and call(st=p + 1) == -1 and call(geom=p + 2) == -1 and \
        b"aligned" in h.oibl_last_error()
    assert call(ws=None) == -1 and call(ws=p + 64) == -1 and b"256" in h.oibl_last_error()
    need = h.oibl_jpeg_decode_mixed_workspace_bytes((ctypes.c_size_t * 6)(*t), 4, 4)
    assert need == t[0] + t[1] + 512 and t[0] % 256 == 0 and t[1] % 256 == 0
    rc = call(wsb=need - 1)
    assert rc != 0 and rc != -1 and b"workspace" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "jpeg_decode_mixed")
    assert h.oibl_jpeg_decode_mixed_workspace_bytes(None, 4, 4) == 0
    assert h.oibl_jpeg_decode_mixed_workspace_bytes((ctypes.c_size_t * 6)(*t), 0, 4) == 0


def test_resize_mixed_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    mean = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    good = dict(x=p, nb=1000, geom=p, sizes=[(48, 64), (640, 16)], N=2, H2=40, W2=72, kind=0, mean=mean, std=mean,
                out=p, ws=p, wsb=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        s = None if a["sizes"] is None else np.ascontiguousarray(np.asarray(a["sizes"], np.int32))
        sp = None if s is None else s.ctypes.data_as(ctypes.c_void_p)
        return h.oibl_resize_u8_mixed(a["x"], a["nb"], a["geom"], sp, a["N"], a["H2"], a["W2"], a["kind"], a["mean"],
                                      a["std"], a["out"], a["ws"], a["wsb"], None)

    def query(sizes, N, H2, W2):
        s = np.ascontiguousarray(np.asarray(sizes, np.int32))
        return h.oibl_resize_u8_mixed_workspace_bytes(s.ctypes.data_as(ctypes.c_void_p), N, H2, W2)
    for key in ("x", "geom", "sizes", "out"):
        assert call(**{key: None}) == -1 and b"null" in h.oibl_last_error(), key
    for kw in (dict(N=0), dict(N=65536), dict(H2=0), dict(W2=32769), dict(sizes=[(48, 64), (0, 16)]),
               dict(sizes=[(32769, 64), (640, 16)])):
        assert call(**kw) == -1 and b"bad shape" in h.oibl_last_error(), kw
    assert call(nb=0) == -1 and call(nb=1 << 40) == -1 and b"packed_bytes" in h.oibl_last_error()
    # the per-image limit of 16: 640 -> 40 is exactly 16, 656 -> 40 is beyond it, and the message names the image
    assert call(sizes=[(48, 64), (656, 16)]) == -1
    msg = h.oibl_last_error()
    assert b"image 1" in msg and b"656 x 16" in msg and b"limit of 16" in msg
    assert call(sizes=[(48, 1153), (640, 16)]) == -1 and b"image 0" in h.oibl_last_error()
    assert query([(48, 64), (656, 16)], 2, 40, 72) == 0 and query([(48, 64), (640, 16)], 2, 40, 72) > 0
    assert call(kind=2) == -1 and b"out_kind" in h.oibl_last_error()
    assert call(kind=1, mean=None) == -1 and b"mean3_host" in h.oibl_last_error()
    assert call(kind=1, out=p + 2) == -1 and call(geom=p + 2) == -1 and b"aligned" in h.oibl_last_error()
    assert call(ws=None) == -1 and call(ws=p + 64) == -1 and b"256" in h.oibl_last_error()
    # rows of the batch's largest ksize: 64 -> 72 upscales (3 taps), 640 -> 40 has 2 * 16 + 1 = 33
    need = query(good["sizes"], 2, 40, 72)
    a256 = lambda v: (v + 255) // 256 * 256        # noqa: E731
    assert need == a256(2 * 72 * 2 * 4) + a256(2 * 72 * 3 * 4) + a256(2 * 40 * 2 * 4) + a256(2 * 40 * 33 * 4)
    rc = call(wsb=need - 1)
    assert rc != 0 and rc != -1 and b"workspace" in h.oibl_last_error()
    assert query(good["sizes"], 0, 40, 72) == 0 and query(good["sizes"], 2, 0, 72) == 0


def test_the_new_kernels_do_not_spill():
    from openibl_amd import build
    usage = build.resource_usage()
    mixed = {k: v for k, v in usage.items() if "jmix_" in k}
    assert sorted(n.split("jmix_")[1].split("_kernel")[0] for n in mixed) == ["chunk", "colour", "entropy", "idct"]
    resize = {k: v for k, v in usage.items() if "resize_mixed_" in k}
    assert len(resize) == 3, sorted(resize)                   # the table kernel and the two output kinds
    for name, u in {**mixed, **resize}.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 0) + u.get("AGPRs", 0) <= 128, (name, u)
    # the shared stage text compiles to the same budget in the uniform kernels as in the mixed ones
    for stage in ("entropy", "idct", "colour"):
        a = next(v for k, v in usage.items() if f"jpeg_{stage}_kernel" in k)
        b = next(v for k, v in mixed.items() if f"jmix_{stage}_kernel" in k)
        assert a["LDS"] == b["LDS"] and abs(a["VGPRs"] - b["VGPRs"]) <= 8, (stage, a, b)


# ---- 4. MixedJpegBatch and collate_mixed ----------------------------------------------------------------------------
def test_from_files_packs_the_fixture_batch(golden):
    from openibl_amd import jpeg
    b = jpeg.MixedJpegBatch.from_files(files(golden), target=(40, 72))
    assert len(b) == b.n == 9 and not b.is_cuda and not b.uniform
    assert b.sizes.dtype == torch.int32 and b.sizes.tolist() == [list(s) for s in SIZES]
    assert b.dev_index.tolist() == list(range(7)) and b.host_index.tolist() == [7, 8]
    assert b.reasons == ("",) * 7 + ("progressive", "not a JPEG file")
    assert b.records.shape == (7, jpeg.REC_BYTES) and b.segments.shape == (6 + 8, 2)
    assert b.max_segments == 8 and b.max_segment_bytes == int(jpeg.parse(golden["s_120x160_420"]).segments[0, 1])
    hdr = b.records[:, :64].numpy().view(np.int32)
    assert hdr[:, 13].tolist() == [0, 1, 2, 3, 4, 5, 13] and hdr[:, 14].tolist() == [1, 1, 1, 1, 1, 8, 1]
    for i, n in enumerate(DEVICE):       # segments are offsets into the packed scan
        p = jpeg.parse(golden["s_" + n])
        at = int(b.segments[hdr[i, 13], 0])
        assert np.array_equal(b.scan[at:at + 16].numpy(), p.scan[:16])
    # the table of all nine images, and the seven the device decodes: their own coefficient bases, the batch's pixels
    geom, totals = jpeg.mixed_layout(SIZES)
    assert np.array_equal(b.geom.numpy(), geom) and b.totals == totals
    dgeom, dtotals = jpeg.mixed_layout(SIZES[:7])
    assert np.array_equal(b.dev_geom[:, :4].numpy(), dgeom[:, :4])
    assert np.array_equal(b.dev_geom[:, 4:6].numpy(), geom[:7, 4:6])
    assert b.dev_totals == dtotals[:2] + (totals[2],) + dtotals[3:]
    # the host slots: one packed tensor with offsets
    assert b.host_offsets == (0, 40 * 56 * 3, 40 * 56 * 3 + 24 * 30 * 3) and b.host_pixels.dim() == 1
    assert np.array_equal(b.host_pixels[:6720].numpy().reshape(40, 56, 3), golden["y_40x56_progressive"])
    assert np.array_equal(b.host_pixels[6720:].numpy().reshape(24, 30, 3), golden["y_24x30_png"])
    # device files only, host files only, one image, one size
    only = jpeg.MixedJpegBatch.from_files(files(golden, NAMES[7:]))
    assert only.records.shape[0] == 0 and only.dev_geom.shape == (0, 8) and only.host_index.tolist() == [0, 1]
    one = jpeg.MixedJpegBatch.from_files([golden["s_37x53_420"]])
    assert one.n == 1 and one.uniform and one.totals[2] == 37 * 53 * 3
    same = jpeg.MixedJpegBatch.from_files([golden["s_120x160_420"], golden["s_120x160_420_rstrow"]])
    assert same.uniform and same.max_segments == 8
    with pytest.raises(ValueError, match="empty"):
        jpeg.MixedJpegBatch.from_files([])


def test_the_shrink_limit_fires_at_656_and_not_at_640(golden):
    from openibl_amd import jpeg
    from tests.helpers import jpeg_ref as ref
    tall = ref.pil_encode(ref.make_image(3, 656, 16, "smooth"), subsampling=2)
    assert jpeg.parse(tall).device and jpeg.parse(tall).height == 656
    ok = jpeg.MixedJpegBatch.from_files([golden["s_48x64_grey"], golden["s_640x16_420"]], target=(40, 72))
    assert ok.n == 2
    with pytest.raises(ValueError, match=r"image 1 is 656 x 16.*40 x 72.*limit of 16"):
        jpeg.MixedJpegBatch.from_files([golden["s_48x64_grey"], tall], target=(40, 72))
    items = [(torch.from_numpy(golden["s_48x64_grey"]), "a", 0), (torch.from_numpy(tall), "b", 1)]
    with pytest.raises(ValueError, match="image 1 is 656 x 16"):
        functools.partial(jpeg.collate_mixed, target=(40, 72))(items)
    assert jpeg.collate_mixed(items)[0].n == 2                      # without a target the device call raises instead
    assert jpeg.collate_mixed(items, target=(41, 72))[0].n == 2     # 656 = 16 * 41
    # the width counts as well, and a host-decoded file too
    with pytest.raises(ValueError, match="image 0 is 48 x 64"):
        jpeg.MixedJpegBatch.from_files([golden["s_48x64_grey"]], target=(40, 3))
    with pytest.raises(ValueError, match="image 1 is 24 x 30"):
        jpeg.MixedJpegBatch.from_files([golden["s_9x8_444"], golden["s_24x30_png"]], target=(1, 16))


def test_collate_mixed_handles_the_fields_like_collate(golden):
    from openibl_amd import jpeg
    items = [(torch.from_numpy(golden["s_" + n]), n, i, 0.5, 1.5) for i, n in enumerate(NAMES)]
    batch, fnames, pids, x, y = jpeg.collate_mixed(items)
    assert isinstance(batch, jpeg.MixedJpegBatch) and list(fnames) == list(NAMES) and pids.tolist() == list(range(9))
    assert x.shape == (9,) and y.shape == (9,)
    bare = jpeg.collate_mixed([torch.from_numpy(golden["s_" + n]) for n in NAMES[:3]])
    assert isinstance(bare, jpeg.MixedJpegBatch) and bare.n == 3
    # the uniform collate still refuses the mix, with the message users know
    with pytest.raises(ValueError, match="mixed stored sizes.*use a batch size of 1 or a loader that groups them"):
        jpeg.JpegBatch.from_files(files(golden, NAMES[:3]))
    with pytest.raises(ValueError, match="mixed stored sizes"):
        jpeg.collate(items[:2])


def test_pin_memory_and_to_round_trip(golden):
    from openibl_amd import jpeg
    b = jpeg.MixedJpegBatch.from_files(files(golden))
    c = b.to("cpu")
    assert c is not b and c.n == 9 and c.totals == b.totals and c.reasons == b.reasons and c.sizes is b.sizes
    for name in jpeg.MixedJpegBatch._TENSORS:
        assert torch.equal(getattr(c, name), getattr(b, name)), name
    assert c.host_offsets == b.host_offsets and c.max_segment_bytes == b.max_segment_bytes
    assert callable(b.pin_memory) and callable(b.cuda) and callable(b.is_pinned)
    if torch.cuda.is_available():
        p = b.pin_memory()
        assert p.is_pinned() and torch.equal(p.scan, b.scan) and torch.equal(p.geom, b.geom)
        empty = jpeg.MixedJpegBatch.from_files(files(golden, DEVICE)).pin_memory()      # no host pixels: nothing to pin
        assert empty.is_pinned()


# ---- 5. refusals of the Python layers -------------------------------------------------------------------------------
def test_a_cpu_batch_has_no_fallback_and_arguments_are_checked(golden):
    from openibl_amd import jpeg, ops
    from openibl_amd.lib import OpenIBLAmdError
    b = jpeg.MixedJpegBatch.from_files(files(golden))
    for call in (lambda: ops.decode_jpeg_mixed(b), lambda: ops.decode_resize_jpeg(b, (40, 72)),
                 lambda: ops.decode_jpeg_mixed(b, scan="chunked", chunk_bytes=16),
                 lambda: ops.resize_u8_mixed(torch.zeros(b.totals[2], dtype=torch.uint8), b.sizes, (40, 72)),
                 lambda: ops.decode_resize_jpeg(jpeg.JpegBatch.from_files([golden["s_9x8_444"]]), (16, 16))):
        with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="MixedJpegBatch"):
        ops.decode_jpeg_mixed(jpeg.JpegBatch.from_files([golden["s_9x8_444"]]))
    with pytest.raises(ValueError, match="MixedJpegBatch or a JpegBatch"):
        ops.decode_resize_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), (16, 16))
    with pytest.raises(ValueError, match="scan must be one of"):
        ops.decode_jpeg_mixed(b, scan="nope")
    with pytest.raises(ValueError, match="chunk_bytes"):
        ops.decode_jpeg_mixed(b, scan="chunked", chunk_bytes=3)
    # without a target at collation the call itself names the image beyond the shrink limit
    with pytest.raises(ValueError, match=r"image 6 is 640 x 16.*16 x 16.*limit of 16"):
        ops.decode_resize_jpeg(b, (16, 16))
    with pytest.raises(ValueError, match="image 6 is 640 x 16"):
        ops.resize_u8_mixed(torch.zeros(b.totals[2], dtype=torch.uint8), b.sizes, (16, 16))
    with pytest.raises(ValueError, match="size must be"):
        ops.decode_resize_jpeg(b, 40)
    with pytest.raises(ValueError, match="out must be"):
        ops.decode_resize_jpeg(b, (40, 72), out="half")
    with pytest.raises(ValueError, match="packed buffer has"):
        ops.resize_u8_mixed(torch.zeros(100, dtype=torch.uint8), b.sizes, (40, 72))
    with pytest.raises(ValueError, match="1-D uint8"):
        ops.resize_u8_mixed(torch.zeros((4, 8, 8, 3), dtype=torch.uint8), [(8, 8)] * 4, (40, 72))
    assert jpeg.STATUS_TEXT[jpeg.ST_BAD_GEOM] == "geometry table inconsistent" and jpeg.ST_BAD_GEOM == 5


def test_input_decode_of_a_mixed_batch_needs_a_fixed_resize(golden):
    """The refusals come before any library call: nothing is loaded, the batch stays on the host."""
    from openibl_amd import jpeg
    from openibl_amd.augment import Resize
    from openibl_amd.extract import apply_input_decode, input_resizer, is_mixed_batch
    b = jpeg.MixedJpegBatch.from_files(files(golden))
    assert is_mixed_batch(b) and not is_mixed_batch(jpeg.JpegBatch.from_files([golden["s_9x8_444"]]))
    pending = []
    with pytest.raises(ValueError, match="needs input_resize"):
        apply_input_decode(b, "cpu", pending)
    with pytest.raises(ValueError, match="needs input_resize"):
        apply_input_decode(b, "cpu", pending, resize=input_resizer(None))
    with pytest.raises(ValueError, match="keep_aspect"):
        apply_input_decode(b, "cpu", pending, resize=input_resizer(Resize(48, 64, keep_aspect=True, out="uint8")))
    assert pending == []
    with pytest.raises(ValueError, match="JpegBatch"):                  # the message of the uniform path stays
        apply_input_decode(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), "cpu", pending, resize=input_resizer((48, 64)))
