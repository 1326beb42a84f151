"""The chunked route of the device JPEG decoder (csrc/jpeg_chunked.h, csrc/jpeg.hip), without a GPU: the
chunk state machine's shared text as a host program that emulates the workgroup, under the address and
undefined-behaviour sanitizers, against the serial route's jpeg_decode_segment on the same input; the C ABI's
validation; the route selection of the Python layer."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from conftest import load_golden

ROOT = Path(__file__).resolve().parent.parent
CASES = ("8x8_444", "16x16_420", "9x17_422", "17x31_420", "37x53_444", "37x53_422", "37x53_420", "48x64_420_q30",
         "48x64_420_q75", "48x64_420_q95", "48x64_420_rst1", "48x64_420_rst3", "48x64_420_rstrow", "48x64_422_opt",
         "37x53_grey", "48x64_444_flat", "48x64_444_noise", "40x104_444_rst65")
LONG = ("420_q75_smooth", "444_q95_noise", "422_opt", "grey", "420_rst2rows")


@pytest.fixture(scope="module")
def golden():
    return load_golden("jpeg_decode")


@pytest.fixture(scope="module")
def long_files():
    return load_golden("jpeg_chunked")


def many_files(golden):
    o = golden["many_offsets"]
    return [golden["many_bytes"][o[i]:o[i + 1]] for i in range(len(o) - 1)]


def test_fixture_holds_the_long_files(long_files):
    from openibl_amd import jpeg
    assert tuple(long_files["names"]) == LONG and str(long_files["pil_version"])
    assert (ROOT / "tests" / "golden" / "jpeg_chunked.npz").stat().st_size < 512 << 10
    for n in LONG:
        p = jpeg.parse(long_files["s_" + n])
        assert p.device and long_files["y_" + n].shape == (120, 160, 3), (n, p.reason)
    noise = jpeg.parse(long_files["s_444_q95_noise"])
    assert noise.scan.size > 40000 and noise.scan.tobytes().count(b"\xff\x00") > 50 and noise.segments.shape[0] == 1
    rst = jpeg.parse(long_files["s_420_rst2rows"])
    assert rst.segments.shape[0] == 4 and int((rst.segments[:, 1] - rst.segments[:, 0]).min()) > 500


# ---- 1. the harness -------------------------------------------------------------------------------------------------
class Decoded:
    """What the harness reports for one stream."""

    def __init__(self, status_serial, status_chunked, rows, coef_serial, coef_chunked):
        self.status_serial, self.status_chunked = status_serial, status_chunked
        self.rows = rows                       # per segment (serial status, chunked status, rounds, lanes, damaged)
        self.coef_serial, self.coef_chunked = coef_serial, coef_chunked


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/helpers/jpeg_chunked_harness.cpp + csrc/jpeg_chunked.h as a program of its own under
    -fsanitize=address,undefined; nothing is preloaded and no Python binding is involved."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert shutil.which(cxx) is not None or Path(cxx).exists(), "no host C++ compiler (g++ or the ROCm clang++)"
    exe = tmp_path_factory.mktemp("jpeg_chunked_harness") / "jpeg_chunked_harness"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "openibl_amd" / "csrc"),
                    str(ROOT / "tests" / "helpers" / "jpeg_chunked_harness.cpp"), "-o", str(exe)], check=True)

    def run(streams, chunk_bytes):
        """streams: files the parser sends to the device -> [Decoded] from the harness."""
        from openibl_amd import jpeg
        blob = [struct.pack("<i", len(streams))]
        for data in streams:
            p = jpeg.parse(data)
            assert p.device, p.reason
            blob += [struct.pack("<5i", p.height, p.width, p.scan.size, p.segments.shape[0], chunk_bytes),
                     p.record.tobytes(), p.segments.astype("<i4").tobytes(), p.scan.tobytes()]
        fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
        fin.write_bytes(b"".join(blob))
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True,
                           env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
        assert r.returncode == 0, r.stderr[-3000:]
        raw, at, out = fout.read_bytes(), 0, []
        for _ in streams:
            ss, sc, n, nseg = struct.unpack_from("<4i", raw, at)
            rows = np.frombuffer(raw, "<i4", 5 * nseg, at + 16).reshape(nseg, 5)
            at += 16 + 20 * nseg
            out.append(Decoded(ss, sc, rows, np.frombuffer(raw, "<i2", n, at), np.frombuffer(raw, "<i2", n, at + 2 * n)))
            at += 4 * n
        assert at == len(raw)
        return out
    return run


# ---- 2. good streams ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_bytes", [4, 7, 16, 64, 128, 4096])
def test_chunked_equals_serial_on_the_good_streams(golden, long_files, harness, chunk_bytes):
    names = list(CASES) + ["many%d" % i for i in range(70)] + list(LONG)
    streams = [golden["s_" + n] for n in CASES] + many_files(golden) + [long_files["s_" + n] for n in LONG]
    out = harness(streams, chunk_bytes)
    lanes = 0
    for name, got in zip(names, out):
        assert got.status_serial == 0 and got.status_chunked == 0, (name, got.rows)
        assert not got.rows[:, :2].any() and (got.rows[:, 4] == -1).all(), (name, got.rows)
        assert np.array_equal(got.coef_chunked, got.coef_serial), name
        assert (got.rows[:, 2] >= 1).all() and (got.rows[:, 2] <= got.rows[:, 3]).all(), (name, got.rows)
        lanes = max(lanes, int(got.rows[:, 3].max()))
    by_name = dict(zip(names, out))
    if chunk_bytes == 4096:          # the route of a single lane for every file of the older fixture
        assert all(int(g.rows[:, 3].max()) == 1 for n, g in by_name.items()
                   if n not in LONG and n != "48x64_444_noise")
        assert by_name["48x64_444_noise"].rows[0, 3] == 2
        assert by_name["444_q95_noise"].rows[0, 3] == 12
    if chunk_bytes == 16:            # the settle loop really iterates (a Python model of it takes 173 rounds here)
        assert by_name["48x64_444_noise"].rows[0, 2] >= 20, by_name["48x64_444_noise"].rows
        assert by_name["48x64_444_noise"].rows[0, 3] > 400
    if chunk_bytes == 4:             # more chunks than lanes: the last lane takes the remainder
        assert lanes == 1024 and by_name["444_q95_noise"].rows[0, 3] == 1024


# ---- 3. damaged streams ---------------------------------------------------------------------------------------------
def _front_of_the_damage(data, rows):
    """A mask over coef[3][Bh][Bw][64]: False for the blocks of every damaged segment from its damaged block on."""
    from openibl_amd import jpeg
    p = jpeg.parse(data)
    hdr = p.record[:64].view(np.int32)
    ncomp, hs, vs, dri = int(hdr[0]), int(hdr[1]), int(hdr[2]), int(hdr[12])
    H, W = p.height, p.width
    Bw, Bh = 2 * ((W + 15) // 16), 2 * ((H + 15) // 16)
    mcus_x, mcus_y = -(-W // (8 * hs)), -(-H // (8 * vs))
    total, luma = mcus_x * mcus_y, hs * vs
    bpm = luma + 2 if ncomp == 3 else 1
    mask = np.ones((3, Bh, Bw, 64), bool)
    for k, (_, _, _, _, damaged) in enumerate(rows):
        if damaged < 0:
            continue
        first = min(k * dri, total) if dri else 0
        n_mcu = min(dri, total - first) if dri else total
        for blk in range(int(damaged), n_mcu * bpm):
            m, c = first + blk // bpm, blk % bpm
            my, mx = divmod(m, mcus_x)
            if c < luma:
                mask[0, my * vs + c // hs, mx * hs + c % hs] = False
            else:
                mask[c - luma + 1, my, mx] = False
    return mask.reshape(-1)


@pytest.mark.parametrize("chunk_bytes", [4, 16, 64])
def test_chunked_reports_what_serial_reports_on_damaged_streams(golden, harness, chunk_bytes):
    """The two damaged fixture streams, every truncation length of a small stream and the 200 seeded single-byte
    corruptions of tests/test_jpeg_decode_cpu.py: the program ends clean under the sanitizers, every segment has the
    serial route's status, and the coefficients are the serial route's in front of the first damaged block."""
    from openibl_amd import jpeg
    small = golden["s_16x16_420"]
    b0 = jpeg.parse(small).scan_begin
    streams = [golden["s_truncated"], golden["s_xor"]] + [small[:n] for n in range(b0 + 1, small.size)]
    rng = np.random.RandomState(1234)
    for i in range(200):
        base = golden["s_" + ("48x64_420_rst3", "16x16_420", "48x64_444_noise", "40x104_444_rst65")[i % 4]]
        s0 = jpeg.parse(base).scan_begin
        hurt = base.copy()
        hurt[rng.randint(s0, base.size - 2)] ^= rng.randint(1, 256)
        streams.append(hurt)
    streams = [s for s in streams if jpeg.parse(s).device]
    assert len(streams) > 150 + small.size - b0 - 1
    damaged = differ_behind = 0
    for i, (data, got) in enumerate(zip(streams, harness(streams, chunk_bytes))):
        assert got.status_chunked == got.status_serial, (i, got.rows)
        assert np.array_equal(got.rows[:, 1], got.rows[:, 0]), (i, got.rows)
        assert ((got.rows[:, 4] >= 0) == (got.rows[:, 1] != 0)).all(), (i, got.rows)
        assert (got.rows[:, 2] <= got.rows[:, 3]).all()
        front = _front_of_the_damage(data, got.rows)
        assert np.array_equal(got.coef_chunked[front], got.coef_serial[front]), (i, got.rows)
        damaged += got.status_serial != 0
        differ_behind += not np.array_equal(got.coef_chunked, got.coef_serial)
        if not got.rows[:, 1].any():
            assert front.all() and np.array_equal(got.coef_chunked, got.coef_serial)
    assert damaged > small.size - b0 - 10
    print(f"chunk_bytes {chunk_bytes}: {damaged} damaged streams of {len(streams)}, {differ_behind} differ behind "
          f"the damage")


# ---- 4. the ABI -----------------------------------------------------------------------------------------------------
NEW = ("oibl_jpeg_decode_chunked_workspace_bytes", "oibl_jpeg_decode_chunked")


def test_abi_declared_exported_bound_documented():
    import ctypes
    from openibl_amd import lib
    header = (ROOT / "include" / "openibl_amd.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in NEW:
        assert name + "(" in header and name in lib.SIGNATURES and name in doc and hasattr(raw, name)


def test_abi_validation_launches_nothing():
    import ctypes
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(1024)           # never dereferenced: validation fails first
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    good = dict(scan=p, n=100, rec=p, seg=p, S=4, mx=1, N=4, H=48, W=64, cb=128, out=p, st=p, ws=p, wsb=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        return h.oibl_jpeg_decode_chunked(a["scan"], a["n"], a["rec"], a["seg"], a["S"], a["mx"], a["N"], a["H"],
                                          a["W"], a["cb"], a["out"], a["st"], a["ws"], a["wsb"], None)
    for key in ("scan", "rec", "seg", "out", "st"):
        assert call(**{key: None}) == -1 and b"null" in h.oibl_last_error(), key
    for cb in (3, 65537, 0, -128):
        assert call(cb=cb) == -1 and b"chunk_bytes" in h.oibl_last_error(), cb
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=7), dict(W=32769), dict(H=32769), dict(S=3)):
        assert call(**kw) == -1 and b"bad shape" in h.oibl_last_error(), kw
    assert call(n=0) == -1 and call(n=1 << 31) == -1 and b"scan_len" in h.oibl_last_error()
    assert call(mx=0) == -1 and call(mx=5) == -1 and b"max_segments" in h.oibl_last_error()
    assert call(rec=p + 2) == -1 and call(st=p + 1) == -1 and b"aligned" in h.oibl_last_error()
    assert call(ws=None) == -1 and call(ws=p + 64) == -1 and b"256" in h.oibl_last_error()
    need = h.oibl_jpeg_decode_chunked_workspace_bytes(4, 48, 64, 4, 128)
    rc = call(wsb=need - 1)
    assert rc != 0 and rc != -1 and b"workspace" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "jpeg_decode_chunked")


def test_abi_workspace_query():
    from openibl_amd import lib
    h = lib.load()
    q = h.oibl_jpeg_decode_chunked_workspace_bytes
    # coefficients (int16) and planes (uint8) of 3 MCU-padded components, the segments' statuses and rounds
    assert q(4, 48, 64, 4, 128) == 4 * 3 * 48 * 64 * 3 + 512
    assert q(1, 37, 53, 1, 4) == q(1, 37, 53, 1, 65536) == 3 * 48 * 64 * 3 + 512
    assert q(4, 48, 64, 4, 128) == h.oibl_jpeg_decode_workspace_bytes(4, 48, 64, 4) + 256
    for bad in ((0, 48, 64, 1, 128), (65536, 48, 64, 65536, 128), (1, 0, 64, 1, 128), (1, 48, 7, 1, 128),
                (1, 32769, 64, 1, 128), (1, 48, 32769, 1, 128), (2, 48, 64, 1, 128), (1, 48, 64, (1 << 28) + 1, 128),
                (1, 48, 64, 1, 3), (1, 48, 64, 1, 65537), (1, 48, 64, 1, 0)):
        assert q(*bad) == 0, bad


def test_python_rounds_view_lies_where_the_c_layout_puts_it():
    """`ops._jpeg_rounds` is Python's one copy of the workspace layout: the byte offset of its view, plus the rounds
    and the planes behind it, must be the size the C queries give — for the uniform sizes (a width and a height that
    are no multiples of 16, an S that is no multiple of 64) and for a mixed size list."""
    import ctypes
    import torch
    from openibl_amd import jpeg, lib, ops
    h = lib.load()
    a256 = lambda v: (v + 255) // 256 * 256        # noqa: E731

    def offset(need, coef_bytes, S):
        ws = torch.empty(need, dtype=torch.uint8)
        view = ops._jpeg_rounds(ws, coef_bytes, S)
        assert view.dtype == torch.int32 and view.shape == (S,)
        return view.data_ptr() - ws.data_ptr()

    for N, H, W, S in ((1, 8, 8, 1), (4, 48, 64, 4), (2, 37, 53, 65), (3, 120, 161, 100), (1, 17, 31, 257)):
        need = h.oibl_jpeg_decode_chunked_workspace_bytes(N, H, W, S, 64)
        blocks = N * 3 * jpeg.plane_blocks(H, W)
        assert need > 0 and jpeg.plane_blocks(H, W) == (-(-H // 16) * 2) * (-(-W // 16) * 2)
        assert offset(need, blocks * 128, S) + a256(4 * S) + a256(blocks * 64) == need, (N, H, W, S)
    sizes = [(37, 53), (120, 161), (8, 8), (48, 64)]
    _, totals = jpeg.mixed_layout(sizes)
    for S in (4, 70):
        need = h.oibl_jpeg_decode_mixed_workspace_bytes((ctypes.c_size_t * 6)(*totals), len(sizes), S)
        assert need > 0 and offset(need, totals[0], S) + a256(4 * S) + a256(totals[1]) == need, S


def test_the_new_kernel_does_not_spill():
    from openibl_amd import build
    usage = {k: v for k, v in build.resource_usage().items() if "jscan_" in k}
    assert len(usage) == 1 and "jscan_chunk_kernel" in next(iter(usage)), usage
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 0) + u.get("AGPRs", 0) <= 128, (name, u)
        assert u.get("LDS", 0) <= 32 << 10, (name, u)      # the lane tables and the four Huffman tables


# ---- 5. the Python layer --------------------------------------------------------------------------------------------
def test_max_segment_bytes(golden, long_files):
    from openibl_amd import jpeg
    free = long_files["s_444_q95_noise"]
    p = jpeg.parse(free)
    assert jpeg.JpegBatch.from_files([free]).max_segment_bytes == p.scan_end - p.scan_begin > 40000
    rst = long_files["s_420_rst2rows"]
    sizes = [int(e - b) for b, e in jpeg.parse(rst).segments]
    assert len(sizes) == 4 and jpeg.JpegBatch.from_files([rst]).max_segment_bytes == max(sizes) < sum(sizes)
    both = jpeg.JpegBatch.from_files([rst, free, rst])
    assert both.max_segment_bytes == p.scan_end - p.scan_begin and both.max_segments == 4
    assert both.to("cpu").max_segment_bytes == both.max_segment_bytes
    assert jpeg.JpegBatch.from_files([golden["s_8x8_444"]]).max_segment_bytes < 100
    # a trailing constructor argument with a default
    old = jpeg.JpegBatch(both.n, both.height, both.width, both.scan, both.records, both.segments, both.max_segments,
                         both.dev_index, both.host_index, both.host_pixels, both.reasons)
    assert old.max_segment_bytes == 0
    assert jpeg.CHUNK_BYTES >= 4 and jpeg.CHUNKED_MIN_BYTES >= jpeg.CHUNK_BYTES


def test_routes_are_checked_and_a_cpu_batch_has_no_fallback(golden):
    import torch
    from openibl_amd import jpeg, ops
    from openibl_amd.lib import OpenIBLAmdError
    batch = jpeg.JpegBatch.from_files([golden["s_8x8_444"]])
    with pytest.raises(ValueError, match="scan must be one of"):
        ops.decode_jpeg(batch, scan="nope")
    for cb in (3, 65537):
        with pytest.raises(ValueError, match="chunk_bytes"):
            ops.decode_jpeg(batch, scan="chunked", chunk_bytes=cb)
    for scan in ("auto", "serial", "chunked"):
        with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
            ops.decode_jpeg(batch, scan=scan)
    with pytest.raises(ValueError, match="JpegBatch"):
        ops.decode_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), scan="chunked")
    assert jpeg.scan_route(True) == "auto" and jpeg.scan_route("chunked") == "chunked"
    with pytest.raises(ValueError, match="input_decode"):
        jpeg.scan_route("nope")
