"""The specification of the device JPEG decoder, without a GPU: the numpy model (tests/helpers/jpeg_ref.py — the
arithmetic csrc/jpeg_entropy.h and csrc/jpeg.hip repeat) against the fixture tests/golden/jpeg_decode.npz, which
holds Pillow's own outputs, and against the installed Pillow; the routing of `jpeg.parse` / `jpeg.probe`; the C ABI's
validation; the entropy decoder's shared text as a host program under the address and undefined-behaviour sanitizers;
the refusals of the Python layers."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden
from helpers import jpeg_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CASES = ("8x8_444", "16x16_420", "9x17_422", "17x31_420", "37x53_444", "37x53_422", "37x53_420", "48x64_420_q30",
         "48x64_420_q75", "48x64_420_q95", "48x64_420_rst1", "48x64_420_rst3", "48x64_420_rstrow", "48x64_422_opt",
         "37x53_grey", "48x64_444_flat", "48x64_444_noise", "40x104_444_rst65")
FALLBACKS = {"progressive": "progressive", "cmyk": "4 components", "png": "not a JPEG", "9x4_420": "narrower"}


@pytest.fixture(scope="module")
def golden():
    return load_golden("jpeg_decode")


def many_files(golden):
    o = golden["many_offsets"]
    return [golden["many_bytes"][o[i]:o[i + 1]] for i in range(len(o) - 1)]


def test_fixture_holds_the_cases(golden):
    assert tuple(golden["names"]) == CASES and str(golden["pil_version"])
    assert tuple(golden["fallbacks"]) == tuple(FALLBACKS) and tuple(golden["damaged"]) == ("truncated", "xor")
    assert len(many_files(golden)) == 70 and golden["many_y"].shape == (70, 16, 16, 3)
    assert all(golden["y_" + n].shape == (48, 64, 3) for n in golden["mixed4"]) and len(golden["mixed4"]) == 4
    assert (ROOT / "tests" / "golden" / "jpeg_decode.npz").stat().st_size < 1 << 20
    # stuffed FFs, ZRL-capable noise and a flat image are really there
    assert b"\xff\x00" in golden["s_48x64_444_noise"].tobytes()
    assert len(np.unique(golden["y_48x64_444_flat"].reshape(-1, 3), axis=0)) == 1


# ---- 1. the model is Pillow ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_model_equals_the_fixture(golden, name):
    got = ref.decode(golden["s_" + name])
    assert got.status == 0 and np.array_equal(got.rgb, golden["y_" + name])


def test_model_equals_the_fixture_on_the_many(golden):
    for i, f in enumerate(many_files(golden)):
        got = ref.decode(f)
        assert got.status == 0 and np.array_equal(got.rgb, golden["many_y"][i]), i


def test_model_reports_the_damage(golden):
    assert ref.decode(golden["s_truncated"]).status == ref.OUT_OF_BYTES
    assert ref.decode(golden["s_xor"]).status != 0


SWEEP = [(h, w, ss, q, kind, kw)
         for (h, w) in ((1, 8), (8, 8), (5, 13), (16, 16), (17, 9), (31, 17), (40, 33), (53, 37), (64, 48), (96, 128))
         for ss in (0, 1, 2) for q in (30, 75, 95) for kind in ("smooth", "noise")
         for kw in ({}, {"restart_marker_blocks": 3}, {"optimize": True})]


def test_model_equals_the_installed_pil_on_a_fresh_sweep():
    pytest.importorskip("PIL")
    bad = []
    for h, w, ss, q, kind, kw in SWEEP:        # widths >= 8 only; every case is judged
        data = ref.pil_encode(ref.make_image(h + w + q, h, w, kind), quality=q, subsampling=ss, **kw)
        got = ref.decode(data)
        if got.status or not np.array_equal(got.rgb, ref.pil_decode(data)):
            bad.append((h, w, ss, q, kind, kw, got.status))
    for h, w in ((37, 53), (8, 8), (1, 9)):
        data = ref.pil_encode(ref.make_image(h, h, w), mode="L", quality=75)
        got = ref.decode(data)
        if got.status or not np.array_equal(got.rgb, ref.pil_decode(data)):
            bad.append((h, w, "grey", got.status))
    assert not bad, bad


# ---- 2. parse and probe -------------------------------------------------------------------------------------------
def test_parse_sends_every_device_case_to_the_device(golden):
    from openibl_amd import jpeg
    for name in CASES:
        data = golden["s_" + name]
        p = jpeg.parse(data)
        assert p.device and jpeg.probe(data) == (True, ""), (name, p.reason)
        assert (p.height, p.width, 3) == golden["y_" + name].shape
        hdr = p.record[:64].view(np.int32)
        assert hdr[14] == p.segments.shape[0] and hdr[15] == 0 and p.record.shape == (jpeg.REC_BYTES,)
        # the segments tile the scan, a restart marker between each two
        assert p.segments[0, 0] == 0 and p.segments[-1, 1] == p.scan_end - p.scan_begin
        assert (p.segments[1:, 0] == p.segments[:-1, 1] + 2).all()
    assert jpeg.parse(golden["s_48x64_420_rst1"]).segments.shape[0] == 12
    assert jpeg.parse(golden["s_48x64_420_rst3"]).segments.shape[0] == 4
    assert jpeg.parse(golden["s_48x64_420_rstrow"]).segments.shape[0] == 3
    assert jpeg.parse(golden["s_40x104_444_rst65"]).segments.shape[0] == 65
    for f in many_files(golden):
        assert jpeg.parse(f).device


def test_parse_sends_every_fallback_file_to_the_host_with_the_reason(golden):
    from openibl_amd import jpeg
    for name, why in FALLBACKS.items():
        ok, reason = jpeg.probe(golden["f_" + name])
        assert not ok and why in reason, (name, reason)
    assert jpeg.probe(b"")[0] is False and jpeg.probe(b"\xff\xd8\xff")[0] is False


def test_parse_marks_missing_restart_markers(golden):
    from openibl_amd import jpeg
    data = golden["s_48x64_420_rst1"].copy()
    p = jpeg.parse(data)
    cut = data[:p.scan_begin + int(p.segments[5, 1])]          # the file ends in front of the sixth marker
    q = jpeg.parse(cut)
    assert q.device and q.record[:64].view(np.int32)[15] == jpeg.ST_BAD_RESTART and q.segments.shape[0] == 6
    data[p.scan_begin + int(p.segments[2, 1]) + 1] = 0xD7       # a marker out of sequence
    assert jpeg.parse(data).record[:64].view(np.int32)[15] == jpeg.ST_BAD_RESTART


# ---- 3. the ABI ---------------------------------------------------------------------------------------------------
def test_abi_declared_exported_bound_documented():
    import ctypes
    from openibl_amd import lib
    header = (ROOT / "include" / "openibl_amd.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ("oibl_jpeg_decode_workspace_bytes", "oibl_jpeg_decode"):
        assert name + "(" in header and name in lib.SIGNATURES and name in doc and hasattr(raw, name)


def test_abi_validation_launches_nothing():
    import ctypes
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(1024)           # never dereferenced: validation fails first
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    good = dict(scan=p, n=100, rec=p, seg=p, S=4, mx=1, N=4, H=48, W=64, out=p, st=p, ws=p, wsb=1 << 40)

    def call(**kw):
        a = dict(good, **kw)
        return h.oibl_jpeg_decode(a["scan"], a["n"], a["rec"], a["seg"], a["S"], a["mx"], a["N"], a["H"], a["W"],
                                  a["out"], a["st"], a["ws"], a["wsb"], None)
    for key in ("scan", "rec", "seg", "out", "st"):
        assert call(**{key: None}) == -1 and b"null" in h.oibl_last_error(), key
    for kw in (dict(N=0), dict(N=65536), dict(H=0), dict(W=7), dict(W=32769), dict(H=32769), dict(S=3)):
        assert call(**kw) == -1 and b"bad shape" in h.oibl_last_error(), kw
    assert call(n=0) == -1 and call(n=1 << 31) == -1 and b"scan_len" in h.oibl_last_error()
    assert call(mx=0) == -1 and call(mx=5) == -1 and b"max_segments" in h.oibl_last_error()
    assert call(rec=p + 2) == -1 and call(st=p + 1) == -1 and b"aligned" in h.oibl_last_error()
    assert call(ws=None) == -1 and call(ws=p + 64) == -1 and b"256" in h.oibl_last_error()
    need = h.oibl_jpeg_decode_workspace_bytes(4, 48, 64, 4)
    rc = call(wsb=need - 1)
    assert rc != 0 and rc != -1 and b"workspace" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "jpeg_decode")


def test_abi_workspace_query():
    from openibl_amd import lib
    h = lib.load()
    q = h.oibl_jpeg_decode_workspace_bytes
    # coefficients (int16) and planes (uint8) of 3 MCU-padded components, the segment status
    assert q(4, 48, 64, 4) == 4 * 3 * 48 * 64 * 3 + 256
    assert q(1, 37, 53, 1) == 3 * 48 * 64 * 3 + 256
    assert q(1024, 480, 640, 1024 * 30) >= 1024 * 480 * 640 * 9
    for bad in ((0, 48, 64, 1), (65536, 48, 64, 65536), (1, 0, 64, 1), (1, 48, 7, 1), (1, 32769, 64, 1),
                (1, 48, 32769, 1), (2, 48, 64, 1), (1, 48, 64, (1 << 28) + 1)):
        assert q(*bad) == 0, bad


def test_the_three_kernels_do_not_spill():
    from openibl_amd import build
    usage = {k: v for k, v in build.resource_usage().items() if "jpeg_" in k}
    assert sorted(n.split("jpeg_")[1].split("_kernel")[0] for n in usage) == ["colour", "entropy", "idct"], usage
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 0) + u.get("AGPRs", 0) <= 128, (name, u)


# ---- 4. the host harness ------------------------------------------------------------------------------------------
def _model_coefs(data, H, W):
    """The model's coefficients in the kernel's layout coef[3][Bh][Bw][64]."""
    got = ref.decode(data)
    Bw, Bh = 2 * ((W + 15) // 16), 2 * ((H + 15) // 16)
    out = np.zeros((3, Bh, Bw, 64), np.int16)
    for c, blocks in enumerate(got.coefs):
        out[c, :blocks.shape[0], :blocks.shape[1]] = blocks
    return got.status, out.reshape(-1)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/helpers/jpeg_entropy_harness.cpp + csrc/jpeg_entropy.h as a program of its own under
    -fsanitize=address,undefined; nothing is preloaded and no Python binding is involved."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert shutil.which(cxx) is not None or Path(cxx).exists(), "no host C++ compiler (g++ or the ROCm clang++)"
    exe = tmp_path_factory.mktemp("jpeg_harness") / "jpeg_entropy_harness"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", str(ROOT / "openibl_amd" / "csrc"),
                    str(ROOT / "tests" / "helpers" / "jpeg_entropy_harness.cpp"), "-o", str(exe)], check=True)

    def run(streams):
        """streams: files the parser sends to the device -> [(status, coef)] from the harness."""
        from openibl_amd import jpeg
        blob = [struct.pack("<i", len(streams))]
        for data in streams:
            dri = None
            if isinstance(data, tuple):            # (file, a restart interval to write into its record)
                data, dri = data
            p = jpeg.parse(data)
            assert p.device, p.reason
            if dri is not None:
                p.record[:64].view(np.int32)[12] = dri
            blob += [struct.pack("<4i", p.height, p.width, p.scan.size, p.segments.shape[0]), p.record.tobytes(),
                     p.segments.astype("<i4").tobytes(), p.scan.tobytes()]
        fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
        fin.write_bytes(b"".join(blob))
        r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True,
                           env={"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"})
        assert r.returncode == 0, r.stderr[-3000:]
        raw, at, out = fout.read_bytes(), 0, []
        for _ in streams:
            status, n = struct.unpack_from("<2i", raw, at)
            out.append((status, np.frombuffer(raw, "<i2", n, at + 8)))
            at += 8 + 2 * n
        assert at == len(raw)
        return out
    return run


def test_harness_equals_the_model_on_the_good_streams(golden, harness):
    streams = [golden["s_" + n] for n in CASES] + many_files(golden)
    for data, (status, coef) in zip(streams, harness(streams)):
        from openibl_amd import jpeg
        p = jpeg.parse(data)
        want_status, want = _model_coefs(data, p.height, p.width)
        assert status == 0 and want_status == 0 and np.array_equal(coef, want)


def _device_streams(candidates):
    from openibl_amd import jpeg
    return [c for c in candidates if jpeg.parse(c).device]


def test_harness_runs_clean_on_damaged_streams(golden, harness):
    """The two damaged fixture streams, every truncation length of a small stream and 200 seeded single-byte
    corruptions of streams with and without restarts: the program ends clean under the sanitizers and reports damage
    wherever the model does.  (A corruption that makes the parser send the file to the host is not a device case.)"""
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
    streams = _device_streams(streams)
    assert len(streams) > 150 + small.size - b0 - 1
    damaged = 0
    for data, (status, _) in zip(streams, harness(streams)):
        if ref.decode(data).status:
            damaged += 1
            assert status != 0
    assert damaged > small.size - b0 - 10       # truncations are damage; so are most corruptions


def test_harness_survives_damaged_tables_and_records(golden, harness):
    """Corruptions in front of the scan — Huffman counts and values, quantisation tables, the restart interval — that
    the parser still sends to the device: no out-of-range access, whatever the status."""
    from openibl_amd import jpeg
    rng = np.random.RandomState(99)
    streams = []
    for i in range(200):
        base = golden["s_" + ("48x64_422_opt", "48x64_420_rst1", "37x53_grey")[i % 3]]
        hurt = base.copy()
        hurt[rng.randint(2, jpeg.parse(base).scan_begin)] ^= rng.randint(1, 256)
        streams.append(hurt)
    streams = _device_streams(streams)
    assert len(streams) > 50
    harness(streams)
    # restart intervals the C ABI can be handed but no file can hold: no signed overflow in the MCU range
    out = harness([(golden["s_48x64_420_rst3"], d) for d in (0x7FFFFFFF, 0x7FFFFFF0, 1 << 30, 65536, -5)] +
                  [(golden["s_16x16_420"], 0x7FFFFFFF)])
    assert out[-1][0] == 0                       # one segment, one MCU: any interval of at least 1 decodes it


def test_parse_routes_a_huffman_table_of_an_unknown_class_to_the_host(golden):
    from openibl_amd import jpeg
    data = golden["s_48x64_422_opt"].copy()
    at = data.tobytes().index(b"\xff\xc4")
    for tc in (2, 7, 15):
        hurt = data.copy()
        hurt[at + 4] = (tc << 4) | (hurt[at + 4] & 15)
        ok, reason = jpeg.probe(hurt)
        assert not ok and "Huffman" in reason


# ---- 5. refusals of the Python layers -----------------------------------------------------------------------------
def test_a_cpu_batch_has_no_fallback(golden):
    from openibl_amd import jpeg, ops
    from openibl_amd.lib import OpenIBLAmdError
    batch = jpeg.JpegBatch.from_files([golden["s_8x8_444"]])
    assert batch.shape == (1, 8, 8, 3) and not batch.is_cuda and len(batch) == 1
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ops.decode_jpeg(batch)
    with pytest.raises(ValueError, match="JpegBatch"):
        ops.decode_jpeg(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))


def test_mixed_sizes_are_refused_and_a_batch_of_one_is_fine(golden):
    from openibl_amd import jpeg
    with pytest.raises(ValueError, match="mixed stored sizes"):
        jpeg.JpegBatch.from_files([golden["s_8x8_444"], golden["s_16x16_420"]])
    with pytest.raises(ValueError, match="mixed stored sizes"):
        jpeg.collate([(torch.from_numpy(golden["s_8x8_444"]), "a", 0), (torch.from_numpy(golden["s_37x53_grey"]), "b", 1)])
    for name in CASES:
        assert jpeg.JpegBatch.from_files([golden["s_" + name]]).n == 1


def test_collate_packs_the_batch(golden):
    from openibl_amd import jpeg
    pytest.importorskip("PIL")
    names = list(golden["mixed4"])
    items = [(torch.from_numpy(golden["s_" + n]), n, i, 0.5, 1.5) for i, n in enumerate(names)]
    png = np.asarray(golden["fy_png"])
    batch, fnames, pids, _, _ = jpeg.collate(items)
    assert list(fnames) == names and pids.tolist() == [0, 1, 2, 3]
    assert batch.n == 4 and batch.records.shape == (4, jpeg.REC_BYTES) and batch.host_pixels.shape[0] == 0
    assert batch.segments.shape == (1 + 1 + 4 + 1, 2) and batch.max_segments == 4
    hdr = batch.records[:, :64].numpy().view(np.int32)
    assert hdr[:, 13].tolist() == [0, 1, 2, 6] and hdr[:, 14].tolist() == [1, 1, 4, 1]
    # segments are offsets into the packed scan: the first byte of each image's scan is where its file has it
    for i, n in enumerate(names):
        p = jpeg.parse(golden["s_" + n])
        at = int(batch.segments[hdr[i, 13], 0])
        assert np.array_equal(batch.scan[at:at + 16].numpy(), p.scan[:16])
    # a file the device does not take travels as pixels
    mixed = jpeg.JpegBatch.from_files([golden["s_37x53_444"], golden["f_png"], golden["f_progressive"]])
    assert mixed.dev_index.tolist() == [0] and mixed.host_index.tolist() == [1, 2]
    assert np.array_equal(mixed.host_pixels[0].numpy(), png) and mixed.reasons[1] == "not a JPEG file"
    assert mixed.pin_memory is not None and mixed.to("cpu").n == 3


def test_raw_preprocessor_hands_over_the_files_bytes(golden, tmp_path):
    from ibl.utils.data.preprocessor import Preprocessor
    (tmp_path / "a.jpg").write_bytes(golden["s_37x53_420"].tobytes())
    item = Preprocessor([("a.jpg", 7, 1.0, 2.0)], root=str(tmp_path), raw=True)[0]
    assert item[0].dtype == torch.uint8 and item[0].dim() == 1 and item[1:] == ("a.jpg", 7, 1.0, 2.0)
    assert np.array_equal(item[0].numpy(), golden["s_37x53_420"])
    with pytest.raises(ValueError, match="raw"):
        Preprocessor([("a.jpg", 7, 1.0, 2.0)], root=str(tmp_path), transform=lambda x: x, raw=True)


def test_input_decode_with_a_tensor_batch_is_refused():
    from openibl_amd.extract import apply_input_decode
    with pytest.raises(ValueError, match="JpegBatch"):
        apply_input_decode(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), "cpu", [])
