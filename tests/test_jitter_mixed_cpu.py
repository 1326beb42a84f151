"""The colour jitter on a packed batch of mixed sizes (csrc/augment_geom.h, oibl_color_jitter_u8_mixed,
ops.color_jitter_mixed), without a GPU: the C ABI and its validation, the geometry and the pixel text as a host program
under the address and undefined-behaviour sanitizers, and the refusals of the Python layer."""
import ctypes
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import color_jitter_ref as ref

ROOT = Path(__file__).resolve().parent.parent
NEW = ("oibl_color_jitter_u8_mixed_workspace_bytes", "oibl_color_jitter_u8_mixed")
B, C, S, H, X = ref.BRIGHTNESS, ref.CONTRAST, ref.SATURATION, ref.HUE, ref.SKIP
# H W 3 = 3 mod 4; one chunk of 4096 pixels; one chunk and a tail; 1 pixel; five parts; 1 mod 4; 2 mod 4
SIZES = ((37, 53), (64, 64), (64, 65), (1, 1), (120, 160), (5, 7), (3, 2), (8, 8), (48, 64))
ORDERS = ((C, B, S, H), (B, C, H, S), (H, S, C, B), (S, H, B, C), (B, S, H, X), (X, X, X, X), (H, C, X, B),
          (S, X, C, X), (C, H, S, B))


# ---- 1. the ABI -----------------------------------------------------------------------------------------------------
def test_abi_declared_exported_bound_documented():
    from openibl_amd import lib
    header = (ROOT / "include" / "openibl_amd.h").read_text()
    doc = (ROOT / "INTEGRATION.md").read_text()
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in NEW:
        assert name + "(" in header and name in lib.SIGNATURES and name in doc and hasattr(raw, name)


def _sizes(sizes):
    s = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    return s, s.ctypes.data_as(ctypes.c_void_p)


def test_workspace_query_is_the_largest_part_count_and_zero_for_what_the_call_rejects():
    from openibl_amd import lib
    h = lib.load()

    def query(sizes, n=None):
        s, p = _sizes(sizes)
        return h.oibl_color_jitter_u8_mixed_workspace_bytes(p, s.shape[0] if n is None else n)
    a256 = lambda v: (v + 255) // 256 * 256        # noqa: E731
    assert query([(5, 7)]) == 256                                             # one sum
    assert query([(480, 640)] * 12) == a256(12 * 75 * 8)                      # the uniform call's
    assert query([(480, 640)] * 12) == h.oibl_color_jitter_u8_workspace_bytes(12, 480, 640)
    assert query([(8, 8), (120, 160), (64, 65)]) == a256(3 * 5 * 8)           # rows of the largest part count
    assert query([(16384, 16384), (1, 1)]) == 2 * 1024 * 8                    # at most 1024 sums per image
    assert query([(1100, 4000)]) == a256(538 * 8)                             # chunks of 8192 pixels
    for bad in ([(0, 8)], [(8, 8), (8, 32769)], [(-1, 8)], [(16385, 16384)], [(32768, 32768)]):
        assert query(bad) == 0, bad
    assert query([(8, 8)], 0) == 0 and query([(8, 8)] * 2, -1) == 0 and query([(8, 8)], 65536) == 0
    assert h.oibl_color_jitter_u8_mixed_workspace_bytes(None, 1) == 0


def test_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(1024)           # never dereferenced: validation fails first
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    good = dict(x=p, nb=100000, geom=p, sizes=[(48, 64), (37, 53)], N=2, rec=p, out=p, ws=p, wsb=1 << 30)

    def call(**kw):
        a = dict(good, **kw)
        sp = None if a["sizes"] is None else _sizes(a["sizes"])[1]
        return h.oibl_color_jitter_u8_mixed(a["x"], a["nb"], a["geom"], sp, a["N"], a["rec"], a["out"], a["ws"],
                                            a["wsb"], None)
    for key in ("x", "geom", "sizes", "out"):
        assert call(**{key: None}) == -1 and b"null" in h.oibl_last_error(), key
    for n in (0, 65536, -2):
        assert call(N=n) == -1 and b"bad shape" in h.oibl_last_error() and b"N = " in h.oibl_last_error()
    assert call(nb=0) == -1 and call(nb=1 << 40) == -1 and b"packed_bytes" in h.oibl_last_error()
    # a violated limit names the image
    for sizes, words in (([(48, 64), (0, 16)], (b"image 1 is 0 x 16",)), ([(32769, 4), (8, 8)], (b"image 0 is 32769 x 4",)),
                         ([(8, 8), (-7, 8)], (b"image 1 is -7 x 8",)),
                         ([(8, 8), (16384, 16385)], (b"image 1 is 16384 x 16385", b"2^28"))):
        assert call(sizes=sizes) == -1
        assert b"bad shape" in h.oibl_last_error() and all(w in h.oibl_last_error() for w in words), sizes
    assert call(geom=p + 2) == -1 and call(rec=p + 1) == -1 and b"aligned" in h.oibl_last_error()
    # the workspace: short or misaligned is OIBL_E_WORKSPACE, and only a call with records needs one
    need = h.oibl_color_jitter_u8_mixed_workspace_bytes(_sizes(good["sizes"])[1], 2)
    assert need == 256
    for kw in (dict(wsb=need - 1), dict(ws=p + 64), dict(ws=None)):
        rc = call(**kw)
        assert rc != 0 and rc != -1 and b"workspace" in h.oibl_last_error(), kw
        with pytest.raises(lib.OpenIBLAmdError):
            lib.check(rc, "color_jitter_u8_mixed")
    # no records, in place: nothing to do, nothing launched (no device here to launch on)
    assert call(rec=None, ws=None, wsb=0) == 0


# ---- 2. the host program --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    """tests/helpers/jitter_mixed_harness.cpp + csrc/augment_geom.h + csrc/augment_pixel.h as a program of its own under
    -fsanitize=address,undefined; nothing is preloaded and no Python binding is involved."""
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert shutil.which(cxx) is not None or Path(cxx).exists(), "no host C++ compiler (g++ or the ROCm clang++)"
    exe = tmp_path_factory.mktemp("jitter_mixed_harness") / "jitter_mixed_harness"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    str(ROOT / "openibl_amd" / "csrc"), str(ROOT / "tests" / "helpers" / "jitter_mixed_harness.cpp"),
                    "-o", str(exe)], check=True)
    env = {"ASAN_OPTIONS": "detect_leaks=1", "PATH": "/usr/bin:/bin"}

    def sweep():
        r = subprocess.run([str(exe), "sweep"], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout.splitlines()

    def run(sizes, records, packed, overrides=()):
        """-> (ok [N], the packed buffer after both passes in place)."""
        sizes = np.asarray(sizes, "<i4").reshape(-1, 2)
        n = sizes.shape[0]
        rec = np.zeros((n, 8), "<i4") if records is None else np.asarray(records, "<i4").reshape(n, 8)
        blob = [struct.pack("<3i", n, len(overrides), records is not None), sizes.tobytes(), rec.tobytes(),
                np.asarray(packed, np.uint8).tobytes(), np.asarray(overrides, "<i4").reshape(-1, 3).tobytes()]
        fin, fout = exe.parent / "in.bin", exe.parent / "out.bin"
        fin.write_bytes(b"".join(blob))
        r = subprocess.run([str(exe), "run", str(fin), str(fout)], capture_output=True, text=True, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        raw = fout.read_bytes()
        nbytes, = struct.unpack_from("<q", raw, 0)
        assert nbytes == len(packed) and len(raw) == 8 + 4 * n + nbytes
        return np.frombuffer(raw, "<i4", n, 8), np.frombuffer(raw, np.uint8, nbytes, 8 + 4 * n)
    run.sweep = sweep
    return run


def test_parts_cover_every_pixel_once_and_agree_with_the_uniform_geometry(harness):
    lines = harness.sweep()
    assert lines[-1] == "ok"
    seen = {ln.split(":")[0]: ln for ln in lines[:-1]}
    # the sweep has the sizes it is there for
    assert "1 pixels, 1 parts of 4096" in seen["1 x 1"] and "% 4 = 3" in seen["37 x 53"]
    assert "4096 pixels, 1 parts of 4096" in seen["64 x 64"] and "2 parts of 4096" in seen["64 x 65"]
    assert "1024 parts of 4096" in seen["2048 x 2048"] and "513 parts of 8192" in seen["2048 x 2049"]
    assert "538 parts of 8192" in seen["1100 x 4000"]
    for big in ("16384 x 16384", "32768 x 8192", "8192 x 32768"):
        assert "268435456 pixels, 1024 parts of 262144" in seen[big]
    assert {ln.split("% 4 = ")[1] for ln in lines[:-1]} == {"0", "1", "2", "3"}


def packed_batch(sizes, seed=3, fill=0xA5):
    """(packed buffer with the padding filled with a pattern, offsets, the images) for random images of `sizes`."""
    from openibl_amd import jpeg
    rng = np.random.default_rng(seed)
    geom, totals = jpeg.mixed_layout(sizes)
    offs = jpeg.geom_pixel_offsets(geom)
    packed = np.full(totals[2], fill, np.uint8)
    imgs = []
    for (h, w), o in zip(sizes, offs.tolist()):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[: max(h // 4, 1)] //= 8
        imgs.append(img)
        packed[o:o + 3 * h * w] = img.reshape(-1)
    return packed, offs.tolist(), imgs


def fixed_records(n, seed=11):
    rng = np.random.default_rng(seed)
    orders = [ORDERS[i % len(ORDERS)] for i in range(n)]
    return ref.pack_records(orders, rng.uniform(0.3, 1.7, (n, 3)), [ref.hue_byte(v) for v in rng.uniform(-0.5, 0.5, n)])


def padding_mask(sizes, offs, nbytes):
    pad = np.ones(nbytes, bool)
    for (h, w), o in zip(sizes, offs):
        pad[o:o + 3 * h * w] = False
    return pad


def test_pixel_text_in_place_is_the_model_and_a_tail_never_leaves_its_image(harness):
    """The compiled pixel text (augment_pixel.h, contraction off) through both passes, in place, lane by lane: every
    image is the numpy model's (which test_color_jitter_cpu.py holds to PIL), in two batch orders, and the bytes
    between the images keep their pattern.  The buffer has exactly the layout's size under the address sanitizer."""
    rec = fixed_records(len(SIZES))
    want = {}
    for order in (list(range(len(SIZES))), list(reversed(range(len(SIZES))))):
        sizes = [SIZES[i] for i in order]
        packed, offs, imgs = packed_batch(sizes, seed=3)
        # the same image content wherever it stands: draw per size
        for k, i in enumerate(order):
            img = np.random.default_rng(100 + i).integers(0, 256, SIZES[i] + (3,), dtype=np.uint8)
            imgs[k] = img
            packed[offs[k]:offs[k] + img.size] = img.reshape(-1)
        ok, got = harness(sizes, rec[order], packed)
        assert ok.tolist() == [1] * len(sizes)
        pad = padding_mask(sizes, offs, packed.size)
        assert pad.sum() > 0 and (got[pad] == 0xA5).all()
        for k, i in enumerate(order):
            h, w = SIZES[i]
            mine = got[offs[k]:offs[k] + 3 * h * w].reshape(h, w, 3)
            if i not in want:
                want[i] = ref.model_jitter(imgs[k], *ref.unpack_record(rec[i]))
            assert np.array_equal(mine, want[i]), (order[:2], SIZES[i])
    assert any(o % 4 == 0 and (3 * h * w) % 4 for (h, w), o in zip(sizes, offs))       # images that end inside a dword
    # without records nothing changes
    packed, offs, _ = packed_batch(SIZES)
    ok, got = harness(SIZES, None, packed)
    assert ok.all() and np.array_equal(got, packed)


def test_inconsistent_rows_are_skipped_and_every_accepted_extent_is_inside(harness):
    """Rows of the geometry table overwritten behind the layout function.  A refused image keeps its bytes, every
    other image is what it is in the untouched batch; the program itself checks that an accepted row lies inside
    [0, packed_bytes) and inside the grid, and the buffer has exactly packed_bytes bytes."""
    sizes = list(SIZES)
    rec = fixed_records(len(sizes))
    packed, offs, _ = packed_batch(sizes)
    _, clean = harness(sizes, rec, packed)
    nbytes = packed.size
    Hh, Ww, LO, HI = 0, 1, 4, 5
    last = len(sizes) - 1
    cases = [(0, Hh, 0), (0, Hh, -5), (0, Hh, 32769), (0, Ww, -1), (0, Ww, 1 << 30),    # sides outside their range
             (4, LO, nbytes), (4, LO, nbytes - 3 * 120 * 160 + 1), (4, LO, -1),         # offsets beyond the buffer
             (4, HI, 1), (4, HI, -1), (4, HI, 256), (4, HI, 0x7FFFFFFF),                # high offset bits
             (last, Hh, 49), (3, Hh, 32768), (3, Ww, 32768),                            # an extent that passes the end
             (7, Hh, 641), (7, Ww, 4096),
             (0, Ww, 880)]       # 37 x 880 lies inside the buffer but has 8 parts where the grid has 5
    assert nbytes == 97920 and 37 * 880 * 3 <= nbytes and -(-37 * 880 // 4096) == 8
    for image, entry, value in cases:
        ok, got = harness(sizes, rec, packed, overrides=[(image, entry, value)])
        assert ok.tolist() == [int(i != image) for i in range(len(sizes))], (image, entry, value)
        h, w = sizes[image]
        mine = slice(offs[image], offs[image] + 3 * h * w)
        assert np.array_equal(got[mine], packed[mine]), (image, entry, value)          # nothing written
        rest = np.ones(nbytes, bool)
        rest[mine] = False
        assert np.array_equal(got[rest], clean[rest]), (image, entry, value)
    # a row that stays inside the buffer and the grid (a smaller image at the same place) is accepted: bounded
    ok, got = harness(sizes, rec, packed, overrides=[(4, Hh, 100)])
    assert ok.all()
    tail = slice(offs[4] + 3 * 100 * 160, offs[4] + 3 * 120 * 160)
    assert np.array_equal(got[tail], packed[tail])
    # every row wrong at once
    ok, got = harness(sizes, rec, packed, overrides=[(i, HI, 255) for i in range(len(sizes))])
    assert not ok.any() and np.array_equal(got, packed)


def test_the_new_kernels_do_not_spill_and_the_uniform_ones_kept_their_budget():
    from openibl_amd import build
    usage = build.resource_usage()
    mixed = {k: v for k, v in usage.items() if "jitter_mixed_" in k}
    uniform = {k: v for k, v in usage.items() if "jitter_partial_kernel" in k or "jitter_apply_kernel" in k}
    assert len(mixed) == 2 and len(uniform) == 3, (sorted(mixed), sorted(uniform))
    for name, u in {**mixed, **uniform}.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 0) + u.get("AGPRs", 0) <= 64 and u["LDS"] == 32, (name, u)


# ---- 3. refusals of the Python layer --------------------------------------------------------------------------------
def test_ops_color_jitter_mixed_checks_its_arguments_and_has_no_cpu_fallback():
    from openibl_amd import jpeg, ops
    from openibl_amd.lib import OpenIBLAmdError
    sizes = [(37, 53), (8, 8)]
    _, totals = jpeg.mixed_layout(sizes)
    packed = torch.zeros(totals[2], dtype=torch.uint8)
    rec = torch.zeros((2, 8), dtype=torch.int32)
    for params in (None, rec):
        for out in (None, packed):
            with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
                ops.color_jitter_mixed(packed, sizes, params, out=out)
    for bad, sz, params, out, match in (
            (packed.float(), sizes, rec, None, "1-D uint8"), (packed.view(-1, 1), sizes, rec, None, "1-D uint8"),
            (packed[:100], sizes, rec, None, "packed buffer has 100 bytes"), (packed, [], rec, None, "empty"),
            (packed, [(0, 4), (8, 8)], rec, None, "image 0 is 0 x 4"),
            (packed, [(8, 8), (16384, 16385)], rec, None, "image 1 is 16384 x 16385: more than 2\\^28"),
            (packed, sizes, rec.float(), None, "int32"), (packed, sizes, rec[:1], None, "params must be"),
            (packed, sizes, torch.zeros((8, 2), dtype=torch.int32).t(), None, "contiguous"),
            (packed, sizes, rec, packed[:-1], "out must be"), (packed, sizes, rec, packed.float(), "out must be")):
        with pytest.raises(ValueError, match=match):
            ops.color_jitter_mixed(bad, sz, params, out=out)
