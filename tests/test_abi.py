"""The C-ABI shared library: it builds (hipcc cross-compiles for gfx950 without a GPU), loads, and
exports exactly the entry points include/openibl_amd.h declares.  No compute call is made here —
only argument validation, which returns before any HIP call."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_loads():
    from openibl_amd import build, lib
    path = build.build(verbose=False)
    assert path.exists()
    h = lib.load()
    assert h.oibl_abi_version() == lib.ABI_VERSION
    assert h.oibl_target_arch() == b"gfx950"
    assert h.oibl_elem_size(0) == 2 and h.oibl_elem_size(1) == 4 and h.oibl_elem_size(7) == 0


def test_every_declared_symbol_is_exported_and_bound():
    from openibl_amd import lib
    names = declared_functions()
    assert len(names) >= 25
    raw = ctypes.CDLL(str(lib.lib_path()))
    for n in names:
        assert hasattr(raw, n), f"{n} is declared in the header but not exported"
    assert sorted(lib.SIGNATURES) == names, "lib.SIGNATURES and the header disagree"


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TDB"})


def test_product_library_exports_the_header_and_nothing_else():
    """libopenibl_amd.so exports exactly the functions the header declares: no oibl_debug_* hook, no test
    entry, no mutable hook variable (they are compile-time constants in this build); the hooks live in
    libopenibl_amd_dbg.so, which exports the same public surface plus them."""
    from openibl_amd import lib
    names = declared_functions()
    prod = [n for n in _exported(lib.lib_path()) if n.startswith("oibl_")]
    assert prod == names, sorted(set(prod) ^ set(names))
    dbg = [n for n in _exported(lib.debug_lib_path()) if n.startswith("oibl_")]
    assert sorted(set(dbg) - set(names)) == sorted(lib._HOOKS), "debug library: unexpected extra exports"
    assert set(names) <= set(dbg)
    # no writable hook state in the product: the hook variables are g_* statics in the debug build only
    import subprocess
    syms = subprocess.run(["nm", str(lib.lib_path())], capture_output=True, text=True).stdout
    assert not [ln for ln in syms.splitlines() if " g_" in ln and ln.split()[-2] in "bBdD" and "g_zero_line" not in ln and "g_err" not in ln]


def test_header_is_plain_c(tmp_path):
    """The boundary is C: the header must compile as C with no HIP / C++ / torch includes."""
    import shutil
    import subprocess
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "t.c"
    src.write_text('#include "openibl_amd.h"\nint main(void) { return OIBL_OK; }\n')
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", str(HEADER.parent), "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)


def test_argument_validation_reports_errors():
    from openibl_amd import lib
    h = lib.load()
    rc = h.oibl_pca_forward(None, 1, 64, None, None, 128, 0, 1, None, None, 0, None)
    assert rc == -1 and b"null" in h.oibl_last_error()
    rc = h.oibl_conv3x3_nhwc(None, 1, 8, 8, 64, None, None, 64, 1, 0, 0, None, None)
    assert rc == -1
    rc = h.oibl_row_topk(None, None, 1, 1, 1, 10, 0, None, None, None)
    assert rc == -1
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "row_topk")
    assert h.oibl_vgg16_workspace_bytes(1, 8, 8, 0) == 0           # image too small
    assert h.oibl_vgg16_workspace_bytes(32, 480, 640, 0) >= 2 * 32 * 480 * 640 * 64


def test_workspace_queries_and_storage_types_host_side():
    """Host-only parts of the matching ABI: workspace sizes (pure arithmetic) and the validation of
    storage-type codes, which returns before any HIP call."""
    from openibl_amd import lib
    h = lib.load()
    BF16, F32 = 0, 1
    ST_F32, ST_F16, ST_BF16 = 0, 1, 2
    m, n, d, k = 8192, 81920, 4096, 10
    # the untyped entry points are the typed ones on float32 storage
    for prec in (BF16, F32):
        assert h.oibl_pairwise_workspace_bytes(m, n, d, prec) == \
            h.oibl_pairwise_st_workspace_bytes(m, n, d, prec, ST_F32, ST_F32)
        assert h.oibl_sqdist_topk_workspace_bytes(m, n, d, k, prec) == \
            h.oibl_sqdist_topk_st_workspace_bytes(m, n, d, k, prec, ST_F32, ST_F32)
    # bf16 mode: a bf16-stored operand is read in place (no operand copy), fp16 needs the bf16 copy
    w32 = h.oibl_pairwise_st_workspace_bytes(m, n, d, BF16, ST_F32, ST_F32)
    w16 = h.oibl_pairwise_st_workspace_bytes(m, n, d, BF16, ST_F16, ST_F16)
    wbf = h.oibl_pairwise_st_workspace_bytes(m, n, d, BF16, ST_BF16, ST_BF16)
    assert w32 == w16 and w32 - wbf >= (m + n) * d * 2 and wbf < 4 * (m + n) * 2
    # fp32 mode: 16-bit rows are widened into the workspace, float32 rows are read in place
    f32 = h.oibl_pairwise_st_workspace_bytes(m, n, d, F32, ST_F32, ST_F32)
    f16 = h.oibl_pairwise_st_workspace_bytes(m, n, d, F32, ST_F16, ST_BF16)
    assert f16 - f32 >= (m + n) * d * 4
    # the fused top-k never reserves the [m][n] matrix, the exact path is bounded by 1 GiB tiles
    assert h.oibl_sqdist_topk_st_workspace_bytes(m, n, d, k, BF16, ST_F32, ST_F32) < m * n * 4
    # unknown codes / empty problems
    assert h.oibl_pairwise_st_workspace_bytes(m, n, d, BF16, 3, ST_F32) == 0
    assert h.oibl_sqdist_topk_st_workspace_bytes(m, n, d, k, BF16, ST_F32, -1) == 0
    assert h.oibl_sqdist_topk_st_workspace_bytes(0, n, d, k, BF16, ST_F32, ST_F32) == 0
    buf = ctypes.create_string_buffer(64)      # never dereferenced: validation fails first
    ptr = ctypes.addressof(buf)
    rc = h.oibl_sqdist_topk_st(ptr, 5, 1, ptr, 0, 1, 64, 1, 0, BF16, 0, ptr, ptr, None, ptr, 0, None)
    assert rc == -1 and b"storage type" in h.oibl_last_error()
    rc = h.oibl_pairwise_sqdist_st(ptr, 0, 1, ptr, 9, 1, 64, BF16, ptr, 1, ptr, 0, None)
    assert rc == -1 and b"storage type" in h.oibl_last_error()
    rc = h.oibl_resize_bilinear_nchw(None, 1, 3, 8, 8, None, 4, 4, None)
    assert rc == -1 and b"null" in h.oibl_last_error()
    rc = h.oibl_resize_bilinear_nchw(ptr, 1, 3, 8, 8, ptr, 0, 4, None)
    assert rc == -1 and b"bad shape" in h.oibl_last_error()
    rc = h.oibl_sum_l2_normalize(ptr, 0, 4, 64, ptr, None)
    assert rc == -1 and b"bad shape" in h.oibl_last_error()
    rc = h.oibl_cast_f32_to_f16(None, None, 8, None)
    assert rc == -1


def test_product_has_no_cpu_fallback():
    """Forward on a CPU tensor fails loudly instead of silently computing somewhere else."""
    import torch
    import hubconf
    from openibl_amd.lib import OpenIBLAmdError
    m = hubconf.vgg16_netvlad().eval()
    with pytest.raises((OpenIBLAmdError, RuntimeError)):
        m(torch.zeros(1, 3, 32, 32))


def test_oracle_is_not_imported_by_the_product():
    import ast
    bad = []
    for pkg in ("openibl_amd", "ibl"):
        for f in (ROOT / pkg).rglob("*.py"):
            tree = ast.parse(f.read_text())
            for node in ast.walk(tree):
                mods = []
                if isinstance(node, ast.Import):
                    mods = [a.name for a in node.names]
                elif isinstance(node, ast.ImportFrom) and node.module:
                    mods = [node.module]
                if any(m == "oracle" or m.startswith("oracle.") for m in mods):
                    bad.append(str(f))
    hub = ast.parse((ROOT / "hubconf.py").read_text())
    assert not bad, bad


def test_every_entry_point_is_documented_for_binders():
    """INTEGRATION.md names every function include/openibl_amd.h declares."""
    import re
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    header = re.sub(r"/\*.*?\*/", "", (root / "include" / "openibl_amd.h").read_text(), flags=re.S)
    names = sorted(set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", header)))
    doc = (root / "INTEGRATION.md").read_text()
    assert len(names) >= 49
    assert not [n for n in names if n not in doc]


def test_backbone_workspace_queries_host_side():
    """oibl_vgg16_workspace_bytes / oibl_conv3x3_workspace_bytes are host arithmetic (tile counts, the f16mx
    split plan): every precision, batch sizes on both sides of every split decision, odd image sizes — no
    crash (round 4 shipped a division by zero here for one GPU call), monotone in the batch, and the f16mx
    plan splits exactly where the tiling leaves a nearly empty round."""
    from openibl_amd import lib
    h = lib.load()
    BF16, F32, X3, MX = 0, 1, 2, 3
    for prec in (BF16, F32, X3, MX):
        last = 0
        for n in (1, 2, 3, 5, 8, 16, 32, 33):
            b = h.oibl_vgg16_workspace_bytes(n, 480, 640, prec)
            assert b > n * 240 * 320 * 64 * (2 if prec == BF16 else 4), (prec, n, b)
            assert b >= last or prec == MX                       # (the f16mx plan's scratch is not monotone)
            last = b
            assert h.oibl_vgg16_u8_workspace_bytes(n, 480, 640, prec) == b + n * 3 * 480 * 640 * 4
        for (H, W) in ((16, 16), (17, 31), (224, 224), (352, 500), (479, 637), (960, 1280)):
            assert h.oibl_vgg16_workspace_bytes(1, H, W, prec) > 0
        assert h.oibl_vgg16_workspace_bytes(1, 15, 640, prec) == 0 and h.oibl_vgg16_workspace_bytes(0, 480, 640, prec) == 0
    ws = lambda n, hh, ww, ci, co, pool: h.oibl_conv3x3_workspace_bytes(n, hh, ww, ci, co, pool, MX)   # noqa: E731
    assert ws(32, 30, 40, 512, 512, 0) == 9 * (150 - 128) * 256 * 512 * 4       # conv5_x at batch 32: 44 tiles x 9 parts
    assert ws(32, 60, 80, 512, 512, 0) == 0 and ws(32, 120, 160, 256, 256, 0) == 0 and ws(32, 240, 320, 64, 128, 0) == 0
    assert ws(1, 30, 40, 512, 512, 0) == 9 * 1200 * 512 * 4                      # one image: the whole layer, 9 parts
    assert ws(1, 60, 80, 512, 512, 1) == 9 * 4800 * 512 * 4                      # pooled: split only as a whole
    assert ws(1, 120, 160, 128, 256, 0) == 3 * 19200 * 256 * 4
    assert ws(1, 240, 320, 64, 128, 0) == 0                                      # 150 short tiles: not worth it
    assert ws(1, 24, 32, 64, 64, 1) == 0 and ws(1, 24, 32, 96, 128, 0) == 0      # no ring tiling: no plan, no crash
    for prec in (BF16, F32, X3):
        assert h.oibl_conv3x3_workspace_bytes(1, 30, 40, 512, 512, 0, prec) > 0 # their own split-K (128-row tiles)
        assert h.oibl_conv3x3_workspace_bytes(32, 60, 80, 512, 512, 0, prec) == 0
    assert h.oibl_conv3x3_workspace_bytes(1, 30, 40, 512, 512, 0, 7) == 0


def test_hot_kernels_stay_inside_their_register_budgets():
    """The compiler's per-kernel report of the current build (hipcc -Rpass-analysis=kernel-resource-usage,
    kept by openibl_amd.build): the kernels of the default path do not spill — ring convolutions and
    distances (2 waves per SIMD: <= 256 VGPRs), the bf16 stems, every LDS-DMA instantiation of the
    generic core — and the bf16x3 stem fits 16 waves per workgroup (<= 128 VGPRs; the 12 bytes of
    scratch it has are two values parked across the whole kernel, outside its loops).  The
    register-staging variants behind the test hook (GLDS = false) index staged registers and do spill;
    they are not on any default path."""
    import re
    from openibl_amd import build
    usage = build.resource_usage()
    assert len(usage) > 100
    seen = set()
    for name, u in usage.items():
        scratch, vgprs = u.get("ScratchSize", 0), u.get("VGPRs", 0) + u.get("AGPRs", 0)
        if any(k in name for k in ("conv3x3_ring_kernel", "pairwise_ring_kernel", "vgg_stem_kernel",
                                   "conv3x3_halo_kernel", "conv3x3_halo4_kernel", "pairwise_f16r_kernel",
                                   "pca_small_kernel", "pca_stream_kernel")):
            assert scratch == 0 and vgprs <= 256, (name, u)
            seen.add(re.sub(r"I.*", "", name))
        elif "vgg_stem_x3_kernel" in name or "vgg_stem_mx_kernel" in name:
            # the 16-wave f16mx stem (stem_mx16.h): no scratch at all; bf16x3 (stem_x3.h): two values parked outside its loops
            assert u["VGPRs"] <= 128 and u.get("AGPRs", 0) == 0, (name, u)
            assert scratch == 0 if "vgg_stem_mx_kernel" in name else scratch <= 16, (name, u)
            seen.add("mxstem" if "vgg_stem_mx_kernel" in name else "x3stem")
        elif "conv3x3_igemm_kernel" in name:
            glds = re.search(r"ELb([01])ELb([01])ELb([01])EEE", name).group(2)
            if glds == "1":
                assert scratch == 0, (name, u)
        elif any(k in name for k in ("pairwise_kernel", "gemm_nt_kernel", "netvlad_assign_kernel", "pca_partial_kernel")):
            if re.search(r"ELb1EEE", name):
                assert scratch == 0, (name, u)
    assert {"x3stem", "mxstem"} <= seen and len(seen) >= 5


def test_hot_kernels_hold_exactly_their_matrix_instructions():
    """The TEXT of the hot kernels, from the gfx950 code objects of the current build (openibl_amd.build.kernel_text):
    a ring kernel holds one body per stagger group, and a body one copy of its K loop and one peeled pair of last
    K-tiles — 16 phases (20 with an odd number of K-tiles) of 8 (bf16), 12 (bf16x3) or 6 (f16mx) matrix instructions.
    More means the compiler has cloned the body: in round 4 three correlated branches on a diagnostic flag did, and
    the product step lost 4.5 % with the flag off.  The product library holds exactly the instantiations the dispatch
    can launch: a kernel more is an experiment that shipped."""
    import re
    from openibl_amd import build
    text = build.kernel_text()
    if not text:
        import pytest
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    per_phase = {0: 8, 1: 12, 3: 6}      # operand codes of ring_core.h: bf16, bf16x3, f16mx

    def family(stem):
        return {n: t for n, t in text.items() if re.search(stem + r"I", n) and not n.endswith(".kd")}

    # convolutions: wave rows {2, 4} x pooled or not x the three arithmetics (f16mx operands write f16mx lines), and
    # the odd K-tile count that only bf16 Cin = 64 has, on the 512 x 128 tile
    ring = {}
    for name, t in family("conv3x3_ring_kernel").items():
        m = re.search(r"conv3x3_ring_kernelILi(\d)ELb([01])ELb([01])ELi(\d)ELb([01])EEE", name)
        assert m, name
        wm, pool, odd, p, outmx = (int(g) for g in m.groups())
        ring[(wm, pool, odd, p, outmx)] = t
        assert t["mfma"] == per_phase[p] * (20 if odd else 16) * 2, (name, t)
        assert t["bytes"] < 64 * 1024, (name, t)          # the instruction cache two CUs share
    want = {(wm, pool, 0, p, int(p == 3)) for wm in (2, 4) for pool in (0, 1) for p in per_phase}
    want |= {(4, pool, 1, 0, 0) for pool in (0, 1)}
    assert set(ring) == want and len(family("conv3x3_ring_kernel")) == 14, sorted(ring)
    # distances: filter pass or full matrix x the three arithmetics, 16 phases per group body
    pair = {}
    for name, t in family("pairwise_ring_kernel").items():
        m = re.search(r"pairwise_ring_kernelILb([01])ELi(\d)EEE", name)
        assert m, name
        pair[(int(m.group(1)), int(m.group(2)))] = t
        assert t["mfma"] == per_phase[int(m.group(2))] * 32, (name, t)
    assert set(pair) == {(f, p) for f in (0, 1) for p in per_phase} and len(family("pairwise_ring_kernel")) == 6, sorted(pair)
    # the 4-wave halo kernel of the 128-output-channel layers: 18 K-tiles x 4 phases x 6, one body; the fp16 filter
    # pass of the f16r top-k: the bf16 ring loop (16 phases x 8) per stagger-group body
    halo4 = family("conv3x3_halo4_kernel")
    assert len(halo4) == 2 and all(t["mfma"] == 432 and t["bytes"] < 64 * 1024 for t in halo4.values()), halo4
    f16r = family("pairwise_f16r_kernel")
    assert len(f16r) == 2 and all(t["mfma"] == 256 for t in f16r.values()), f16r
    # the packed PCA stream: 32 tiles x 4 k-pairs per chunk, a generic and a last-chunk body
    pk = {n: t for n, t in text.items() if "pca_stream_kernel" in n and not n.endswith(".kd")}
    assert pk and all(t["mfma"] == 256 for t in pk.values()), pk
    # the 8-wave halo kernel: 18 K-tiles x 4 phases x 6 per stagger-group body, pooled or not
    halo = family("conv3x3_halo_kernel")
    assert len(halo) == 2 and all(t["mfma"] == 864 for t in halo.values()), halo
    stems = {n: t["mfma"] for n, t in text.items() if "vgg_stem" in n and not n.endswith(".kd")}
    assert sorted(set(stems.values())) == [126, 168, 234], stems


def test_mx_variant_hook_takes_only_the_routes_that_exist():
    """oibl_debug_set_mx_variant (debug library): 0 = default dispatch, 1 = ring kernels only, 3 = halo kernel
    wherever legal.  The codes of the removed experiments (late issue, timing loops, stamps, halo4 everywhere, the
    halo kernel's first waits) are refused with an error status and leave the selection as it was."""
    from openibl_amd import lib
    h = lib.debug_hooks()
    try:
        for v in (0, 1, 3):
            assert h.oibl_debug_set_mx_variant(v) == 0, v
        for v in (2, 4, 5, 6, 7, 8, 13, 19, -1):
            assert h.oibl_debug_set_mx_variant(v) == -1, v          # OIBL_E_INVALID
        assert b"mx_variant" in h.oibl_last_error()
    finally:
        h.oibl_debug_set_mx_variant(0)
        lib.use_product_library()
