"""The SFRS region head at the C boundary, without a GPU: the header declares its three entry points, the built
product library exports them, their argument validation returns before any HIP call, and the compiler's report of the
current build shows the new kernels without scratch, inside the register budget and on the matrix cores."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"
ENTRIES = ("oibl_region_workspace_bytes", "oibl_region_vlad_forward", "oibl_region_scores")
KERNELS = ("region_aggregate_kernel", "region_rowstats_kernel", "region_apply_kernel", "region_score_kernel")


def test_header_declares_and_library_exports_the_region_entries():
    from openibl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported by the product library"
        assert name in lib.SIGNATURES
        assert name in (ROOT / "INTEGRATION.md").read_text()


def test_region_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    K, C = 64, 512
    # parts [N][4][slabs][K][C] + stats: 30 x 40 -> quarters of 300 pixels -> 5 slabs of 60
    assert h.oibl_region_workspace_bytes(12, 30, 40, K, C) >= 12 * 4 * 5 * K * C * 4 + 12 * 9 * K * 4
    assert h.oibl_region_workspace_bytes(1, 4, 6, K, C) >= 4 * K * C * 4
    assert h.oibl_region_workspace_bytes(12, 31, 40, K, C) == 0 and h.oibl_region_workspace_bytes(12, 30, 39, K, C) == 0
    assert h.oibl_region_workspace_bytes(0, 30, 40, K, C) == 0
    # the decomposition does not depend on the batch: the workspace is linear in N
    assert h.oibl_region_workspace_bytes(48, 30, 40, K, C) == 4 * h.oibl_region_workspace_bytes(12, 30, 40, K, C)
    buf = ctypes.create_string_buffer(4096 + 256)       # never dereferenced: validation fails first
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    F32, BF16 = 1, 0
    rc = h.oibl_region_vlad_forward(None, 1, 4, 6, K, C, F32, ptr, ptr, 1, ptr, ptr, 0, None)
    assert rc == -1 and b"null" in h.oibl_last_error()
    rc = h.oibl_region_vlad_forward(ptr, 1, 5, 6, K, C, F32, ptr, ptr, 1, ptr, ptr, 1 << 30, None)
    assert rc == -1 and b"5 x 6" in h.oibl_last_error()
    rc = h.oibl_region_vlad_forward(ptr, 1, 4, 7, K, C, F32, ptr, ptr, 1, ptr, ptr, 1 << 30, None)
    assert rc == -1 and b"4 x 7" in h.oibl_last_error()
    rc = h.oibl_region_vlad_forward(ptr, 1, 4, 6, K, C, BF16, ptr, ptr, 1, ptr, ptr, 1 << 30, None)
    assert rc == -1 and b"fp32" in h.oibl_last_error()
    rc = h.oibl_region_vlad_forward(ptr, 1, 4, 6, 32, C, F32, ptr, ptr, 1, ptr, ptr, 1 << 30, None)
    assert rc == -1 and b"num_clusters" in h.oibl_last_error()
    rc = h.oibl_region_vlad_forward(ptr, 1, 4, 6, K, C, F32, ptr, ptr, 1, ptr, ptr, 1024, None)
    assert rc == -2 and b"workspace" in h.oibl_last_error()
    rc = h.oibl_region_scores(ptr, 1, 1, 32768, ptr, None)
    assert rc == -1 and b"at least one pair" in h.oibl_last_error()
    rc = h.oibl_region_scores(None, 1, 2, 32768, ptr, None)
    assert rc == -1 and b"null" in h.oibl_last_error()
    rc = h.oibl_region_scores(ptr, 0, 2, 32768, ptr, None)
    assert rc == -1
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "region_scores")


def test_region_kernels_do_not_spill_and_fit_the_register_file():
    """hipcc's per-kernel report of the current build: no scratch, at most 256 VGPRs.  The aggregation kernel
    runs one wave per SIMD like netvlad_fused_kernel, whose scheme it is, and like it also uses accumulation
    registers beside its 256 VGPRs (the compiler reports them apart: VGPRs 256 + AGPRs ~165 of the 512-entry file
    a lone wave owns); the three streaming kernels stay inside 256 registers in all."""
    from openibl_amd import build
    usage = build.resource_usage()
    seen = set()
    for name, u in usage.items():
        for k in KERNELS:
            if k in name:
                assert u.get("ScratchSize", 0) == 0, (name, u)
                assert u["VGPRs"] <= 256, (name, u)
                assert u["VGPRs"] + u.get("AGPRs", 0) <= (512 if k == "region_aggregate_kernel" else 256), (name, u)
                seen.add(k)
    assert seen == set(KERNELS), sorted(set(KERNELS) - seen)


def test_region_aggregation_runs_on_the_matrix_cores():
    """The text of the aggregation kernel: per chunk 128 matrix instructions for the logits and 128 for the
    aggregation (one copy of each loop body or more, never none)."""
    from openibl_amd import build
    text = build.kernel_text()
    if not text:
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    hits = {n: t for n, t in text.items() if "region_aggregate_kernel" in n and not n.endswith(".kd")}
    assert len(hits) == 1, sorted(hits)
    (t,) = hits.values()
    print("region_aggregate_kernel:", t)
    assert t["mfma"] >= 128 + 8, t        # the logits fully unrolled + at least one body of the aggregation loop
    for k in KERNELS[1:]:
        for n, u in text.items():
            if k in n and not n.endswith(".kd"):
                assert u["mfma"] == 0, (n, u)
