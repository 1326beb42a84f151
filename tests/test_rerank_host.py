"""k-reciprocal re-ranking on the device, the parts that need no GPU: the C boundary (header, exports, binder
table, argument validation that returns before any HIP call), the integer form of the reference's 2/3 rule, the
limits and the errors of the Python surface, and the compiler's report on the new kernels."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"
ENTRIES = ("oibl_rerank_row_extremes_workspace_bytes", "oibl_rerank_row_extremes", "oibl_rerank_set_stride",
           "oibl_rerank_sets", "oibl_rerank_weights", "oibl_rerank_expand", "oibl_rerank_invert_workspace_bytes",
           "oibl_rerank_invert", "oibl_rerank_jaccard_workspace_bytes", "oibl_rerank_jaccard")
KERNELS = ("rerank_sqnorm_kernel", "rerank_extremes_kernel", "rerank_rowmax_kernel", "rerank_sets_kernel",
           "rerank_weights_kernel", "rerank_expand_kernel", "rerank_colcount_kernel", "rerank_scan_kernel",
           "rerank_fill_kernel", "rerank_colsort_kernel", "rerank_jaccard_kernel")


def test_header_declares_and_library_exports_the_rerank_entries():
    from openibl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(lib.lib_path()))
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported by the product library"
        assert name in lib.SIGNATURES
        assert name in doc, f"{name} is not named in INTEGRATION.md"


def test_integer_two_thirds_rule_equals_the_reference_expression():
    """rerank.py:62 of the reference tests `len(intersect) > 2. / 3 * len(sub)` in floating point; the set kernel tests
    3 * |intersect| > 2 * |sub| in integers.  Equal for every pair of sizes a set of at most 64 members allows (the
    kernel's sub sets have at most round(31 / 2) + 1 = 17)."""
    for sub in range(0, 65):
        for inter in range(0, sub + 1):
            assert (inter > 2. / 3 * sub) == (3 * inter > 2 * sub), (inter, sub)
            assert (inter > 2.0 / 3.0 * sub) == (3 * inter > 2 * sub), (inter, sub)


def test_half_is_rounded_like_the_reference_and_strides_cover_the_worst_case():
    from openibl_amd import lib, ops
    h = lib.load()
    for k1 in range(1, 32):
        half = ops.rerank_half(k1)
        assert half == int(np.around(k1 / 2.0)), k1           # rerank.py:60: halves to even (k1 = 25 -> 12)
        # base <= k1 + 1 members, each adds at most half + 1
        assert ops.rerank_set_stride(k1) == (k1 + 1) * (half + 2) == h.oibl_rerank_set_stride(k1, half)
        assert ops.rerank_set_stride(k1) <= 576
    assert h.oibl_rerank_set_stride(32, 16) == 0 and h.oibl_rerank_set_stride(0, 0) == 0
    assert h.oibl_rerank_set_stride(31, 31) == 0              # would outgrow the kernel's member buffer


def test_limits_raise_value_error_before_any_device_call():
    from openibl_amd import ops
    from openibl_amd.rerank import re_ranking_features
    q, g = torch.zeros(3, 64), torch.zeros(5, 64)             # CPU tensors: a device call would raise another error
    for bad in (dict(k1=32), dict(k1=0), dict(k2=9), dict(k2=0), dict(k1=40, k2=12)):
        with pytest.raises(ValueError, match="built for"):
            re_ranking_features(q, g, **bad)
    with pytest.raises(ValueError, match="k1 <= 31"):
        ops.rerank_check_limits(32, 1)
    with pytest.raises(ValueError, match="k2 <= 8"):
        ops.rerank_check_limits(20, 9)
    ops.rerank_check_limits(31, 8)
    ops.rerank_check_limits(20, 6)
    ops.rerank_check_limits(25, 1)
    with pytest.raises(ValueError):
        re_ranking_features(q, torch.zeros(5, 32))            # dimension mismatch
    with pytest.raises(ValueError):
        re_ranking_features(q.double(), g.double())


def test_no_cpu_fallback():
    """Descriptors on the host raise the package's error (the host implementation is re_ranking, by name)."""
    from openibl_amd import ops
    from openibl_amd.lib import OpenIBLAmdError
    from openibl_amd.rerank import re_ranking_features
    import ibl.utils.rerank as ref_surface
    assert ref_surface.re_ranking_features is re_ranking_features
    q, g = torch.randn(3, 64), torch.randn(5, 64)
    with pytest.raises(OpenIBLAmdError):
        re_ranking_features(q, g, k1=4, k2=2)
    with pytest.raises(OpenIBLAmdError):
        ops.rerank_row_extremes(q)
    with pytest.raises(OpenIBLAmdError):
        ops.rerank_sets(torch.zeros((4, 5), dtype=torch.int32), 4)


def test_evaluator_option_defaults_off_and_fails_loudly(monkeypatch):
    from ibl.evaluators import Evaluator
    from openibl_amd.lib import OpenIBLAmdError
    model = torch.nn.Identity()
    assert Evaluator(model).device_rerank is False
    ev = Evaluator(model, device_rerank=True)
    assert ev.device_rerank is True
    query = [("q0.png", 0, 0.0, 0.0)]
    gallery = [("g0.png", 0, 0.0, 0.0), ("g1.png", 1, 0.0, 0.0)]
    # the limit is checked before anything is extracted: the loaders are never touched
    with pytest.raises(ValueError, match="k1 <= 31"):
        ev.evaluate(None, query + gallery, query, gallery, [[0]], gallery_loader=None, rerank=True, rr_topk=40)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ev.evaluate(None, query + gallery, query, gallery, [[0]], gallery_loader=None, rerank=True, rr_topk=25)


def test_rerank_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    buf = ctypes.create_string_buffer(4096 + 256)       # never dereferenced: validation fails first
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    n, d = 16816, 4096
    # one partial per row and column chunk, a few chunks: far below the n x n matrix
    w = h.oibl_rerank_row_extremes_workspace_bytes(n, d)
    assert n * 4 <= w <= 64 * n * 4 and w < n * n * 4 // 100
    w250 = h.oibl_rerank_row_extremes_workspace_bytes(92232, d)
    assert 92232 * 4 <= w250 <= 64 * 92232 * 4
    assert h.oibl_rerank_row_extremes_workspace_bytes(0, d) == 0
    rc = h.oibl_rerank_row_extremes(None, n, d, ptr, ptr, ptr, 1 << 30, None)
    assert rc == -1 and b"null" in h.oibl_last_error()
    rc = h.oibl_rerank_row_extremes(ptr, n, 100, ptr, ptr, ptr, 1 << 30, None)
    assert rc == -1 and b"d=100" in h.oibl_last_error()
    rc = h.oibl_rerank_row_extremes(ptr, n, d, ptr, ptr, ptr, 16, None)
    assert rc == -2 and b"workspace" in h.oibl_last_error()
    rc = h.oibl_rerank_sets(ptr, 33, n, 32, 16, ptr, ptr, 1024, None)
    assert rc == -1 and b"k1 = 32" in h.oibl_last_error()
    rc = h.oibl_rerank_sets(ptr, 20, n, 20, 10, ptr, ptr, 252, None)
    assert rc == -1 and b"k1 + 1 = 21" in h.oibl_last_error()          # 20 ranks per item are one too few
    rc = h.oibl_rerank_sets(ptr, 21, n, 20, 10, ptr, ptr, 251, None)
    assert rc == -1 and b"stride 251" in h.oibl_last_error()
    rc = h.oibl_rerank_sets(None, 21, n, 20, 10, ptr, ptr, 252, None)
    assert rc == -1 and b"null" in h.oibl_last_error()
    rc = h.oibl_rerank_weights(ptr, ptr, ptr, n, d, ptr, ptr, 577, ptr, None)
    assert rc == -1 and b"stride 577" in h.oibl_last_error()
    rc = h.oibl_rerank_expand(ptr, 21, n, 9, ptr, ptr, ptr, 252, ptr, ptr, ptr, 9 * 252, None)
    assert rc == -1 and b"k2 = 9" in h.oibl_last_error()
    rc = h.oibl_rerank_expand(ptr, 21, n, 6, ptr, ptr, ptr, 252, ptr, ptr, ptr, 5 * 252, None)
    assert rc == -1 and b"output stride" in h.oibl_last_error()
    assert h.oibl_rerank_invert_workspace_bytes(n, 1000) >= n * 4 + 2 * 1000 * 4
    rc = h.oibl_rerank_invert(ptr, ptr, ptr, 252, n, n * 252 + 1, ptr, ptr, ptr, ptr, 1 << 40, None)
    assert rc == -1 and b"nnz" in h.oibl_last_error()
    rc = h.oibl_rerank_invert(ptr, ptr, ptr, 252, n, 1000, ptr, ptr, ptr, ptr, 64, None)
    assert rc == -2 and b"workspace" in h.oibl_last_error()
    # the Jaccard pass keeps one row of G floats per resident workgroup, never Q x n
    assert 0 < h.oibl_rerank_jaccard_workspace_bytes(8280, 83952) <= 1024 * 83952 * 4 + 256
    assert h.oibl_rerank_jaccard_workspace_bytes(5, 13) == (5 * 13 * 4 + 255) // 256 * 256
    rc = h.oibl_rerank_jaccard(ptr, ptr, ptr, 252, ptr, ptr, ptr, ptr, 5, 13, 0.7, 0.3, ptr, 12, ptr, 1 << 30, None)
    assert rc == -1 and b"ldd=12" in h.oibl_last_error()
    rc = h.oibl_rerank_jaccard(ptr, ptr, ptr, 252, ptr, ptr, ptr, ptr, 5, 13, 0.7, 0.3, ptr, 13, ptr, 8, None)
    assert rc == -2 and b"workspace" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(rc, "rerank_jaccard")


def test_rerank_kernels_do_not_spill_and_the_contraction_runs_on_the_matrix_cores():
    """hipcc's per-kernel report of the current build: no scratch anywhere; the row-extremes kernel keeps the budget
    of two workgroups per CU (<= 256 registers in all) and holds the fp32 core's 64 matrix instructions per K-step
    (4 sub-steps x 2 x 2 tiles x 4), the sparse stages hold none."""
    from openibl_amd import build
    usage = build.resource_usage()
    seen = set()
    for name, u in usage.items():
        for k in KERNELS:
            if k in name:
                assert u.get("ScratchSize", 0) == 0, (name, u)
                assert u["VGPRs"] + u.get("AGPRs", 0) <= 256, (name, u)
                seen.add(k)
    assert seen == set(KERNELS), sorted(set(KERNELS) - seen)
    text = build.kernel_text()
    if not text:
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    for k in KERNELS:
        hits = {n: t for n, t in text.items() if k in n and not n.endswith(".kd")}
        assert len(hits) == 1, (k, sorted(hits))
        (t,) = hits.values()
        assert t["mfma"] == (64 if k == "rerank_extremes_kernel" else 0), (k, t)
