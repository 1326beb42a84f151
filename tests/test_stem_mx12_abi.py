"""The 12-wave f16mx stem (csrc/stem_mx12.h) in the current build, read the way tests/test_abi.py reads the other hot
kernels: the compiler's resource report and the text of the gfx950 code object.  A workgroup of 12 waves leaves a
wave 168 vector registers; the consumers hold 64 accumulators and 64 operand registers in them, so a spill lands in
their matrix loop.  The text holds one body per stage and input half (2 x 9 taps x 12) and one conv1_1 body (6) at each
of the three places the producers run it: more means the compiler has cloned a body."""
from openibl_amd import build


def _only(table):
    hits = {n: v for n, v in table.items() if "stem_mx12_kernel" in n and not n.endswith(".kd")}
    assert len(hits) == 1, sorted(hits)
    return next(iter(hits.values()))


def test_register_budget():
    u = _only(build.resource_usage())
    assert u["VGPRs"] <= 168, u
    assert u.get("AGPRs", 0) == 0, u
    assert u.get("ScratchSize", 0) == 0, u


def test_matrix_instructions_and_code_size():
    text = build.kernel_text()
    if not text:
        import pytest
        pytest.skip("llvm-objdump / clang-offload-bundler not found next to hipcc")
    t = _only(text)
    assert t["mfma"] == 2 * 9 * 12 + 3 * 6 == 234, t
    assert t["bytes"] < 64 * 1024, t
