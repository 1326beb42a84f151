"""The forward descriptor head (csrc/netvlad.hip, csrc/region.hip) in the trained and the saturated regime, at the
slab, chunk and tile edges of every dispatch path, against the fp64 oracle (GPU).

Cases, inputs and references: tests/helpers/head_forward_ref.py; tests/test_head_forward_cases_cpu.py shows on the host
that every case is well conditioned (plain fp32 reproduces fp64 within 5e-6), is in the regime it names (mean max_k a
>= 0.70 at sharpen 1, >= 0.9999 at sharpen 4) and has the slab arithmetic it is listed for.

Bars (the project's own): fp32 maps 5e-6 rel-L2, per image and on the whole tensor; bf16 maps 2e-5 against the oracle
on the bf16-rounded map and weight; region head 5e-6 on the whole tensor and 1e-4 per (image, region) vector.  Every
measured error is printed next to the host-fp32 figure of the same case.

Bit-equalities asserted are the ones the code promises: a row's result does not depend on its batch mates within one
kernel selection; raw-only and normalised-only calls of the fused path give the bits of the call that asks for both;
ops.netvlad_head is ops.netvlad; two runs are identical.  Two paths are never compared for closeness — each is held
to fp64 — only for `not torch.equal`, to show that the hook did select another kernel.
"""
from contextlib import contextmanager, nullcontext

import pytest
import torch

from helpers import head_forward_ref as hf
from openibl_amd import ops

pytestmark = pytest.mark.gpu

TOL = {"fp32": hf.TOL_F32, "bf16": hf.TOL_BF16}


@contextmanager
def netvlad_hook(value):
    """oibl_debug_set_netvlad_slabs: 0 five launches never split, 1 default, 2 five launches with the pixel split
    for fp32 maps of any N (the split itself still needs N <= 4), 3 the fused kernel at any N (fp32 maps)."""
    from openibl_amd import lib
    hooks = lib.debug_hooks()
    hooks.oibl_debug_set_netvlad_slabs(value)
    try:
        yield
    finally:
        hooks.oibl_debug_set_netvlad_slabs(1)


def _map(x, precision, dev):
    return (x if precision == "fp32" else x.to(torch.bfloat16)).to(dev)


def _call(feat, n, aw, c, normalize=True, raw=True, nrm=True, hook=None):
    f = feat[:n].contiguous()
    if hook is None:
        return ops.netvlad(f, aw, c, normalize, want_raw=raw, want_norm=nrm)
    with netvlad_hook(hook):
        return ops.netvlad(f, aw, c, normalize, want_raw=raw, want_norm=nrm)


def _judge(name, got, want, tol, host):
    """Whole tensor and per image against fp64 at `tol`; finite."""
    got = got.cpu()
    n = got.shape[0]
    whole, worst = hf.rel_l2(got, want[:n]), hf.worst_row(got, want[:n], n)
    print(f"{name}: whole {whole:.3e} worst image {worst:.3e} (bar {tol:.1e}; host fp32 {host:.3e})")
    assert torch.isfinite(got).all(), f"{name}: non-finite values"
    assert whole <= tol and worst <= tol, f"{name}: whole {whole:.3e} worst image {worst:.3e} > {tol:g}"
    return worst


def _same(a, b, n=None):
    return all(torch.equal(u if n is None else u[:n], v if n is None else v[:n]) for u, v in zip(a, b))


CASE_IDS = [(c, p) for c in hf.NETVLAD_CASES for p in c.precisions]


@pytest.mark.parametrize("sharpen", hf.SHARPEN)
@pytest.mark.parametrize("case,precision", CASE_IDS,
                         ids=[f"{c.path}-{c.drawn}x{c.hw[0]}x{c.hw[1]}-{p}" for c, p in CASE_IDS])
def test_netvlad_trained_at_the_edges(dev, case, precision, sharpen):
    x, aw, c, _ = hf.netvlad_case(case, sharpen)
    ref = hf.netvlad_reference(case, sharpen, precision)
    feat, awd, cd = _map(x, precision, dev), aw.to(dev), c.to(dev)
    hook = 3 if case.path == "fused3" else None
    tol, tag = TOL[precision], f"{case.path} {case.drawn}x{case.hw} sharpen {sharpen} {precision}"
    outs = {n: _call(feat, n, awd, cd, hook=hook) for n in case.calls}
    for n, (raw, nrm) in outs.items():
        _judge(f"{tag} N={n} raw", raw, ref["raw"], tol, ref["host_raw"])
        _judge(f"{tag} N={n} normalised", nrm, ref["nrm"], tol, ref["host_nrm"])
        rn = nrm.double().norm(dim=1)
        assert float((rn - 1).abs().max()) <= 1e-5
    big = outs[case.drawn]
    assert _same(_call(feat, case.drawn, awd, cd, hook=hook), big), "two runs differ"
    for n in case.calls:                                   # rows independent of their batch mates (one kernel selection)
        assert _same(outs[n], big, n), f"rows of the N={n} call differ from the N={case.drawn} call"
    if precision == "fp32":                                # (netvlad_head widens a bf16 map: another kernel)
        with nullcontext() if hook is None else netvlad_hook(hook):
            assert torch.equal(ops.netvlad_head(feat, awd, cd, True), big[1])
    # the case reached the path it names: another selection gives other bits
    if case.path == "unsplit":
        assert _same(_call(feat, case.drawn, awd, cd, hook=0), big)            # never split == default: unsplit
        if precision == "fp32":
            assert not torch.equal(_call(feat, case.drawn, awd, cd, hook=3)[0], big[0])
    elif case.path == "slabs":
        whole = _call(feat, case.drawn, awd, cd, hook=0)
        assert not torch.equal(whole[0], big[0]) and not torch.equal(whole[1], big[1])
    elif case.path == "fused":
        for h in (0, 2):                                   # both mean the five launches, unsplit, at N >= 16
            old = _call(feat, 18, awd, cd, hook=h)
            assert not torch.equal(old[0], outs[18][0]) and not torch.equal(old[1], outs[18][1])
    else:
        old = _call(feat, case.drawn, awd, cd)
        assert not torch.equal(old[0], big[0]) and not torch.equal(old[1], big[1])
    if case.path in ("fused", "fused3"):                   # one output asked for: the bits of the call for both
        n = case.calls[0]
        assert torch.equal(_call(feat, n, awd, cd, nrm=False, hook=hook)[0], outs[n][0])
        assert torch.equal(_call(feat, n, awd, cd, raw=False, hook=hook)[1], outs[n][1])


@pytest.mark.parametrize("path,precision", [("five", "fp32"), ("fused3", "fp32"), ("five", "bf16")])
@pytest.mark.parametrize("scale", hf.LARGE_LOGIT_SCALES)
def test_netvlad_large_logits_without_input_normalisation(dev, scale, path, precision):
    """max |logit| ~ 800 and ~ 3200: a softmax that forgets its maximum overflows; the pixel that is all zeros has
    the uniform softmax."""
    x, aw, c, _ = hf.large_logit_case(scale)
    xi, wi = (x, aw) if precision == "fp32" else (hf.bf16_mirror(x), hf.bf16_mirror(aw))
    want_raw, want_nrm = hf.oracle_netvlad(xi, wi, c, False)
    hr, hn = hf.host_fp32(xi, wi, c, False)
    feat, awd, cd = _map(x, precision, dev), aw.to(dev), c.to(dev)
    hook = 3 if path == "fused3" else None
    raw, nrm = _call(feat, 2, awd, cd, normalize=False, hook=hook)
    tag = f"scale {scale} {path} {precision} (max |logit| {hf.max_abs_logit(xi, wi, False):.0f})"
    _judge(f"{tag} raw", raw, want_raw, TOL[precision], hf.worst_row(hr, want_raw, 2))
    _judge(f"{tag} normalised", nrm, want_nrm, TOL[precision], hf.worst_row(hn, want_nrm, 2))
    if precision == "fp32":
        other = _call(feat, 2, awd, cd, normalize=False, hook=None if hook == 3 else 3)
        assert not torch.equal(other[0], raw)              # (the hook did select the other kernel)


def _judge_region(tag, vec, want, host):
    vec = vec.cpu()
    rows = want.shape[0] * 9
    whole, worst = hf.rel_l2(vec, want), hf.worst_row(vec, want, rows)
    print(f"{tag}: whole {whole:.3e} (bar {hf.TOL_REGION:.1e}) worst vector {worst:.3e} (bar {hf.TOL_VEC:.1e}; "
          f"host fp32 {host:.3e})")
    assert torch.isfinite(vec).all(), f"{tag}: non-finite values"
    assert whole <= hf.TOL_REGION and worst <= hf.TOL_VEC, (tag, whole, worst)
    norms = vec.double().norm(dim=-1)
    assert float((norms - 1).abs().max()) <= 1e-5, f"{tag}: not unit vectors"


@pytest.mark.parametrize("sharpen", hf.SHARPEN)
@pytest.mark.parametrize("case", hf.REGION_CASES, ids=lambda c: f"{c.drawn}x{c.hw[0]}x{c.hw[1]}")
def test_region_head_trained_at_the_edges(dev, case, sharpen):
    x, aw, c, _ = hf.region_case(case, sharpen)
    want = hf.oracle_region(x, aw, c, True)
    host = hf.worst_row(hf.host_fp32(x, aw, c, True, region=True), want, case.drawn * 9)
    xd, awd, cd = x.to(dev), aw.to(dev), c.to(dev)
    vec = ops.region_vlad(xd, awd, cd, True)
    tag = f"region {case.drawn}x{case.hw} sharpen {sharpen}"
    _judge_region(tag, vec, want, host)
    # region 0 is the whole image: the normalised VLAD of the oracle, to the bar
    _, whole_img = hf.oracle_netvlad(x, aw, c, True)
    e0 = hf.worst_row(vec[:, 0].cpu(), whole_img, case.drawn)
    print(f"{tag}: region 0 against the whole image's normalised VLAD, worst image {e0:.3e}")
    assert e0 <= hf.TOL_REGION
    assert torch.equal(ops.region_vlad(xd[:1].contiguous(), awd, cd, True), vec[:1]), "image 0 alone: other bits"
    assert torch.equal(ops.region_vlad(xd, awd, cd, True), vec), "two runs differ"


def test_region_head_large_logits_without_input_normalisation(dev):
    x, aw, c, _ = hf.region_raw_case()
    want = hf.oracle_region(x, aw, c, False)
    host = hf.worst_row(hf.host_fp32(x, aw, c, False, region=True), want, 18)
    vec = ops.region_vlad(x.to(dev), aw.to(dev), c.to(dev), False)
    _judge_region(f"region 2x{hf.REGION_RAW_HW} x {hf.REGION_RAW_SCALE}, normalize_input=False "
                  f"(max |logit| {hf.max_abs_logit(x, aw, False):.0f})", vec, want, host)
