"""The frozen-trunk cache without a GPU: the ABI of its entry points (declared, bound, exported, documented, validated
before any HIP call), the host arithmetic of `TrunkCache`, its refusals, and its staleness rules on a stub cache."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("oibl_vgg16_pool4_lines_forward", "oibl_vgg16_pool4_lines_forward_u8",
           "oibl_vgg16_conv5_from_pool4_workspace_bytes", "oibl_vgg16_conv5_from_pool4")
BF16, F32, X3, MX = 0, 1, 2, 3


def test_entries_are_declared_bound_exported_and_documented():
    from openibl_amd import lib
    assert lib.ABI_VERSION == 3 and lib.load().oibl_abi_version() == 3
    code = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "openibl_amd.h").read_text(), flags=re.S)
    doc = (ROOT / "INTEGRATION.md").read_text()
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in lib.SIGNATURES and hasattr(raw, name) and name in doc, name
        decl = re.search(r"\b%s\((.*?)\);" % name, code, flags=re.S).group(1)
        assert len(decl.split(",")) == len(lib.SIGNATURES[name][1]), name


def _aligned():
    buf = ctypes.create_string_buffer(8192)
    return buf, ctypes.addressof(buf) // 256 * 256 + 256      # some non-null, 256-byte aligned address


def test_conv5_from_pool4_argument_validation():
    """Every bad argument returns OIBL_E_INVALID (-1) or OIBL_E_WORKSPACE (-2) with its message before any HIP call
    (there is no device here to call)."""
    from openibl_amd import lib
    h = lib.load()
    buf, p = _aligned()
    arr = (ctypes.c_void_p * 13)(*([p] * 13))
    holes = (ctypes.c_void_p * 13)(*([p] * 11 + [None, p]))
    good = dict(lines=p, N=2, h=4, w=6, wts=arr, bias=arr, prec=F32, feat=p, ws=p, ws_bytes=1024, stream=None)

    def call(**change):
        return h.oibl_vgg16_conv5_from_pool4(*{**good, **change}.values())

    for change, word in ((dict(lines=None), b"null"), (dict(wts=None), b"null"), (dict(bias=None), b"null"),
                         (dict(feat=None), b"null"), (dict(ws=None), b"null"), (dict(wts=holes), b"null"),
                         (dict(bias=holes), b"null"), (dict(N=0), b"bad shape"), (dict(h=0), b"bad shape"),
                         (dict(w=0), b"bad shape"), (dict(w=-3), b"bad shape"), (dict(prec=7), b"bad precision"),
                         (dict(prec=4), b"bad precision"), (dict(prec=-1), b"bad precision"),
                         (dict(ws=p + 4), b"aligned")):
        assert call(**change) == -1, change
        assert word in h.oibl_last_error(), (change, h.oibl_last_error())
    for prec in (BF16, F32, X3, MX):
        assert call(prec=prec) == -2 and b"workspace" in h.oibl_last_error()       # still no HIP call
        need = h.oibl_vgg16_conv5_from_pool4_workspace_bytes(2, 4, 6, prec)
        assert call(prec=prec, ws_bytes=need - 1) == -2


def test_pool4_lines_argument_validation():
    from openibl_amd import lib
    h = lib.load()
    buf, p = _aligned()
    arr = (ctypes.c_void_p * 13)(*([p] * 13))
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    big = 1 << 40
    f, u = h.oibl_vgg16_pool4_lines_forward, h.oibl_vgg16_pool4_lines_forward_u8
    assert f(p, 1, 8, 8, arr, arr, F32, p, p, big, None) == -1 and b"bad shape" in h.oibl_last_error()
    assert f(p, 0, 32, 48, arr, arr, F32, p, p, big, None) == -1 and b"bad shape" in h.oibl_last_error()
    assert f(p, 1, 32, 48, arr, arr, F32, None, p, big, None) == -1 and b"null" in h.oibl_last_error()
    assert f(None, 1, 32, 48, arr, arr, F32, p, p, big, None) == -1 and b"null" in h.oibl_last_error()
    assert f(p, 1, 32, 48, arr, arr, 9, p, p, big, None) == -1 and b"bad precision" in h.oibl_last_error()
    assert f(p, 1, 32, 48, arr, arr, F32, p, p + 8, big, None) == -1 and b"aligned" in h.oibl_last_error()
    assert f(p, 1, 32, 48, arr, arr, F32, p, p, 1024, None) == -2 and b"workspace" in h.oibl_last_error()
    assert u(p, 1, 32, 48, None, m3, arr, arr, F32, p, p, big, None) == -1 and b"mean" in h.oibl_last_error()
    assert u(p, 1, 32, 48, m3, m3, arr, arr, F32, None, p, big, None) == -1 and b"null" in h.oibl_last_error()
    assert u(p, 1, 8, 48, m3, m3, arr, arr, BF16, p, p, big, None) == -1 and b"bad shape" in h.oibl_last_error()
    # the uint8 entry needs the staging area on top: the fp32 entry's workspace is too short for it
    need = h.oibl_vgg16_workspace_bytes(1, 32, 48, F32)
    assert u(p, 1, 32, 48, m3, m3, arr, arr, F32, p, p, need, None) == -2 and b"workspace" in h.oibl_last_error()


def test_conv5_from_pool4_workspace_query():
    """0 for empty problems and unknown precisions; otherwise the flag slot, two activations and the split-K scratch
    of the three layers — the scratch the single-layer query reports for a 512 -> 512 layer of that size."""
    from openibl_amd import lib
    h = lib.load()
    q = h.oibl_vgg16_conv5_from_pool4_workspace_bytes
    for prec in (BF16, F32, X3, MX):
        assert q(0, 30, 40, prec) == 0 and q(1, 0, 40, prec) == 0 and q(1, 30, 0, prec) == 0 and q(-1, 30, 40, prec) == 0
        for n, hh, ww in ((1, 1, 1), (1, 4, 6), (3, 4, 5), (1, 30, 40), (32, 30, 40), (33, 30, 40)):
            act = (n * hh * ww * 512 * (2 if prec == BF16 else 4) + 255) // 256 * 256
            split = h.oibl_conv3x3_workspace_bytes(n, hh, ww, 512, 512, 0, prec)
            assert q(n, hh, ww, prec) == 256 + 2 * act + split, (prec, n, hh, ww)
    for prec in (4, 7, -1):
        assert q(1, 30, 40, prec) == 0


def test_nbytes_arithmetic():
    from openibl_amd.trunk_cache import TrunkCache
    n = 17416
    assert TrunkCache.nbytes(n, 480, 640, "f16mx") == n * 30 * 40 * 512 * 4
    assert TrunkCache.nbytes(n, 480, 640, "bf16x3") == n * 30 * 40 * 512 * 4
    assert TrunkCache.nbytes(n, 480, 640, "fp32") == n * 30 * 40 * 512 * 4
    assert TrunkCache.nbytes(n, 480, 640, "bf16") == n * 30 * 40 * 512 * 2
    assert TrunkCache.nbytes(5, 70, 90, "fp32") == 5 * 4 * 5 * 512 * 4        # floor at every pool
    assert TrunkCache.nbytes(0, 480, 640, "bf16") == 0
    with pytest.raises(ValueError):
        TrunkCache.nbytes(1, 480, 640, "fp8")


def _model(region=False):
    from openibl_amd import models
    base = models.vgg16(pretrained=False)
    for l in list(base.base.children())[:24]:
        for p in l.parameters():
            p.requires_grad = False
    net = models.NetVLAD(num_clusters=64, dim=512)
    return (models.EmbedRegionNet if region else models.EmbedNet)(base, net).eval()


def _stub(model, **change):
    """A cache object as `fill` would leave it for `model`, without lines on a device."""
    from openibl_amd.models import _fingerprint
    from openibl_amd.trunk_cache import TrunkCache, _trunk_params
    base = model.base_model
    kw = dict(lines=torch.empty(0), batches=[(0, 2, base.precision, [(0, 2)])], precision=base.precision,
              fingerprint=_fingerprint(_trunk_params(base)), n_items=2, image_hw=(64, 96),
              min_tiles=base.F16MX_MIN_TILES)
    kw.update(change)
    return TrunkCache(**kw)


def test_ops_and_cache_refuse_cpu_tensors():
    from openibl_amd import ops
    from openibl_amd.lib import OpenIBLAmdError
    from openibl_amd.trunk_cache import TrunkCache
    w = torch.zeros(9, 512, 512)
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ops.vgg16_pool4_lines(torch.zeros(1, 3, 32, 48), [w] * 13, [torch.zeros(512)] * 13, "fp32")
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        ops.vgg16_conv5_from_pool4(torch.zeros(1, 2, 3, 512), [w] * 13, [torch.zeros(512)] * 13, "fp32")
    model = _model()
    loader = [(torch.zeros(2, 3, 64, 96), None)]
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        TrunkCache.fill(model, loader, [("a",), ("b",)])
    with pytest.raises(OpenIBLAmdError, match="no CPU fallback"):
        _stub(model).descriptors(model)            # a valid cache whose lines are not on a device


def test_single_rank_only(monkeypatch):
    from openibl_amd import evaluators, mining
    from openibl_amd.trunk_cache import TrunkCache
    monkeypatch.setattr(evaluators, "_rank_world", lambda: (0, 2))
    with pytest.raises(RuntimeError, match="single rank"):
        TrunkCache.fill(_model(), [], [])
    with pytest.raises(RuntimeError, match="single rank"):       # as today, with and without a cache
        mining.update_sampler(None, None, None, [], [], [], trunk_cache=None)
    with pytest.raises(RuntimeError, match="single rank"):
        mining.update_sampler(None, None, None, [], [], [])


@pytest.mark.parametrize("region", [False, True])
def test_a_stale_cache_is_refused(region):
    model = _model(region)
    cache = _stub(model)
    cache.check(model)                                           # as filled: valid
    cache.check(model, n_items=2)
    with pytest.raises(RuntimeError, match="holds 2 images"):
        cache.check(model, n_items=3)
    # precision
    model.set_precision("bf16" if model.base_model.precision != "bf16" else "fp32")
    with pytest.raises(RuntimeError, match="precision"):
        cache.check(model)
    with pytest.raises(RuntimeError, match="precision"):
        cache.descriptors(model)
    model.set_precision(cache.precision)
    cache.check(model)
    # a trainable trunk parameter
    w = model.base_model.base[17].weight                         # conv4_1
    w.requires_grad = True
    with pytest.raises(RuntimeError, match="requires_grad"):
        cache.descriptors(model)
    w.requires_grad = False
    cache.check(model)
    # conv5 and the NetVLAD layer may move: they are read live
    with torch.no_grad():
        model.base_model.base[28].weight.add_(1.0)
        model.net_vlad.centroids.mul_(0.5)
    cache.check(model)
    # the trunk may not: an in-place update, then a load_state_dict
    with torch.no_grad():
        model.base_model.base[0].bias.add_(1.0)
    with pytest.raises(RuntimeError, match="fingerprint"):
        cache.descriptors(model)
    cache = _stub(model)
    cache.check(model)
    model.load_state_dict(model.state_dict())
    with pytest.raises(RuntimeError, match="fingerprint"):
        cache.check(model)


def test_public_names():
    import ibl.evaluators
    import inspect
    from openibl_amd import mining, trunk_cache
    assert mining.TrunkCache is trunk_cache.TrunkCache and "TrunkCache" in mining.__all__
    assert inspect.signature(mining.update_sampler).parameters["trunk_cache"].default is None
    assert inspect.signature(ibl.evaluators.extract_features).parameters["trunk_cache"].default is None
