"""Cases and yardsticks of the forward descriptor head tests (tests/test_head_forward_cases_cpu.py,
tests/test_gpu_head_forward_edges.py, the PCA cases of tests/test_gpu_netvlad_pca.py).  TEST INFRASTRUCTURE ONLY.

Inputs are the trained-like recipe of netvlad_grad_ref.draw_trained_inputs (populate=True) with two whole pixels
cleared: x[0, 0, 0, :] and x[-1, -1, -1, :] (the eps clamp of 1 / |x_p| and a pixel whose softmax is uniform).  The
reference is the fp64 oracle (oracle.descriptor, helpers.region_ref); `host_fp32` restates the same head in float32 on
the host and is the CONDITIONING yardstick: a case belongs in the GPU tests only if plain fp32 arithmetic reproduces
the fp64 result within the bar the kernels are held to.

Conditioning rule: a case is DRAWN at N >= 2 images, and a test that calls a kernel on fewer images keeps that draw's
w and c.  The recipe sets c_k to the mean of the normalised pixels labelled k; drawn from ONE image of few pixels a
cluster holds one pixel, c_k is that pixel, and under sharpen = 4 (a_pk = 1 on it) the residual xh_p - c_k is the
rounding of its own subtraction: the fp32 restatement is then wrong by O(1) against fp64.  That is an ill-conditioned
input, not a shape, and it is excluded by construction.

The slab and chunk arithmetic of the kernels is restated here in Python (the `*_slabs` functions); the CPU test ties
these restatements to the constants in the kernel sources and asserts, per case, the edge the case is listed for.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

from helpers import netvlad_grad_ref as nref
from helpers import region_ref
from oracle import descriptor as od

K, C = 64, 512
SHARPEN = (1.0, 4.0)
MIN_MEAN_MAX_A = {1.0: 0.70, 4.0: 0.9999}     # the regime a `sharpen` value must reach (info["mean_max_a"])
EXPF_OVERFLOW = 88.0                           # expf(l) is inf from l = 88.73 on: a softmax without its maximum
TOL_F32, TOL_BF16 = 5e-6, 2e-5                 # tests/test_gpu_netvlad_pca.py's bars against fp64
TOL_REGION, TOL_VEC = 5e-6, 1e-4               # tests/test_gpu_region_backward.py's forward bar; test_gpu_region.py's

_cache = {}


# ---- inputs ---------------------------------------------------------------------------------------------------------
def trained_case(seed, N, h, w, sharpen):
    """(x [N][h][w][C], w [K][C], c [K][C], info) as fp32 torch tensors, once per session; treat them as read-only."""
    key = ("case", seed, N, h, w, float(sharpen))
    if key not in _cache:
        x, aw, c, _, info = nref.draw_trained_inputs(seed, N, h, w, sharpen=float(sharpen), populate=True)
        x[0, 0, 0, :] = 0.0
        x[-1, -1, -1, :] = 0.0
        info = {k: v for k, v in info.items() if k != "descs"}
        _cache[key] = (torch.from_numpy(x), torch.from_numpy(aw), torch.from_numpy(c), info)
    return _cache[key]


def netvlad_seed(h, w):
    return 700 + h + w


def region_seed(h, w):
    return 800 + h + w


def bf16_mirror(t):
    return t.to(torch.bfloat16).float()


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# ---- references -----------------------------------------------------------------------------------------------------
def oracle_netvlad(x, aw, c, normalize_input=True):
    """fp64: (raw [N][K][C], normalised [N][K*C]) of an NHWC map."""
    raw = od.netvlad(_nchw(x).double(), aw.double().view(K, C, 1, 1), c.double(), normalize_input)
    return raw, od.normalize_vlad(raw)


def oracle_region(x, aw, c, normalize_input=True):
    """fp64: [N][9][K*C]."""
    return region_ref.region_vectors(_nchw(x), aw.view(K, C, 1, 1), c, normalize_input)


def host_fp32(x, aw, c, normalize_input=True, region=False):
    """The same head in float32 on the host: (raw, normalised) float32 tensors, or [N][9][K*C] for the region head
    (region_ref.region_vectors' composition: NetVLAD per quarter, the quarters added in region order, normalised)."""
    assert x.dtype == aw.dtype == c.dtype == torch.float32
    f = _nchw(x)
    w4 = aw.view(K, C, 1, 1)
    if not region:
        raw = od.netvlad(f, w4, c, normalize_input)
        return raw, od.normalize_vlad(raw)
    q = [od.netvlad(b.contiguous(), w4, c, normalize_input) for b in region_ref.quarters(f)]
    out = []
    for members in region_ref.REGIONS:
        raw = q[members[0]]
        for m in members[1:]:
            raw = raw + q[m]
        out.append(od.normalize_vlad(raw))
    res = torch.stack(out, dim=1)
    assert res.dtype == torch.float32
    return res


def rel_l2(got, want):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-300))


def worst_row(got, want, rows):
    """max over the leading `rows` axes (flattened) of the rel-L2 of what is left."""
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    g, w_ = got.reshape(rows, -1), want.reshape(rows, -1)
    return float(((g - w_).norm(dim=1) / w_.norm(dim=1).clamp_min(1e-300)).max())


def max_abs_logit(x, aw, normalize_input):
    xd = x.double().reshape(-1, C)
    if normalize_input:
        xd = xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return float((xd @ aw.double().t()).abs().max())


# ---- the kernels' slab arithmetic, restated (netvlad.hip, region.hip, pca.hip) -----------------------------------
NVF_MIN_N = 16                   # fp32 maps: the fused kernel serves batches from this size on
ASSIGN_BM = 128                  # rows of the soft-assignment tile
CHUNK = 32                       # pixels per chunk of the aggregation kernels
RG_SLAB_TARGET = 64
PS_ROWS, PS_SPLITS, PS_MAXN = 8, 8, 2
PK_WAVES, PK_SPLITS, PK_CHUNK, PK_MAXN = 8, 32, 256, 32
PRN_PER = 4


def _sizes(P, px, n):
    return [max(0, min(P - i * px, px)) for i in range(n)]


def nv_pixel_slabs(N, P):
    """Five launches: (slabs, pchunk, pixels per slab) of the aggregation."""
    slabs = 4 if (N <= 4 and P >= 256) else 1
    pchunk = (((P + slabs - 1) // slabs + 31) // 32) * 32 if slabs > 1 else P
    return slabs, pchunk, _sizes(P, pchunk, slabs)


def nvf_slab_px(N):
    return 160 if N >= 16 else 96 if N >= 8 else 64 if N >= 4 else 32


def nvf_slabs(N, P):
    """The fused kernel: (slabs, pixels per slab)."""
    px = nvf_slab_px(N)
    n = (P + px - 1) // px
    return n, _sizes(P, px, n)


def rg_slabs(h, w):
    """The region head: (Pq, slabs per quarter, pixels per slab)."""
    pq = (h // 2) * (w // 2)
    n = (pq + RG_SLAB_TARGET - 1) // RG_SLAB_TARGET
    px = (pq + n - 1) // n
    return pq, n, _sizes(pq, px, n)


def chunks(pixels):
    """32-pixel chunks of a slab: (count, pixels in the last one)."""
    n = (pixels + CHUNK - 1) // CHUNK
    return n, pixels - (n - 1) * CHUNK if n else 0


def pca_small_ok(N, D, d, bf16=False):
    return (not bf16) and N <= PS_MAXN and d % (4 * PS_ROWS) == 0 and D % (PS_SPLITS * 512) == 0


def pca_stream_ok(N, D, d):
    return 1 <= N <= PK_MAXN and d % (32 * PK_WAVES) == 0 and D % (PK_SPLITS * PK_CHUNK) == 0


def pca_splits(N, D, d, bf16=False):
    """The split-K plan of the MFMA tile: (K-steps, splits)."""
    ksteps = D // (64 if bf16 else 32)
    tiles = ((N + 31) // 32) * (d // 128)
    s = 1
    while tiles * s < 512 and ksteps % (s * 2) == 0 and ksteps // (s * 2) >= 16:
        s *= 2
    return ksteps, s


# ---- the case lists ------------------------------------------------------------------------------------------------
# path: "unsplit" five launches, one aggregation workgroup per (image, channel slice); "slabs" five launches, the
# aggregation over 4 pixel slabs; "fused" the fused kernel by default (fp32, N >= 16); "fused3" the fused kernel
# behind hook 3.  `drawn` images are drawn, the kernel is called on the first n of them for every n of `calls`.
NvCase = namedtuple("NvCase", "path drawn calls hw precisions edge")
NETVLAD_CASES = (
    NvCase("unsplit", 2, (2,), (1, 31), ("fp32", "bf16"), "P = 31: a chunk one pixel short"),
    NvCase("unsplit", 2, (2,), (4, 8), ("fp32", "bf16"), "P = 32: exactly one chunk"),
    NvCase("unsplit", 2, (2,), (3, 11), ("fp32", "bf16"), "P = 33: a one-pixel second chunk"),
    NvCase("unsplit", 2, (2,), (15, 17), ("fp32", "bf16"), "P = 255: the last size below the pixel split"),
    NvCase("unsplit", 3, (3,), (1, 43), ("fp32", "bf16"), "N P = 129: the assign tile's row clamp"),
    NvCase("slabs", 2, (2, 1), (16, 16), ("fp32", "bf16"), "P = 256: the first split size, four 64-pixel slabs"),
    NvCase("slabs", 2, (2, 1), (16, 17), ("fp32", "bf16"), "P = 272: pchunk 96, slab 3 empty"),
    NvCase("slabs", 2, (2, 1), (13, 20), ("fp32", "bf16"), "P = 260: pchunk 96, slab 3 empty"),
    NvCase("slabs", 2, (2, 1), (11, 35), ("fp32", "bf16"), "P = 385: pchunk 128, slab 3 is one pixel"),
    NvCase("fused", 20, (16, 18, 20), (3, 53), ("fp32",), "P = 159: one slab, a chunk one pixel short"),
    NvCase("fused", 20, (16, 18, 20), (8, 20), ("fp32",), "P = 160: exactly one slab"),
    NvCase("fused", 20, (16, 18, 20), (7, 23), ("fp32",), "P = 161: a one-pixel second slab"),
    NvCase("fused", 20, (16, 18, 20), (3, 107), ("fp32",), "P = 321: two full slabs and a one-pixel third"),
    NvCase("fused3", 2, (2, 1), (3, 11), ("fp32",), "N = 2: 32-pixel slabs, P = 33"),
    NvCase("fused3", 5, (5, 4), (5, 13), ("fp32",), "N = 5: 64-pixel slabs, P = 65"),
    NvCase("fused3", 9, (9, 8), (1, 97), ("fp32",), "N = 9: 96-pixel slabs, P = 97"),
)
# normalize_input=False: the N = 2, 7 x 23 trained map (sharpen 1) times these scales
LARGE_LOGIT_HW, LARGE_LOGIT_SCALES = (7, 23), (0.25, 1.0)

RgCase = namedtuple("RgCase", "drawn hw edge")
REGION_CASES = (
    RgCase(2, (2, 2), "Pq = 1"),
    RgCase(2, (8, 16), "Pq = 32: one full chunk"),
    RgCase(2, (6, 22), "Pq = 33: a one-pixel second chunk"),
    RgCase(2, (2, 66), "Pq = 33, a quarter is a single row"),
    RgCase(2, (14, 18), "Pq = 63"),
    RgCase(2, (16, 16), "Pq = 64: one full slab"),
    RgCase(2, (10, 26), "Pq = 65: two slabs, 33 + 32"),
    RgCase(3, (4, 6), "three images, Pq = 6"),
)
REGION_RAW_HW, REGION_RAW_SCALE = (6, 22), 0.25      # the normalize_input=False case


def netvlad_case(case, sharpen):
    h, w = case.hw
    return trained_case(netvlad_seed(h, w), case.drawn, h, w, sharpen)


def large_logit_case(scale):
    h, w = LARGE_LOGIT_HW
    x, aw, c, info = trained_case(netvlad_seed(h, w), 2, h, w, 1.0)
    return x * float(scale), aw, c, info


def region_case(case, sharpen):
    h, w = case.hw
    return trained_case(region_seed(h, w), case.drawn, h, w, sharpen)


def region_raw_case():
    h, w = REGION_RAW_HW
    x, aw, c, info = trained_case(region_seed(h, w), 2, h, w, 1.0)
    return x * REGION_RAW_SCALE, aw, c, info


def netvlad_reference(case, sharpen, precision):
    """{"raw", "nrm"} fp64 of the drawn images (bf16: of the bf16-rounded map and weight), and {"host_raw",
    "host_nrm"} the worst per-image error of the fp32 host restatement on the same inputs; once per session."""
    key = ("nvref", case, float(sharpen), precision)
    if key not in _cache:
        x, aw, c, _ = netvlad_case(case, sharpen)
        if precision == "bf16":
            x, aw = bf16_mirror(x), bf16_mirror(aw)
        raw, nrm = oracle_netvlad(x, aw, c, True)
        hr, hn = host_fp32(x, aw, c, True)
        N = x.shape[0]
        _cache[key] = {"raw": raw, "nrm": nrm, "host_raw": worst_row(hr, raw, N), "host_nrm": worst_row(hn, nrm, N)}
    return _cache[key]


# PCA off the production shape: W ~ 0.01 N(0,1), b ~ 0.1 N(0,1), unit-norm rows
def pca_problem(seed, N, D, d):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn((d, D), generator=g) * 0.01
    b = torch.randn(d, generator=g) * 0.1
    v = torch.nn.functional.normalize(torch.randn((N, D), generator=g), dim=1)
    return v, w, b


def pca_oracle(v, w, b, bf16=False, l2norm=True):
    """od.pca_project in fp64 (bf16: of the bf16-rounded v and w); l2norm False: the projection itself."""
    if bf16:
        v, w = bf16_mirror(v), bf16_mirror(w)
    if l2norm:
        return od.pca_project(v.double(), w.double(), b.double())
    return v.double() @ w.double().t() + b.double()
