"""NetVLAD initialisation without a checkpoint, the parts that need no GPU: the C boundary of csrc/netvlad_init.hip
(header, exports, bindings, argument validation before any HIP call), numpy's draws of the sampled positions in the
reference's order, the fill order of sample_local_descriptors with an injected gather, the cache file through the
npz path (h5py made unimportable for the test), and the golden fixture against a float64 evaluation of the
reference's formula."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "openibl_amd.h"
ENTRIES = ("oibl_local_descriptors", "oibl_assign_gap_workspace_bytes", "oibl_assign_gap")
KERNELS = ("local_descriptors_kernel", "assign_normalize_kernel", "assign_gap_kernel", "assign_gap_sum_kernel")


def test_header_declares_and_library_exports_the_init_entries():
    from openibl_amd import lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    declared = set(re.findall(r"\b(oibl_[a-z0-9_]+)\s*\(", text))
    raw = ctypes.CDLL(str(lib.lib_path()))
    for name in ENTRIES:
        assert name in declared, f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported by the product library"
        assert name in lib.SIGNATURES
        assert name in (ROOT / "INTEGRATION.md").read_text()


def test_argument_validation_launches_nothing():
    from openibl_amd import lib
    h = lib.load()
    # the workspace is the transposed copy of the normalised centres, K padded to a multiple of 64
    assert h.oibl_assign_gap_workspace_bytes(50000, 64, 512) >= 64 * 512 * 4
    assert h.oibl_assign_gap_workspace_bytes(1, 2, 64) >= 64 * 64 * 4
    assert h.oibl_assign_gap_workspace_bytes(300, 256, 64) >= 256 * 64 * 4
    for bad in ((0, 64, 512), (10, 1, 512), (10, 257, 512), (10, 64, 96), (10, 64, 0)):
        assert h.oibl_assign_gap_workspace_bytes(*bad) == 0, bad
    buf = ctypes.create_string_buffer(4096 + 256)       # never dereferenced: validation fails first
    ptr = (ctypes.addressof(buf) + 255) // 256 * 256
    big = 1 << 30

    def gap(descs=ptr, n=10, clsts=ptr, K=64, C=512, ca=ptr, g=ptr, gs=ptr, ws=ptr, ws_bytes=big):
        return h.oibl_assign_gap(descs, n, clsts, K, C, ca, g, gs, ws, ws_bytes, None)

    for kw in ({"descs": None}, {"clsts": None}, {"ca": None}, {"g": None}, {"gs": None}, {"ws": None}):
        assert gap(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert gap(K=1) == -1 and b"num_clusters" in h.oibl_last_error() and b"got 1" in h.oibl_last_error()
    assert gap(K=257) == -1 and b"num_clusters" in h.oibl_last_error() and b"got 257" in h.oibl_last_error()
    assert gap(C=96) == -1 and b"multiple of 64" in h.oibl_last_error() and b"96" in h.oibl_last_error()
    assert gap(n=0) == -1 and b"n = 0" in h.oibl_last_error()
    assert gap(ws=ptr + 64) == -1 and b"aligned" in h.oibl_last_error()
    assert gap(ws_bytes=1024) == -2 and b"workspace" in h.oibl_last_error()
    with pytest.raises(lib.OpenIBLAmdError):
        lib.check(-2, "assign_gap")

    F32, BF16, X3 = 1, 0, 2

    def loc(feat=ptr, N=2, P=24, C=64, prec=F32, pos=ptr, S=5, out=ptr):
        return h.oibl_local_descriptors(feat, N, P, C, prec, pos, S, out, None)

    for kw in ({"feat": None}, {"pos": None}, {"out": None}):
        assert loc(**kw) == -1 and b"null" in h.oibl_last_error(), kw
    assert loc(C=96) == -1 and b"multiple of 64" in h.oibl_last_error()
    assert loc(prec=X3) == -1 and b"bf16 or fp32" in h.oibl_last_error()
    assert loc(N=0) == -1 and loc(P=0) == -1 and loc(S=0) == -1 and b"bad shape" in h.oibl_last_error()
    assert BF16 == 0


def test_init_kernels_do_not_spill_and_fit_the_register_file():
    """hipcc's report of the current build: no scratch, inside 256 registers (the gap kernel holds 8 descriptors x up
    to 4 cluster passes of accumulators per lane)."""
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


def test_sample_positions_are_numpys_draws_in_image_order():
    from openibl_amd.cluster import sample_positions
    np.random.seed(43)
    want = np.stack([np.random.choice(1200, 100, replace=False) for _ in range(5)])
    np.random.seed(43)
    got = sample_positions(5, 1200, 100)
    assert got.shape == (5, 100) and np.array_equal(got, want)
    rng = np.random.RandomState(7)
    want = np.stack([rng.choice(24, 24, replace=False) for _ in range(3)])
    got = sample_positions(3, 24, 24, rng=np.random.RandomState(7))
    assert np.array_equal(got, want) and all(sorted(r) == list(range(24)) for r in got.tolist())
    with pytest.raises(ValueError):
        sample_positions(2, 24, 25)
    with pytest.raises(ValueError):
        np.random.choice(24, 25, replace=False)        # as numpy does


class _FakeBase:
    """features_nhwc of image i (whose pixels all hold the value v_i) is a 2 x 3 x 64 map whose pixel p holds
    v_i * 100 + p in every channel."""

    def __init__(self, flagged=False):
        self.calls = []
        self.flagged = flagged

    def _map(self, x, offset=0.0):
        v = x.reshape(x.shape[0], -1)[:, 0]
        pix = torch.arange(6, dtype=torch.float32).view(1, 2, 3, 1)
        return (v.view(-1, 1, 1, 1) * 100 + pix + offset).expand(-1, -1, -1, 64).contiguous()

    def features_nhwc(self, x, defer_flag=False):
        assert defer_flag
        self.calls.append(int(x.shape[0]))
        return self._map(x, 0.5 if self.flagged else 0.0)     # a flagged f16mx map is NOT the one to keep

    def settle_range_flag(self, x):
        return self._map(x) if self.flagged else None


def _fake_gather(feat, pos):
    N, C = feat.shape[0], feat.shape[-1]
    flat = feat.reshape(N, -1, C)
    return torch.stack([flat[n, int(p)] for n in range(N) for p in pos[n]])


@pytest.mark.parametrize("flagged", [False, True])
def test_sample_local_descriptors_fills_in_the_reference_order(flagged):
    from openibl_amd.cluster import sample_local_descriptors

    class Model:
        base_model = _FakeBase(flagged)

    # 3 batches of 3 images (the last as the loader's 5-tuple), 2 per image, 14 descriptors -> 7 images
    imgs = [torch.full((3, 3, 4, 4), float(3 * b)) + torch.arange(3.).view(3, 1, 1, 1) for b in range(4)]
    batches = [imgs[0], imgs[1], (imgs[2], None, None, None, None), imgs[3]]
    rng = np.random.RandomState(43)
    out = sample_local_descriptors(Model, batches, n_descriptors=14, n_per_image=2, rng=rng, gather_fn=_fake_gather)
    assert tuple(out.shape) == (14, 64) and out.dtype == torch.float32
    assert Model.base_model.calls == [3, 3, 1]               # stops at ceil(14 / 2) = 7 images, the 4th batch unread
    rng = np.random.RandomState(43)
    want = [[100.0 * i + p for p in rng.choice(6, 2, replace=False)] for i in range(7)]
    assert out[:, 0].view(7, 2).tolist() == want             # row = batchix + ix * nPerImage
    # an odd total: the last image's rows are cut
    out = sample_local_descriptors(_FakeBase(), [imgs[0]], n_descriptors=5, n_per_image=2,
                                   rng=np.random.RandomState(43), gather_fn=_fake_gather)
    assert out[:, 0].tolist() == [v for row in want[:3] for v in row][:5]
    with pytest.raises(RuntimeError, match="7 images"):
        sample_local_descriptors(_FakeBase(), batches[:2], n_descriptors=14, n_per_image=2, gather_fn=_fake_gather)
    with pytest.raises(ValueError):
        sample_local_descriptors(_FakeBase(), batches, n_descriptors=14, n_per_image=7, gather_fn=_fake_gather)


def test_cache_file_round_trips_through_the_npz_path(tmp_path, monkeypatch):
    from openibl_amd import cluster

    monkeypatch.setitem(sys.modules, "h5py", None)            # `import h5py` raises ImportError: the npz path, everywhere
    seen = {}

    def fake_kmeans(descs, num_clusters, max_iter, seed, **kw):
        seen.update(n=tuple(descs.shape), k=num_clusters, it=max_iter, seed=seed)
        return np.asarray(descs[:num_clusters].numpy() * 2, dtype=np.float32)

    monkeypatch.setattr(cluster, "kmeans_centroids", fake_kmeans)
    imgs = [torch.full((4, 3, 4, 4), float(4 * b)) + torch.arange(4.).view(4, 1, 1, 1) for b in range(2)]
    path = str(tmp_path / "logs" / "vgg16_pitts_4_desc_cen.hdf5")
    got = cluster.build_init_cache(_FakeBase(), imgs, path, num_clusters=4, seed=43, max_iter=7, n_descriptors=16,
                                   n_per_image=2, rng=np.random.RandomState(1), gather_fn=_fake_gather)
    assert got == path and Path(path).is_file()
    assert seen == {"n": (16, 64), "k": 4, "it": 7, "seed": 43}
    with open(path, "rb") as f:
        assert f.read(2) == b"PK"                             # without h5py: an npz archive AT the .hdf5 path
    z = np.load(path)
    assert sorted(z.files) == ["centroids", "descriptors"]
    clsts, descs = cluster.load_init_cache(path)
    assert clsts.dtype == descs.dtype == np.float32 and clsts.shape == (4, 64) and descs.shape == (16, 64)
    assert np.array_equal(descs, z["descriptors"]) and np.array_equal(clsts, descs[:4] * 2)
    # the PCA parameter file still goes through the same helpers
    from openibl_amd import pca
    p2 = pca._write_params(str(tmp_path / "pca.h5"), np.eye(3), np.ones(3), np.zeros((3, 1)), np.zeros((3, 1)))
    U, lams, mu, Utmu = pca._read_params(p2)
    assert np.array_equal(U, np.eye(3)) and lams.shape == (3,) and mu.shape == Utmu.shape == (3, 1)


def test_init_params_names_what_is_missing_and_needs_the_device():
    from openibl_amd import lib, models
    pool = models.create("netvlad", num_clusters=64, dim=128)
    with pytest.raises(ValueError, match="clsts"):
        pool._init_params()
    pool.clsts = np.zeros((64, 128), np.float32)
    with pytest.raises(ValueError, match="traindescs"):
        pool._init_params()
    pool.traindescs = np.zeros((10, 128), np.float32)
    pool.clsts = np.zeros((20, 128), np.float32)
    with pytest.raises(ValueError, match="64 clusters"):
        pool._init_params()
    if not torch.cuda.is_available():
        pool.clsts = np.ones((64, 128), np.float32)
        with pytest.raises(lib.OpenIBLAmdError, match="no CPU fallback"):
            pool._init_params()


def test_golden_holds_the_issue_cases_and_is_well_conditioned():
    """The fixture against a float64 evaluation of ibl/models/netvlad.py:35-42 on its own inputs: 1e-5, so that the
    1e-4 bar of the GPU tests measures the kernel."""
    g = load_golden("netvlad_init")
    shapes = {}
    for name in g["cases"].tolist():
        clsts, descs = g[f"{name}_clsts"], g[f"{name}_traindescs"]
        K, C = clsts.shape
        shapes[name] = (K, C, descs.shape[0])
        assert np.array_equal(g[f"{name}_centroids"], clsts) and g[f"{name}_conv_weight"].shape == (K, C, 1, 1)
        c, d = clsts.astype(np.float64), descs.astype(np.float64)
        ca = c / np.linalg.norm(c, axis=1, keepdims=True)
        dots = np.sort(ca @ d.T, axis=0)[::-1]
        alpha = -np.log(0.01) / np.mean(dots[0] - dots[1])
        assert abs(float(g[f"{name}_alpha"]) - alpha) <= 1e-5 * alpha, name
        w = g[f"{name}_conv_weight"].reshape(K, C).astype(np.float64)
        assert np.linalg.norm(w - alpha * ca) <= 1e-5 * np.linalg.norm(alpha * ca), name
    assert sorted(shapes.values()) == sorted([(64, 128, 257), (20, 128, 257), (2, 64, 1), (256, 64, 300)])
    assert (ROOT / "tests" / "golden" / "netvlad_init.npz").stat().st_size < 500 * 1024
