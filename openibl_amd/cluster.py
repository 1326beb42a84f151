"""NetVLAD centroid initialisation: the k-means of the reference's examples/cluster.py:110-115,

    kmeans = KMeans(n_clusters=args.num_clusters, max_iter=niter, random_state=args.seed).fit(dbFeat[...])
    centroids = kmeans.cluster_centers_

with the Lloyd iterations on the GPU.  What scikit-learn's `KMeans.fit` does for a dense float32
matrix (sklearn/cluster/_kmeans.py: `fit`, `_kmeans_single_lloyd`, `_tolerance`) is restated step by
step:

  * tolerance   tol_abs = mean(var(X, axis=0)) * 1e-4
  * centring    X -= X.mean(axis=0)  (the mean is added back to the centres at the end)
  * seeding     k-means++ with `RandomState(seed)`.  The seeding IS scikit-learn's: its candidate draws
                come out of its own RNG stream and decide everything that follows, so the public
                `sklearn.cluster.kmeans_plusplus` is called on the centred matrix — the same function
                `KMeans.fit` reaches through `_init_centroids` — instead of imitating it.  (The
                reference imports scikit-learn for this step anyway.)
  * one run (n_init = 'auto' = 1 for k-means++) of Lloyd: assign every point to its nearest centre
    (`oibl_sqdist_topk`, k = 1, exact-fp32 mode, ties to the lowest index as `argmin` does), move
    every centre to the mean of its points (`oibl_cluster_means`), relocate empty clusters to the
    points farthest from their centres, stop when the labels repeat or the summed squared centre
    shift is <= tol_abs, at most `max_iter` times.

scikit-learn accumulates the means in float32 in thread-dependent chunks; here they are correctly
rounded, so centres agree to ~1e-6 relative, not bit for bit (tests/golden/kmeans.npz, produced by
the reference's own call).  `assign_fn` / `update_fn` are injection points for the CPU tests.

Around the k-means, the rest of the reference's initialisation flow (README "Initialising NetVLAD without a
checkpoint"):

  * `sample_positions` / `sample_local_descriptors`   examples/cluster.py:93-104: 100 random positions of the
    channel-normalised conv5 map per image (`oibl_local_descriptors` reads only those), with numpy's draws in
    the reference's order — the same seed picks the same positions;
  * `build_init_cache` / `load_init_cache`            the `<arch>_<dataset>_<K>_desc_cen.hdf5` file (datasets
    `descriptors`, `centroids`) that carries both to the training scripts;
  * `netvlad_init`                                    ibl/models/netvlad.py:34-42: alpha, centroids and the
    assignment weights from the centres and the descriptors (`oibl_assign_gap`); `NetVLAD._init_params()` is
    this function plus the three writes.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, Optional, Tuple

import numpy as np

__all__ = ["kmeans_centroids", "sample_positions", "sample_local_descriptors", "netvlad_init",
           "build_init_cache", "load_init_cache"]


def _hip_assign(x_dev, centers: np.ndarray):
    import torch
    from . import ops
    c = torch.from_numpy(centers).to(x_dev.device)
    _, idx = ops.sqdist_topk(x_dev, c, 1, precision="fp32")
    return idx.reshape(-1).contiguous()


def _hip_update(x_dev, labels_dev, centers: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    import torch
    from . import ops
    c = torch.from_numpy(centers).to(x_dev.device).contiguous()
    counts = ops.cluster_means(x_dev, labels_dev, c)
    return c.cpu().numpy(), counts.cpu().numpy()


def _relocate_empty(x: np.ndarray, labels: np.ndarray, centers_old: np.ndarray, centers_new: np.ndarray,
                    counts: np.ndarray) -> None:
    """sklearn/cluster/_k_means_common.pyx `_relocate_empty_clusters_dense`, on the means instead of
    the sums: an empty cluster takes the point farthest from its own centre, that point leaves the
    sum of the cluster it was counted in (its label does not change in this iteration)."""
    empty = np.where(counts == 0)[0]
    if not len(empty):
        return
    dist = ((x - centers_old[labels]) ** 2).sum(axis=1)
    far = np.argpartition(dist, -len(empty))[:-len(empty) - 1:-1]
    sums = centers_new.astype(np.float64) * counts[:, None]
    w = counts.astype(np.float64)
    for new_id, i in zip(empty, far):
        old_id = labels[i]
        sums[old_id] -= x[i]
        sums[new_id] = x[i]
        w[new_id] = 1.0
        w[old_id] -= 1.0
    for c in set(empty.tolist()) | set(labels[far].tolist()):
        if w[c] > 0:
            centers_new[c] = (sums[c] / w[c]).astype(np.float32)
    counts[:] = w.astype(counts.dtype)


def kmeans_centroids(descriptors, num_clusters: int = 64, max_iter: int = 100, seed: int = 43, tol: float = 1e-4,
                     device=None, assign_fn: Optional[Callable] = None, update_fn: Optional[Callable] = None,
                     return_n_iter: bool = False):
    """`KMeans(n_clusters=num_clusters, max_iter=max_iter, random_state=seed).fit(X).cluster_centers_`
    for a dense float32 matrix X [n][d] (numpy or torch).  Returns float32 [num_clusters][d]."""
    from sklearn.cluster import kmeans_plusplus     # the reference's own dependency (cluster.py:13)
    import torch
    x = np.array(descriptors.detach().cpu().numpy() if torch.is_tensor(descriptors) else descriptors,
                 dtype=np.float32, order="C", copy=True)
    if x.ndim != 2 or x.shape[0] < num_clusters:
        raise ValueError(f"n_samples={x.shape[0] if x.ndim == 2 else '?'} should be >= n_clusters={num_clusters}.")
    tol_abs = float(np.mean(np.var(x, axis=0)) * tol)
    x_mean = x.mean(axis=0)
    x -= x_mean
    sq = np.einsum("ij,ij->i", x, x)
    centers, _ = kmeans_plusplus(x, num_clusters, x_squared_norms=sq, random_state=np.random.RandomState(seed))
    centers = np.ascontiguousarray(centers, dtype=np.float32)
    if assign_fn is None or update_fn is None:
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        x_work = torch.from_numpy(x).to(dev)
        assign_fn, update_fn = assign_fn or _hip_assign, update_fn or _hip_update
    else:
        x_work = x
    labels_old = None
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        labels_dev = assign_fn(x_work, centers)
        centers_new, counts = update_fn(x_work, labels_dev, centers)
        labels = labels_dev.cpu().numpy() if torch.is_tensor(labels_dev) else np.asarray(labels_dev)
        labels = labels.astype(np.int64, copy=False)
        if (counts == 0).any():
            _relocate_empty(x, labels, centers, centers_new, counts)
        shift = float(((centers_new.astype(np.float64) - centers.astype(np.float64)) ** 2).sum())
        centers = centers_new
        if labels_old is not None and np.array_equal(labels, labels_old):
            break                                   # strict convergence
        if shift <= tol_abs:
            break
        labels_old = labels
    out = (centers + x_mean).astype(np.float32)
    return (out, n_iter) if return_n_iter else out


# ---- local descriptors (examples/cluster.py:93-104) ------------------------------------------------------------
def sample_positions(n_images: int, P: int, n_per_image: int, rng=np.random) -> np.ndarray:
    """int64 [n_images][n_per_image]: `rng.choice(P, n_per_image, replace=False)` once per image, in image order —
    the draws of examples/cluster.py:100-102, so the same seed picks the same positions.  n_per_image > P raises
    ValueError, as numpy does."""
    if n_per_image > P:
        raise ValueError(f"Cannot take a larger sample ({n_per_image}) than population ({P}) when 'replace=False'")
    out = np.empty((int(n_images), int(n_per_image)), dtype=np.int64)
    for i in range(int(n_images)):
        out[i] = rng.choice(P, n_per_image, replace=False)
    return out


def _hip_gather(feat, positions):
    from . import ops
    return ops.local_descriptors(feat, positions)


def sample_local_descriptors(model, batches: Iterable, n_descriptors: int = 50000, n_per_image: int = 100,
                             rng=np.random, gather_fn: Optional[Callable] = None):
    """The `descriptors` dataset of examples/cluster.py: float32 device tensor [n_descriptors][C], rows
    batchix + ix * n_per_image .. + n_per_image of it the sampled, L2-normalised conv5 descriptors of image ix of
    a batch.  `model` is a VGG or anything with a `base_model`; `batches` yields image tensors or the reference
    loader's 5-tuples (image first).  Each batch goes through `features_nhwc` — no NCHW copy of the map, and only
    the sampled pixels are normalised — with the f16mx range flag settled behind the gather (a flagged batch is
    gathered again from its bf16x3 map, as models._with_range_guard does).  ceil(n_descriptors / n_per_image)
    images are used; a RuntimeError says so when `batches` ends before that.  `gather_fn(feat, positions)` is the
    injection point of the CPU tests."""
    import torch
    base = getattr(model, "base_model", model)
    gather = gather_fn or _hip_gather
    n_images = math.ceil(n_descriptors / n_per_image)
    params = list(base.parameters()) if hasattr(base, "parameters") else []
    dev = params[0].device if params else None
    out, done = None, 0                       # images done
    for batch in batches:
        if done >= n_images:
            break
        x = batch[0] if isinstance(batch, (tuple, list)) else batch
        x = x[: n_images - done]
        if dev is not None:
            x = x.to(dev)
        feat = base.features_nhwc(x, defer_flag=True)
        P = feat.numel() // (int(feat.shape[0]) * int(feat.shape[-1]))
        pos = sample_positions(int(feat.shape[0]), P, n_per_image, rng)
        rows = gather(feat, pos)
        fb = base.settle_range_flag(x)
        if fb is not None:
            rows = gather(fb, pos)
        if out is None:
            out = torch.empty((n_descriptors, int(rows.shape[1])), dtype=torch.float32, device=rows.device)
        start = done * n_per_image
        take = min(int(rows.shape[0]), n_descriptors - start)
        out[start:start + take] = rows[:take]
        done += int(feat.shape[0])
    if done < n_images:
        raise RuntimeError(f"sample_local_descriptors: {n_descriptors} descriptors at {n_per_image} per image need "
                           f"{n_images} images, the batches held {done}")
    return out


# ---- NetVLAD._init_params (ibl/models/netvlad.py:34-42) --------------------------------------------------------
def netvlad_init(clsts, traindescs, device=None):
    """(alpha, centroids [K][C], conv_weight [K][C][1][1]) from the k-means centres `clsts` [K][C] and the training
    descriptors `traindescs` [n][C] (numpy or torch): clsts_assign = clsts / |clsts|, per descriptor the gap between
    its best and second-best product with clsts_assign (`ops.assign_gap`), alpha = -log(0.01) / mean gap in float64
    on the host, centroids = clsts, conv_weight = alpha * clsts_assign.  Tensors are float32 on the device."""
    import torch
    from . import ops

    def to_dev(a):
        t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        dev = device
        if dev is None:
            dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return t.to(device=dev, dtype=torch.float32).contiguous()

    if not torch.cuda.is_available():
        from .lib import OpenIBLAmdError
        raise OpenIBLAmdError("openibl_amd: netvlad_init runs only on an AMD GPU through the HIP extension "
                              "(there is no CPU fallback)")
    c, d = to_dev(clsts), to_dev(traindescs)
    if c.dim() != 2 or d.dim() != 2 or c.shape[1] != d.shape[1]:
        raise ValueError(f"netvlad_init: clsts [K][C] and traindescs [n][C], got {tuple(c.shape)} and {tuple(d.shape)}")
    if d.device != c.device:
        d = d.to(c.device)
    clsts_assign, _, mean_gap = ops.assign_gap(d, c)
    alpha = float(-np.log(0.01) / np.float64(mean_gap))
    conv_weight = (clsts_assign * alpha).reshape(c.shape[0], c.shape[1], 1, 1)
    return alpha, c, conv_weight


# ---- the cache file between the two (examples/cluster.py:84-115, netvlad_img.py:90-95) -------------------------
def build_init_cache(model, batches: Iterable, path: str, num_clusters: int = 64, seed: int = 43,
                     max_iter: int = 100, n_descriptors: int = 50000, n_per_image: int = 100, rng=np.random,
                     gather_fn: Optional[Callable] = None, **kmeans_kwargs) -> str:
    """examples/cluster.py's main: sample the local descriptors, run `kmeans_centroids` on them and write the cache
    file `path` (the reference names it <arch>_<dataset>_<K>_desc_cen.hdf5) with the datasets `descriptors`
    [n_descriptors][C] and `centroids` [num_clusters][C].  HDF5 when h5py is importable, else an npz archive at the
    same path (the convention of openibl_amd.pca); `load_init_cache` reads both.  Returns the path."""
    from .pca import _write_arrays
    descs = sample_local_descriptors(model, batches, n_descriptors, n_per_image, rng=rng, gather_fn=gather_fn)
    centroids = kmeans_centroids(descs, num_clusters=num_clusters, max_iter=max_iter, seed=seed, **kmeans_kwargs)
    return _write_arrays(path, descriptors=descs.detach().cpu().numpy(), centroids=centroids)


def load_init_cache(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(clsts, traindescs) = the `centroids` and `descriptors` datasets of a cache file, as the reference's
    scripts read them (examples/netvlad_img.py:93-95):
        model.net_vlad.clsts, model.net_vlad.traindescs = load_init_cache(path); model._init_params()"""
    from .pca import _read_arrays
    descs, cents = _read_arrays(path, ("descriptors", "centroids"), what="load_init_cache")
    return np.asarray(cents, dtype=np.float32), np.asarray(descs, dtype=np.float32)
