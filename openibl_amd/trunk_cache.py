"""Frozen-trunk cache: the pooled conv4_3 maps of a fixed image set, kept on the device.

Every `--layers conv5` training round re-extracts the descriptors of ALL training images before it mines
(`mining.update_sampler`; examples/netvlad_img.py:73-83, netvlad_img_sfrs.py:74-94).  With train_layers='conv5',
`VGG.__init__` freezes `base[:24]` — conv1_1 .. conv4_3 and the fourth max-pool — and the extraction loader applies
the deterministic test transform: the activation conv5_1 reads is the same bits in every round.  `TrunkCache.fill`
runs that part once and keeps what the backbone STORES there (oibl_vgg16_pool4_lines_forward: bf16, split bf16x3
elements, f16mx lines or fp32, written straight into one [n][h][w][512] device tensor); `cache.descriptors(model)`
then runs conv5_1 .. conv5_3 with the live parameters (oibl_vgg16_conv5_from_pool4: the whole forward's launches for
these layers) and the model's head per recorded batch.  The descriptors are BIT-EQUAL to `_extract_local` on the
loader of the fill; no image is decoded or copied inside the round loop.

    cache = TrunkCache.fill(model, train_extract_loader, dataset)             # once per run
    update_sampler(sampler, model, loader, query, gallery, sub_set, trunk_cache=cache)     # every round

Contract: the images and the transform are those of the fill (the case for the scripts' train_extract_loader); the
trunk must stay as it was (checked: `check`).  Single rank, one image size, the whole set on the device — there is no
partial cache and no host spill.  Training itself (`forward_train`) cannot use the cache: its inputs are augmented.
"""
from __future__ import annotations

import time
from typing import List, Optional, Tuple

import torch

from . import ops
from .lib import OpenIBLAmdError
from .models import _fingerprint

__all__ = ["TrunkCache"]

_TRUNK_MODULES = 24     # base[:24]: conv1_1 .. conv4_3 and the fourth max-pool (VGG._fix_layers['conv5'])
_CONV5 = (24, 26, 28)


def _trunk_params(base) -> List[torch.Tensor]:
    return [p for l in list(base.base.children())[:_TRUNK_MODULES] for p in l.parameters()]


def _core_of(model):
    from .extract import fast_path_supported, unwrap_model
    core = unwrap_model(model)
    if not fast_path_supported(core):
        raise TypeError("TrunkCache: the model must be an EmbedNet, EmbedNetPCA or EmbedRegionNet")
    return core


class TrunkCache:
    """Stored pool4 activations of `n_items` images in dataset order (see the module text).

    lines     [rows][h][w][512] device tensor of the precision's element type (rows >= n_items when the loader pads)
    batches   [(first row, images, effective precision, [(first image, images) of each pass])] of the fill: conv5 is
              run per recorded batch in the recorded arithmetic, as the full flow runs it
    precision the model's precision at fill time;  fingerprint: `models._fingerprint` of the `base[:24]` parameters
    range_fallbacks: batches whose f16mx conv5 pass raised the range flag in `descriptors` and were redone in bf16x3
              from the widened lines (within the mode's 1e-4, but not the bits of the full flow, which restarts such
              a batch from the images);  fill_range_fallbacks: batches stored as bf16x3 elements for that reason"""

    def __init__(self, lines: torch.Tensor, batches, precision: str, fingerprint, n_items: int, image_hw=None,
                 min_tiles=None):
        self.lines = lines
        self.batches = list(batches)
        self.precision = precision
        self.fingerprint = fingerprint
        self.n_items = int(n_items)
        self.image_hw = image_hw
        self.min_tiles = min_tiles
        self.range_fallbacks = 0
        self.fill_range_fallbacks = 0
        self.fill_seconds = 0.0
        self._packed = {}

    # ---- host arithmetic ------------------------------------------------------------------------
    @staticmethod
    def nbytes(n_images: int, H: int, W: int, precision) -> int:
        """Bytes of the cache of n_images H x W images: (H // 16) (W // 16) 512 elements each (floor at every pool),
        2 bytes in bf16, 4 in fp32 / bf16x3 / f16mx."""
        p = ops.precision_code(precision)
        if p == ops.F16R:
            raise ValueError("TrunkCache.nbytes: 'f16r' is a matching arithmetic, not a backbone precision")
        h, w = ops.vgg16_feature_hw(int(H), int(W))
        return int(n_images) * h * w * 512 * (2 if p == ops.BF16 else 4)

    # ---- fill -----------------------------------------------------------------------------------
    @classmethod
    def fill(cls, model, loader, dataset, gpu=None, max_bytes: Optional[int] = None,
             input_resize=None, input_decode=None) -> "TrunkCache":
        """Run `loader` (the extraction loader over `dataset`, fp32 [N][3][H][W] or uint8 [N][H][W][3] batches in
        dataset order) once, eagerly, under no_grad in eval mode, and keep every batch's stored pool4 activation.
        max_bytes: refuse (ValueError) a cache above it; default a quarter of the device's free memory now.
        input_resize: as in `extract_features` — the loader's raw uint8 batches are resized on the device first.
        input_decode: as in `extract_features` — the loader's JpegBatch batches are decoded on the device in front of
        that; RuntimeError lists the damaged files when the loader has ended.  MixedJpegBatch batches (files of mixed
        stored sizes, `jpeg.collate_mixed`) need input_resize=(height, width) and are decoded and resized in one step."""
        from .evaluators import _rank_world
        from .extract import (_batch_names, apply_input_decode, apply_input_resize, check_input_decode, input_resizer,
                              is_mixed_batch)
        from .jpeg import scan_route
        resize = input_resizer(input_resize)
        decoded = []
        rank, world = _rank_world()
        if world != 1:
            raise RuntimeError(
                f"TrunkCache.fill: the frozen-trunk cache runs on a single rank (world size {world}): the "
                "descriptors are not gathered between devices yet; use the host flow (extract_features + "
                "pairwise_distance + sampler.sort_gallery)")
        core = _core_of(model)
        base = core.base_model
        if not torch.cuda.is_available() or not all(p.is_cuda for p in base.parameters()):
            raise OpenIBLAmdError("openibl_amd: TrunkCache.fill runs only on an AMD GPU through the HIP extension "
                                  "(there is no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device() if gpu is None else gpu)
        model.eval()
        n_items = len(dataset)
        try:
            rows = max(n_items, len(loader.sampler))
        except Exception:
            rows = n_items
        prec = base.precision
        lines, hw, batches, row = None, None, [], 0
        cache = None
        t0 = time.time()
        with torch.no_grad():
            for batch in loader:
                imgs = batch[0]
                mixed = bool(input_decode) and is_mixed_batch(imgs)
                if input_decode:
                    imgs = apply_input_decode(imgs, dev, decoded, _batch_names(batch), scan=scan_route(input_decode),
                                              resize=resize)
                if not torch.is_tensor(imgs):
                    imgs = torch.as_tensor(imgs)
                if resize is not None and not mixed:
                    imgs = apply_input_resize(resize, imgs, dev)
                if imgs.dtype != torch.uint8 and imgs.dtype != torch.float32:
                    imgs = imgs.float()
                if imgs.dim() != 4:
                    raise ValueError(f"TrunkCache.fill: a batch of shape {tuple(imgs.shape)} is not a batch of images")
                x = imgs.contiguous().to(dev, non_blocking=True)
                n = int(x.shape[0])
                this_hw = (int(x.shape[1]), int(x.shape[2])) if x.dtype == torch.uint8 else \
                    (int(x.shape[2]), int(x.shape[3]))
                if lines is None:
                    hw = this_hw
                    need = cls.nbytes(rows, hw[0], hw[1], prec)
                    limit = torch.cuda.mem_get_info(dev)[0] // 4 if max_bytes is None else int(max_bytes)
                    if need > limit:
                        raise ValueError(
                            f"TrunkCache.fill: the stored pool4 maps of {rows} images of {hw[0]} x {hw[1]} take "
                            f"{need} bytes in {prec}, above the limit of {limit} bytes (max_bytes; by default a "
                            "quarter of the device's free memory): there is no partial cache and no host spill — "
                            "extract the ordinary way (update_sampler / extract_features without trunk_cache)")
                    h, w = ops.vgg16_feature_hw(*hw)
                    lines = torch.empty((rows, h, w, 512), dtype=ops.elem_dtype(prec), device=dev)
                    cache = cls(lines, [], prec, _fingerprint(_trunk_params(base)), n_items, hw,
                                base.F16MX_MIN_TILES)
                elif this_hw != hw:
                    raise ValueError(f"TrunkCache.fill: the loader yields images of {this_hw[0]} x {this_hw[1]} after "
                                     f"{hw[0]} x {hw[1]}: the cache holds one image size")
                if row + n > rows:
                    raise ValueError(f"TrunkCache.fill: the loader yields more than the {rows} images its sampler and "
                                     "dataset announce")
                batches.append(cache._fill_batch(base, x, row))
                row += n
        check_input_decode(decoded)
        if lines is None or row < n_items:
            raise ValueError(f"TrunkCache.fill: the loader yielded {row} images, the dataset holds {n_items}")
        torch.cuda.current_stream(dev).synchronize()
        cache.batches = batches
        cache.fill_seconds = time.time() - t0
        return cache

    def _fill_batch(self, base, x: torch.Tensor, row: int):
        """One batch's lines into rows [row, row + n): the arithmetic and the passes of VGG.features_nhwc."""
        n = int(x.shape[0])
        dst = self.lines[row:row + n]
        eff = base.effective_precision(x)
        ws, bs = base._packed(x.device, eff)
        if ops.precision_code(eff) != ops.F16MX:
            ops.vgg16_pool4_lines(x, ws, bs, eff, out=dst)
            return (row, n, eff, [(0, n)])
        groups = base.f16mx_groups(x)
        raised = 0
        for i0, cnt in groups:
            _, flag = ops.vgg16_pool4_lines(x[i0:i0 + cnt], ws, bs, eff, return_flag=True, out=dst[i0:i0 + cnt])
            raised |= int(flag.item())           # (a host synchronisation per pass: the fill runs once)
        if not raised:
            return (row, n, eff, groups)
        # beyond fp16 somewhere in the trunk: the batch again in bf16x3, as the model does; split elements are the
        # same size, and the batch's conv5 runs in bf16x3 from now on
        self.fill_range_fallbacks += 1
        ws, bs = base._packed(x.device, "bf16x3")
        ops.vgg16_pool4_lines(x, ws, bs, "bf16x3", out=dst)
        return (row, n, "bf16x3", [(0, n)])

    # ---- validity -------------------------------------------------------------------------------
    def check(self, model, n_items: Optional[int] = None) -> None:
        """RuntimeError unless the cache still describes `model`'s trunk: the `base[:24]` parameters are the tensors
        (storage, version counter, device) of the fill — a `load_state_dict` or an optimizer that touched the trunk
        changes them —, none of them is trainable, and the precision (and the small-batch rule) is the fill's."""
        base = _core_of(model).base_model
        trunk = _trunk_params(base)
        if any(p.requires_grad for p in trunk):
            raise RuntimeError("TrunkCache: a parameter of base[:24] (conv1_1 .. conv4_3) has requires_grad=True: the "
                               "cache is only valid while the trunk is frozen (train_layers='conv5')")
        if base.precision != self.precision:
            raise RuntimeError(f"TrunkCache: the cache was filled in precision {self.precision!r}, the model now runs "
                               f"{base.precision!r}: fill a new cache")
        if self.min_tiles is not None and base.F16MX_MIN_TILES != self.min_tiles:
            raise RuntimeError("TrunkCache: F16MX_MIN_TILES changed since the fill (the batches' arithmetic was "
                               "recorded under the old rule): fill a new cache")
        if _fingerprint(trunk) != self.fingerprint:
            raise RuntimeError("TrunkCache: the fingerprint of the base[:24] parameters changed since the fill (a "
                               "load_state_dict, a move to another device, or an optimizer that touched the trunk): "
                               "fill a new cache")
        if n_items is not None and int(n_items) != self.n_items:
            raise RuntimeError(f"TrunkCache: the cache holds {self.n_items} images, the dataset {int(n_items)}")

    # ---- conv5 weights --------------------------------------------------------------------------
    def _conv5_packed(self, base, precision: str):
        """(packed conv5 weights, biases) in `precision`, re-packed only when the six tensors' fingerprint (or the
        module's cache generation: `invalidate()`) changes, as VGG._packed does for the whole backbone."""
        convs = [base.base[i] for i in _CONV5]
        key = (_fingerprint([c.weight for c in convs] + [c.bias for c in convs]), getattr(base, "_cache_gen", 0))
        if self._packed.get("key") != key:
            self._packed = {"key": key}
        hit = self._packed.get(precision)
        if hit is None:
            ws = [ops.pack_conv3x3(c.weight.detach().float().contiguous(), precision) for c in convs]
            bs = [c.bias.detach().float().contiguous() for c in convs]
            hit = self._packed[precision] = (ws, bs)
        return hit

    # ---- descriptors ----------------------------------------------------------------------------
    def descriptors(self, model, vlad: bool = True, store_dtype=None, pca=None) -> torch.Tensor:
        """[n_items][d] descriptors on the device (float32, or `store_dtype`), what `_extract_local(model, loader,
        vlad, pca, ...)[:n_items]` returns on the loader of the fill — bit-equal — from the cached lines: per recorded
        batch conv5_1 .. conv5_3 with the LIVE parameters, then the model's head (NetVLAD + norms or the global
        max-pool, `ops.l2_normalize`, `pca.infer`, `ops.store_descriptors`).  The lines are read in place.  The f16mx
        range flags of the conv5 passes are read once, behind the last batch; a flagged batch is redone in bf16x3 from
        its widened lines (`range_fallbacks`)."""
        from .extract import _head_fn
        core = _core_of(model)
        self.check(core)
        if not torch.is_tensor(self.lines) or not self.lines.is_cuda:
            raise OpenIBLAmdError("openibl_amd: TrunkCache.descriptors runs only on an AMD GPU through the HIP "
                                  "extension (there is no CPU fallback)")
        model.eval()
        if pca is not None:
            pca.load(gpu=self.lines.device.index)
        base = core.base_model
        dev = self.lines.device
        head = _head_fn(core, vlad, pca, store_dtype)
        rows = self.batches[-1][0] + self.batches[-1][1] if self.batches else 0
        final, flags = None, None
        with torch.no_grad():
            for b, (row, n, prec, groups) in enumerate(self.batches):
                ws, bs = self._conv5_packed(base, prec)
                src = self.lines[row:row + n]
                if ops.precision_code(prec) != ops.F16MX:
                    feat = ops.vgg16_conv5_from_pool4(src, ws, bs, prec)
                else:
                    if flags is None:
                        flags = torch.zeros(len(self.batches), dtype=torch.int32, device=dev)
                    if len(groups) == 1:
                        feat, flag = ops.vgg16_conv5_from_pool4(src, ws, bs, prec, return_flag=True)
                        flags[b:b + 1].bitwise_or_(flag)
                    else:
                        feat = torch.empty(tuple(src.shape), dtype=torch.float32, device=dev)
                        for i0, cnt in groups:
                            _, flag = ops.vgg16_conv5_from_pool4(src[i0:i0 + cnt], ws, bs, prec, return_flag=True,
                                                                 out=feat[i0:i0 + cnt])
                            flags[b:b + 1].bitwise_or_(flag)
                out = head(feat)
                if final is None:
                    final = torch.empty((rows, int(out.shape[1])), dtype=out.dtype, device=dev)
                final[row:row + n].copy_(out)
            if flags is not None:
                for b in torch.nonzero(flags.cpu()).flatten().tolist():      # the one synchronisation
                    row, n, prec, _ = self.batches[b]
                    self.range_fallbacks += 1
                    ws, bs = self._conv5_packed(base, "bf16x3")
                    wide = ops.x3_split(ops.widen_pool4_lines(self.lines[row:row + n], prec))
                    final[row:row + n].copy_(head(ops.vgg16_conv5_from_pool4(wide, ws, bs, "bf16x3")))
        if final is None:
            return torch.empty((0, 0), device=dev)
        return final[:self.n_items]
