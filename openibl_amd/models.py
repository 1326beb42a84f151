"""nn.Module mirror of the reference's model zoo (ibl/models/{vgg,netvlad,__init__}.py).

Same class names, constructor arguments, return conventions and — because `base` is a real
nn.Sequential of the same 29 modules and NetVLAD / pca_layer hold the same parameters —
bit-for-bit the same `state_dict()` keys and shapes, so the released `vgg16_netvlad.pth` and
DDP-saved (`module.`-prefixed) checkpoints load unchanged.  The modules only *own* the parameters;
`forward` never calls them.  It hands raw device pointers to the HIP kernels via openibl_amd.ops:

    VGG.forward          -> oibl_vgg16_conv5_forward      (vgg.py:61-70)
    NetVLAD.forward      -> oibl_netvlad_forward           (netvlad.py:44-61)
    EmbedNet.forward     -> backbone + NetVLAD + norms      (netvlad.py:73-82)
    EmbedNetPCA.forward  -> ... + oibl_pca_forward           (netvlad.py:95-110)

Inference, plus the differentiable part of the reference's default training setting: `EmbedNet.forward_train` carries an
autograd graph to the NetVLAD layer and, with train_layers='conv5', to conv5_1 .. conv5_3 (oibl_netvlad_backward,
oibl_conv3x3_backward); the training loops and their fused losses are ibl.trainers (`NetVLAD._init_params`, the gradient-free
initialisation from k-means centres, is here too: oibl_assign_gap).  Inputs must be CUDA(HIP)
tensors; there is no CPU path.
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import ops

__all__ = ["VGG", "vgg16", "NetVLAD", "EmbedNet", "EmbedNetPCA", "EmbedRegionNet", "names",
           "create", "default_precision"]

_CFG_D = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


def default_precision() -> str:
    """The arithmetic a model runs in when nobody chose one: 'f16mx' (fp16 main term + MX-fp6 cross terms on the
    gfx950 matrix cores: descriptors within north_star's 1e-4 of the reference's fp32 result, range-guarded, 4x the
    rate of exact fp32) — what `torch.hub.load(..., 'vgg16_netvlad')(x)` and an unmodified examples/test.py get
    since round 6.  `OPENIBL_AMD_PRECISION` or `model.set_precision(...)` select 'fp32' (exact fp32 MFMA:
    reference-grade numerics, 8e-7), 'bf16x3' (split bf16: 4e-6 at 3x the bf16 matrix work) or 'bf16' (3e-3: not a
    parity mode)."""
    return os.environ.get("OPENIBL_AMD_PRECISION", "f16mx").lower()


class _PrecisionMixin:
    """`module.set_precision('bf16' | 'f16mx' | 'bf16x3' | 'fp32')` switches the arithmetic of the contractions."""

    def set_precision(self, precision: str):
        ops.precision_code(precision)
        for m in self.modules():
            if isinstance(m, _PrecisionMixin):
                m._precision = precision.lower()
                m._drop_cache()
        return self

    def _drop_cache(self):
        """Forget the packed / cast parameter copies and advance the cache generation: captured forwards
        kept for the model (extract._graph_store) point into those copies and are keyed on the generation."""
        self._cache = {}
        self._cache_gen = getattr(self, "_cache_gen", 0) + 1

    @property
    def precision(self) -> str:
        return getattr(self, "_precision", None) or default_precision()

    def invalidate(self):
        """Drop every packed / cast copy of the parameters (they are rebuilt by the next forward).
        The caches are keyed on (data_ptr, _version, device) of the parameters, which catches
        `load_state_dict`, `.to()` and in-place autograd-visible updates, but NOT writes through
        `param.data` (`p.data.copy_(...)`, the idiom of the reference's NetVLAD._init_params,
        ibl/models/netvlad.py:34-42): call this after such an update.  A GraphedDescriptor froze
        its copies at capture time and has to be re-created."""
        for m in self.modules():
            if isinstance(m, _PrecisionMixin):
                m._drop_cache()
        return self

    def _hook_state_dict_loads(self):
        # load_state_dict copies through param.data as well on some paths: always start clean
        def _drop(module, incompatible_keys):   # (a post hook must return None)
            module.invalidate()
        self.register_load_state_dict_post_hook(_drop)


def _fingerprint(params: List[torch.Tensor]) -> Tuple:
    return tuple((p.data_ptr(), p._version, str(p.device)) for p in params)


class VGG(_PrecisionMixin, nn.Module):
    """VGG16 cfg-D up to conv5_3 without the last ReLU / pool (ibl/models/vgg.py:15-70)."""

    _fix_layers = {"conv5": 24, "conv4": 17, "conv3": 10, "conv2": 5, "full": 0}

    def __init__(self, depth, pretrained=True, cut_at_pooling=False, train_layers="conv5",
                 matconvnet=None):
        super().__init__()
        if depth != 16:
            raise KeyError("Unsupported depth:", depth)
        self.pretrained = pretrained
        self.depth = depth
        self.cut_at_pooling = cut_at_pooling
        self.train_layers = train_layers
        self.feature_dim = 512
        self.matconvnet = matconvnet
        layers, cin = [], 3
        for v in _CFG_D:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.base = nn.Sequential(*layers[:-2])   # drop the last ReLU and max-pool (vgg.py:41-42)
        self.gap = nn.AdaptiveMaxPool2d(1)
        self._cache: Dict = {}
        self.range_fallbacks = 0           # batches recomputed in bf16x3 because f16mx met a value beyond fp16
        self.precision_runs: Dict = {}     # effective precision -> backbone passes run in it
        self._hook_state_dict_loads()
        self._init_params()
        if not pretrained:
            self.reset_params()
        else:
            if matconvnet is None:
                warnings.warn("openibl_amd: ImageNet weights for vgg16 cannot be downloaded here; "
                              "the backbone is randomly initialised until a checkpoint is loaded")
                self.reset_params()
            for l in list(self.base.children())[: VGG._fix_layers[train_layers]]:
                for p in l.parameters():
                    p.requires_grad = False

    def _init_params(self):
        if self.matconvnet is not None:
            self.base.load_state_dict(torch.load(self.matconvnet))
            self.pretrained = True

    def reset_params(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out")
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ---- HIP path ---------------------------------------------------------------------------
    def _convs(self) -> List[nn.Conv2d]:
        return [m for m in self.base if isinstance(m, nn.Conv2d)]

    # Rounds 1-3 ran f16mx batches whose conv4 layers gave fewer than 256 ring tiles in bf16x3 (every Tokyo 24/7
    # query, every ragged last batch).  Since round 4 the f16mx ring kernels split K for layers that would leave
    # the chip idle (csrc/conv.hip, mx_split_plan) and a single 480x640 image runs f16mx in 0.82 ms (bf16x3:
    # 0.95).  Below 8 tiles of 256 conv4 pixels (one image of 320x320, two of 224x224) the split layers' extra
    # launches cost what the cheaper products save and bf16x3 — the other 1e-4 mode, three times as exact — is as
    # fast or faster (profiles/r04_l_small_sizes.md: 0.49 against 0.51 ms at 224x224, 0.44 against 0.49 at
    # 128x160; from 9 tiles on f16mx wins by 7 % and more), so THAT is what such a batch runs in.  In ring tiles
    # (256 pixels x 256 of the 512 channels): 16.  A knob: 0 = f16mx whenever it can run (the kernel tests),
    # 256 = rounds 1-3.
    F16MX_MIN_TILES = 16

    def effective_precision(self, x: torch.Tensor) -> str:
        """The arithmetic the backbone runs this input in: the module's precision, except for f16mx batches of fewer
        than F16MX_MIN_TILES conv4 ring tiles (where it is the slower of the two 1e-4 modes) and single images beyond
        the 32-bit offsets of the f16mx kernels, which run in bf16x3.  (A BATCH beyond those offsets — 95 images of
        480x640 and more — runs f16mx in image groups since round 6: `f16mx_groups`.)  `precision_runs` counts what
        actually ran."""
        p = self.precision
        if ops.precision_code(p) != ops.F16MX:
            return p
        n = int(x.shape[0])
        h, w = (int(x.shape[1]), int(x.shape[2])) if x.dtype == torch.uint8 else (int(x.shape[2]), int(x.shape[3]))
        tiles = -(-(n * (h // 8) * (w // 8)) // 256) * 2
        if self._f16mx_group(h, w) < 1:
            return "bf16x3"
        return p if tiles >= self.F16MX_MIN_TILES else "bf16x3"

    @staticmethod
    def _f16mx_group(h: int, w: int) -> int:
        """Images of h x w one f16mx pass takes: its kernels address their input through 32-bit buffer offsets and have
        no other implementation — the largest activation they read (conv2_2's input, [N][H/2][W/2][128] 4-byte
        elements: 39 MB per 480x640 image) and the stem's fp32 input must stay below 3.5 GB (vgg16_f16mx_fits in
        csrc/vgg.hip is the same test; the C entry point refuses what this lets through): 94 images of 480x640."""
        per = max(3 * h * w * 4, (h // 2) * (w // 2) * 128 * 4, 1)
        return (0xE0000000 - 1) // per

    def f16mx_groups(self, x: torch.Tensor):
        """[(first image, images)] of the passes an f16mx batch is run in: one, unless the batch is beyond the 32-bit
        offsets of the kernels — then equal groups of at most `_f16mx_group` images (128 x 480x640: 2 x 64), each a
        pass of its own into its rows of the feature map, instead of the silent bf16x3 run of rounds 1-5."""
        n = int(x.shape[0])
        h, w = (int(x.shape[1]), int(x.shape[2])) if x.dtype == torch.uint8 else (int(x.shape[2]), int(x.shape[3]))
        cap = max(1, self._f16mx_group(h, w))
        parts = -(-n // cap)
        per = -(-n // parts)
        return [(i, min(per, n - i)) for i in range(0, n, per)]

    def _packed(self, device: torch.device, precision: str = None):
        precision = precision or self.precision
        convs = self._convs()
        params = [c.weight for c in convs] + [c.bias for c in convs]
        if params[0].device != device:
            raise RuntimeError(f"VGG: parameters are on {params[0].device}, input on {device}")
        key = _fingerprint(params)
        if self._cache.get("packed_key") != key:      # weights changed: every precision's packing is stale
            self._cache["packed_key"] = key
            self._cache["packed"] = {}
        hit = self._cache["packed"].get(precision)
        if hit is None:
            ws = [convs[0].weight.detach().float().contiguous()]
            ws += [ops.pack_conv3x3(c.weight.detach().float().contiguous(), precision) for c in convs[1:]]
            bs = [c.bias.detach().float().contiguous() for c in convs]
            hit = self._cache["packed"][precision] = (ws, bs)
        return hit

    def features_nhwc(self, x: torch.Tensor, defer_flag: bool = False) -> torch.Tensor:
        """[N][3][H][W] fp32 (normalised) or [N][H][W][3] uint8 (raw image; the loader's
        ToTensor + Normalize run inside the first kernel) -> conv5_3 map [N][h][w][512] in the
        precision's element type.

        f16mx range guard: the fp16 main term of f16mx exists only for |activation| <= 65504 (x 8: the backbone
        stores its activations times 2^-3).  The kernels raise a device flag when a layer's output is beyond that
        (include/openibl_amd.h, OIBL_F16MX) and a flagged batch is recomputed in bf16x3, the other mode inside the
        1e-4 tolerance, which has no range limit (`range_fallbacks` counts them).  WHERE the flag is read:
          * defer_flag=False (a bare call): here, one 4-byte copy — a host synchronisation behind the backbone;
          * defer_flag=True: not here.  The caller enqueues whatever consumes the map first and then calls
            `settle_range_flag(x)` (the models' forwards do: ONE synchronisation at the end of the whole forward,
            where the caller's `.cpu()` would wait anyway — round 6), or ships
            `last_range_flag()` to a pinned word and settles batches later (extract.EagerLanes, GraphedForward);
          * under a hipGraph capture nothing can be read: the capturer takes `last_range_flag()` and checks it
            after every replay (extract.GraphedForward does).
        `_range_flag` is per-module state of the LAST call: one thread and one stream per model object at a time."""
        if x.dtype != torch.uint8 and x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        prec = self.effective_precision(x)
        ws, bs = self._packed(x.device, prec)
        ev = getattr(self, "profile_events", None)
        self.precision_runs[prec] = self.precision_runs.get(prec, 0) + 1
        if ops.precision_code(prec) != ops.F16MX:
            self._range_flag = None
            return ops.vgg16_conv5(x, ws, bs, prec, events=ev)
        groups = self.f16mx_groups(x)
        if len(groups) == 1:
            feat, flag = ops.vgg16_conv5(x, ws, bs, prec, events=ev, return_flag=True)
        else:
            # a batch beyond the kernels' 32-bit offsets: image groups, each pass into its rows of one map; every
            # pass clears the workspace's flag word when it starts, so the groups' flags are OR-ed into one
            h, w = ops.vgg16_feature_hw(*((x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[2], x.shape[3])))
            feat = torch.empty((int(x.shape[0]), h, w, 512), dtype=torch.float32, device=x.device)
            flag = torch.zeros(1, dtype=torch.int32, device=x.device)
            for i0, cnt in groups:
                _, f = ops.vgg16_conv5(x[i0:i0 + cnt], ws, bs, prec, return_flag=True, out=feat[i0:i0 + cnt])
                flag.bitwise_or_(f)
            self.precision_runs["f16mx(groups)"] = self.precision_runs.get("f16mx(groups)", 0) + len(groups)
        self._range_flag = flag
        if defer_flag or torch.cuda.is_current_stream_capturing():
            return feat
        fb = self.settle_range_flag(x)
        return feat if fb is None else fb

    def settle_range_flag(self, x: torch.Tensor) -> Optional[torch.Tensor]:
        """Read the range flag of the last `features_nhwc(x, defer_flag=True)` pass (a host synchronisation with the
        stream): None when the f16mx map stands, else the batch's map recomputed in bf16x3 — whatever was computed
        from the flagged map has to be recomputed from this one."""
        flag = getattr(self, "_range_flag", None)
        if flag is None or int(flag.item()) == 0:
            return None
        self.range_fallbacks += 1
        if x.dtype != torch.uint8 and x.dtype != torch.float32:
            x = x.float()
        return self.features_fallback(x.contiguous())

    def last_range_flag(self) -> Optional[torch.Tensor]:
        """The f16mx range flag of the last `features_nhwc` call (int32 [1] view of the first word of that
        stream's backbone workspace, rewritten by every later pass on the stream), None if that call did not
        run in f16mx."""
        return getattr(self, "_range_flag", None)

    def features_fallback(self, x: torch.Tensor) -> torch.Tensor:
        """The conv5_3 map of a batch whose f16mx pass raised the range flag: the same network in bf16x3."""
        ws, bs = self._packed(x.device, "bf16x3")
        self.precision_runs["bf16x3(range)"] = self.precision_runs.get("bf16x3(range)", 0) + 1
        return ops.vgg16_conv5(x.contiguous(), ws, bs, "bf16x3")

    def features_train_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        """The conv5_3 map [N][h][w][512] fp32 with an autograd graph to conv5_1, conv5_2 and conv5_3 (`base[24]`,
        `base[26]`, `base[28]`: the reference's --layers conv5, ibl/models/vgg.py:20-26, 50-53).  The trunk up to the
        fourth max-pool is FROZEN: it runs under no_grad in the model's effective precision (ops.vgg16_pool4); an
        f16mx range flag is read — a host synchronisation — before the graph is built, and a flagged batch (or one
        beyond the f16mx kernels' 32-bit offsets) is redone in bf16x3.  The three conv5 layers then run in exact fp32
        on their LIVE parameters (ops.conv3x3_train), whatever the model's precision: their gradients are fp32
        kernels.  A parameter with requires_grad=False gets no gradient and its stage is not launched."""
        if x.dtype != torch.float32:
            x = x.float()
        x = x.contiguous()
        prec = self.effective_precision(x)
        if ops.precision_code(prec) == ops.F16MX and len(self.f16mx_groups(x)) > 1:
            prec = "bf16x3"
        with torch.no_grad():
            ws, bs = self._packed(x.device, prec)
            self.precision_runs[prec] = self.precision_runs.get(prec, 0) + 1
            pool4, flag = ops.vgg16_pool4(x, ws, bs, prec, return_flag=True)
            if flag is not None and int(flag.item()) != 0:
                self.range_fallbacks += 1
                self.precision_runs["bf16x3(range)"] = self.precision_runs.get("bf16x3(range)", 0) + 1
                ws, bs = self._packed(x.device, "bf16x3")
                pool4 = ops.vgg16_pool4(x, ws, bs, "bf16x3")
        self._range_flag = None
        feat = pool4
        for i in (24, 26, 28):
            conv = self.base[i]
            feat = ops.conv3x3_train(feat, conv.weight, conv.bias, relu=i != 28)
        return feat

    def _outputs(self, feat):
        x_nchw = ops.nhwc_to_nchw_f32(feat)
        if self.cut_at_pooling:
            return x_nchw
        return ops.global_maxpool_nhwc(feat), x_nchw

    @torch.no_grad()
    def forward(self, x):
        return _with_range_guard(self, x, self._outputs)


def _with_range_guard(base: "VGG", x: torch.Tensor, head):
    """head(conv5_3 map) with the f16mx range flag settled BEHIND the head's launches: the device never waits for
    the host inside a forward, and the one synchronisation sits where the caller's first read of the result would
    wait anyway.  A flagged batch (rare: DESIGN §4.1a) has map and head recomputed in bf16x3."""
    out = head(base.features_nhwc(x, defer_flag=True))
    if torch.cuda.is_current_stream_capturing():
        return out
    fb = base.settle_range_flag(x)
    return out if fb is None else head(fb)


def vgg16(**kwargs):
    return VGG(16, **kwargs)


class NetVLAD(_PrecisionMixin, nn.Module):
    """NetVLAD layer (ibl/models/netvlad.py:8-61); forward returns the UN-normalised [N][K][C]."""

    def __init__(self, num_clusters=64, dim=512, alpha=100.0, normalize_input=True):
        super().__init__()
        self.num_clusters = num_clusters
        self.dim = dim
        self.alpha = alpha
        self.normalize_input = normalize_input
        self.conv = nn.Conv2d(dim, num_clusters, kernel_size=(1, 1), bias=False)
        self.centroids = nn.Parameter(torch.rand(num_clusters, dim), requires_grad=True)
        self.clsts = None
        self.traindescs = None
        self._cache: Dict = {}
        self._hook_state_dict_loads()

    def _init_params(self):
        """ibl/models/netvlad.py:34-42: alpha, centroids and conv.weight from the k-means centres `self.clsts`
        [K][C] and the training descriptors `self.traindescs` [n][C] (numpy arrays or tensors; see
        openibl_amd.cluster for where they come from).  The arithmetic runs on the HIP device — the module's own
        if its parameters are there, else the current one: the reference's scripts call this before .cuda() —
        and the results are written through `.data.copy_` as the reference does; the packed parameter copies
        and captured forwards are told (invalidate())."""
        for name in ("clsts", "traindescs"):
            if getattr(self, name) is None:
                raise ValueError(f"NetVLAD._init_params: `{name}` is not set (the k-means centres and the sampled "
                                 f"training descriptors: openibl_amd.cluster.load_init_cache)")
        if tuple(self.clsts.shape) != (self.num_clusters, self.dim):
            raise ValueError(f"NetVLAD._init_params: clsts is {tuple(self.clsts.shape)}, the layer holds "
                             f"{self.num_clusters} clusters of dimension {self.dim}")
        if not torch.cuda.is_available():
            raise ops._lib.OpenIBLAmdError("openibl_amd: NetVLAD._init_params runs only on an AMD GPU through the "
                                           "HIP extension (there is no CPU fallback)")
        from .cluster import netvlad_init
        own = self.centroids.device
        dev = own if own.type == "cuda" else torch.device("cuda", torch.cuda.current_device())
        alpha, centroids, conv_weight = netvlad_init(self.clsts, self.traindescs, device=dev)
        self.alpha = alpha
        self.centroids.data.copy_(centroids)
        self.conv.weight.data.copy_(conv_weight)
        self.invalidate()

    def _params(self):
        w = self.conv.weight.detach().float().reshape(self.num_clusters, self.dim).contiguous()
        return w, self.centroids.detach().float().contiguous()

    def aggregate_nhwc(self, feat: torch.Tensor, want_raw: bool, want_norm: bool):
        w, c = self._params()
        return ops.netvlad(feat, w, c, self.normalize_input, want_raw=want_raw, want_norm=want_norm)

    def head_with_grad(self, feat_nhwc: torch.Tensor) -> torch.Tensor:
        """conv5_3 map (NHWC, fp32; bf16 is widened) -> vlad [N][K*C], intra- and L2-normalised, bit-equal to
        `aggregate_nhwc(feat, want_norm=True)` on an fp32 map and carrying an autograd graph to the LIVE
        `conv.weight` and `centroids` (and to the map, if it requires a gradient): netvlad.py:44-61 + 78-80 with
        their backward on the device (ops.netvlad_head)."""
        return ops.netvlad_head(feat_nhwc, self.conv.weight, self.centroids, self.normalize_input)

    @torch.no_grad()
    def forward(self, x):
        """x: the backbone's [N][C][h][w] fp32 map (reference layout)."""
        feat = ops.nchw_f32_to_nhwc(x.float().contiguous(), self.precision)
        raw, _ = self.aggregate_nhwc(feat, want_raw=True, want_norm=False)
        return raw


class EmbedNet(_PrecisionMixin, nn.Module):
    """ibl/models/netvlad.py:63-82: returns (pool_x [N][512], vlad [N][K*C] intra+L2 normalised)."""

    def __init__(self, base_model, net_vlad):
        super().__init__()
        self.base_model = base_model
        self.net_vlad = net_vlad

    def _init_params(self):
        self.base_model._init_params()
        self.net_vlad._init_params()

    def _head(self, feat):
        _, vlad = self.net_vlad.aggregate_nhwc(feat, want_raw=False, want_norm=True)
        return ops.global_maxpool_nhwc(feat), vlad

    @torch.no_grad()
    def forward(self, x):
        return _with_range_guard(self.base_model, x, self._head)

    def forward_train(self, x, train_layers=None):
        """(pool_x [N][512], vlad_x [N][K*C]) as `forward`, with vlad_x carrying an autograd graph to
        `net_vlad.conv.weight` and `net_vlad.centroids`: the "train only the VLAD layer" setting, for any loss
        written in torch and any torch optimizer.  The backbone is FROZEN here: it runs under no_grad in the model's
        precision, through the same range-guarded path as the eval forward, and its parameters receive no gradient
        (pool_x carries no graph either).  The parameters are read live, so the eval forward after an
        `optimizer.step()` sees the stepped weights.  vlad_x is bit-equal to the eval forward's where the conv5 map
        is fp32 (fp32, f16mx, bf16x3); in bf16 the map is widened to fp32 and the fp32 head runs on it, so the bits
        differ from the eval forward's bf16 head.  Unlike the eval forward, which reads the f16mx range flag behind
        the head's launches, this one reads it — a host synchronisation — BEFORE the head is enqueued: the autograd
        graph must be built on the map that stands.

        train_layers='conv5' (opt-in; the reference's default --layers conv5): the graph also reaches conv5_1,
        conv5_2 and conv5_3 — `backward()` fills .grad of their six tensors next to the two of NetVLAD
        (VGG.features_train_nhwc: frozen trunk up to pool4 in the model's precision, the three layers and their
        gradients in exact fp32, so vlad_x is the fp32 head on that map, not the eval forward's bits).  The gradient
        stops at pool4: 'conv4', 'conv3', 'conv2' and 'full' raise NotImplementedError."""
        if train_layers is not None:
            if train_layers in ("conv4", "conv3", "conv2", "full"):
                raise NotImplementedError(f"EmbedNet.forward_train: train_layers={train_layers!r} is not available: "
                                          "the gradient stops at pool4 (conv5_1 .. conv5_3 and the NetVLAD layer are "
                                          "trainable on the device; conv4 and below, with the max-pool's backward, "
                                          "are not)")
            if train_layers != "conv5":
                raise ValueError(f"EmbedNet.forward_train: unknown train_layers {train_layers!r}")
            feat = self.base_model.features_train_nhwc(x)
            with torch.no_grad():
                pool_x = ops.global_maxpool_nhwc(feat.detach())
            return pool_x, self.net_vlad.head_with_grad(feat)
        maps = []

        def keep(feat):
            maps.append(feat)
            return ops.global_maxpool_nhwc(feat)

        with torch.no_grad():
            pool_x = _with_range_guard(self.base_model, x, keep)
        return pool_x, self.net_vlad.head_with_grad(maps[-1])


class EmbedNetPCA(_PrecisionMixin, nn.Module):
    """ibl/models/netvlad.py:84-110: image batch -> [N][dim] unit-norm descriptors."""

    def __init__(self, base_model, net_vlad, dim=4096):
        super().__init__()
        self.base_model = base_model
        self.net_vlad = net_vlad
        self.pca_layer = nn.Conv2d(net_vlad.num_clusters * net_vlad.dim, dim, 1, stride=1, padding=0)
        self._cache: Dict = {}
        self._hook_state_dict_loads()

    def _init_params(self):
        self.base_model._init_params()
        self.net_vlad._init_params()

    def _pca_params(self):
        w, b = self.pca_layer.weight, self.pca_layer.bias
        key = (self.precision, _fingerprint([w, b]))
        hit = self._cache.get("pca")
        if hit is None or hit[0] != key:
            w2 = w.detach().float().reshape(w.shape[0], -1).contiguous()
            self._cache["pca"] = (key, ops.PcaWeight(ops.cast(w2, self.precision)), b.detach().float().contiguous())
            hit = self._cache["pca"]
        return hit[1], hit[2]

    def head_from_features(self, feat: torch.Tensor) -> torch.Tensor:
        """conv5_3 map (NHWC) -> descriptors: NetVLAD, intra + L2 norm, PCA, L2 (netvlad.py:98-108)."""
        _, vlad = self.net_vlad.aggregate_nhwc(feat, want_raw=False, want_norm=True)
        w, b = self._pca_params()
        return ops.pca(vlad, w, b, l2norm=True)

    @torch.no_grad()
    def forward(self, x):
        return _with_range_guard(self.base_model, x, self.head_from_features)

    def graphed(self, example: torch.Tensor, pipeline: bool = False):
        """hipGraph-replayed forward for a fixed batch shape (see GraphedDescriptor)."""
        return GraphedDescriptor(self, example, pipeline=pipeline)


def GraphedDescriptor(model: "EmbedNetPCA", example: torch.Tensor, pipeline: bool = False):
    """`EmbedNetPCA.forward` captured once into hipGraphs and replayed (openibl_amd.extract
    .GraphedForward): backbone (the matrix-core launches) and head (NetVLAD + PCA, ~10 launches).  A
    forward then costs the host two graph launches instead of ~30 kernel launches — on a shared host
    the eager path can become launch-bound at ~5 ms per batch.  Shapes, precision and parameters are
    frozen at capture time; the returned descriptor tensor is static and overwritten by a later call
    (clone it to keep it).

        fwd = model.graphed(example_batch)        # example_batch: resident [N][3][H][W] fp32
        desc = fwd(batch)                         # same shape; copied into the slot's static input
        desc = fwd()                              # again on the batch already in place

    pipeline=True keeps two slots (input, feature map, output each) and runs the head of batch i on
    a second stream while the backbone of batch i+1 already occupies the matrix cores; a batch passed
    to the call travels on a third (copy) stream.  The tensor returned by call i is then complete
    once `fwd.wait()` (or a device synchronisation) has returned, and is overwritten by call i+2."""
    from .extract import GraphedForward, _module_caches
    return GraphedForward(model.base_model.features_nhwc, model.head_from_features, example,
                          pipeline=pipeline, keep=_module_caches(model))


class EmbedRegionNet(_PrecisionMixin, nn.Module):
    """ibl/models/netvlad.py:112-207.  forward() is the evaluation branch (:199-205, identical to
    EmbedNet.forward).  The SFRS region-similarity branch (:123-194) is reached through two methods:
    `region_similarity(x)`, without gradients — what the reference runs on the frozen previous-generation model
    under torch.no_grad() (ibl/trainers.py:243-244) — and `forward_train(x, train_layers)`, the same three outputs
    with an autograd graph to the NetVLAD layer (and conv5), whose backward runs on the device (ops.region_vlad_train,
    ops.region_scores_train): the student's two calls in SFRSTrainer._forward (:240, :245).  forward() in training
    mode keeps raising: it is no_grad like every forward() of this package, and gradient-free tensors handed to a
    trainer would be a trap."""

    def __init__(self, base_model, net_vlad, tuple_size=1):
        super().__init__()
        self.base_model = base_model
        self.net_vlad = net_vlad
        self.tuple_size = tuple_size

    def _init_params(self):
        self.base_model._init_params()
        self.net_vlad._init_params()

    @torch.no_grad()
    def forward(self, x):
        if self.training:
            raise NotImplementedError("EmbedRegionNet: the SFRS training branch is not part of the "
                                      "MI355X inference path; call .eval() first (the forward-only region "
                                      "similarities of a frozen model: region_similarity(x))")
        return _with_range_guard(self.base_model, x, self._head)

    def _head(self, feat):
        _, vlad = self.net_vlad.aggregate_nhwc(feat, want_raw=False, want_norm=True)
        return ops.global_maxpool_nhwc(feat), vlad

    def _tuple_shape(self, batch: int):
        if int(self.net_vlad.num_clusters) != 64:
            raise ValueError(f"EmbedRegionNet: the region head's kernels are built for num_clusters = 64 (got "
                             f"{int(self.net_vlad.num_clusters)}); other cluster counts run in EmbedNet / EmbedNetPCA "
                             f"and in this model's eval forward, not in its region similarities")
        T = int(self.tuple_size)
        if T <= 0 or batch % T:
            raise ValueError(f"EmbedRegionNet: a batch of {batch} images is not a multiple of tuple_size {T}")
        if batch // T < 2:
            raise ValueError(f"EmbedRegionNet: a tuple needs an anchor and at least one pair "
                             f"(batch {batch}, tuple_size {T}: {batch // T} image per tuple)")
        return T, batch // T

    def _region_head(self, feat):
        """conv5_3 map [T*(1+n)][h][w][C] (NHWC), tuple-major, anchor first -> (score, vlad_A, vlad_B)."""
        T, per = self._tuple_shape(int(feat.shape[0]))
        w, c = self.net_vlad._params()
        vec = ops.region_vlad(feat, w, c, self.net_vlad.normalize_input)
        score = ops.region_scores(vec, T)
        vec = vec.view(T, per, 9, vec.shape[-1])
        return score, vec[:, :1], vec[:, 1:]

    @torch.no_grad()
    def region_similarity(self, x):
        """The reference's training-mode forward (_forward_train, netvlad.py:188-194), without gradients, in
        either module mode.  x: images [T*(1+n)][3][H][W], tuple-major, the first image of each tuple is the
        anchor (T = tuple_size, n >= 1 pairs per tuple); H // 16 and W // 16 must be even.  Returns
          score  [T][n][9][9]  score[t, j, a, b] = <vlad_A[t, 0, a], vlad_B[t, j, b]>,
          vlad_A [T][1][9][L], vlad_B [T][n][9][L]   (L = num_clusters * dim; views of one [T][1+n][9][L] tensor),
        fp32 on the device; the 9 regions are [whole, top, bottom, left, right, q0 (top-left), q1 (top-right),
        q2 (bottom-left), q3 (bottom-right)].  The reference's own arithmetic only runs with tuple_size == 1; here
        tuple_size > 1 is the tuple_size == 1 result per tuple, stacked."""
        if x.dim() != 4:
            raise ValueError("EmbedRegionNet.region_similarity: images [N][3][H][W]")
        self._tuple_shape(int(x.shape[0]))
        H, W = (int(x.shape[1]), int(x.shape[2])) if x.dtype == torch.uint8 else (int(x.shape[2]), int(x.shape[3]))
        h, w = ops.vgg16_feature_hw(H, W)
        if h % 2 or w % 2:
            raise ValueError(f"EmbedRegionNet.region_similarity: the conv5 map of a {H} x {W} image is {h} x {w}, "
                             f"both sides must be even to cut it into quarters")
        return _with_range_guard(self.base_model, x, self._region_head)

    def _region_head_train(self, feat):
        """_region_head with a graph: the live parameters, the differentiable head and scores."""
        T, per = self._tuple_shape(int(feat.shape[0]))
        nv = self.net_vlad
        vec = ops.region_vlad_train(feat, nv.conv.weight, nv.centroids, nv.normalize_input)
        score = ops.region_scores_train(vec, T)
        vec = vec.view(T, per, 9, vec.shape[-1])
        return score, vec[:, :1], vec[:, 1:]

    def forward_train(self, x, train_layers=None):
        """(score [T][n][9][9], vlad_A [T][1][9][L], vlad_B [T][n][9][L]) as `region_similarity`, carrying an autograd
        graph to `net_vlad.conv.weight` and `net_vlad.centroids`: the reference's training-mode forward
        (_forward_train, netvlad.py:188-194) for any loss written in torch.  All three outputs are differentiable —
        SFRSTrainer._forward reads vlad_A / vlad_B for loss_hard and score for loss_soft — and autograd adds the two
        gradients that reach the region vectors.  The backbone is FROZEN here: it runs under no_grad in the model's
        precision through the range guard, and the f16mx range flag is read — a host synchronisation — BEFORE the head
        is enqueued, as in EmbedNet.forward_train.  The values are bit-equal to `region_similarity(x)` where the conv5
        map is fp32 (fp32, f16mx, bf16x3); a bf16 map is widened to fp32 in both.

        train_layers='conv5': the map comes from `base_model.features_train_nhwc(x)` and the graph also reaches the
        six conv5 tensors.  'conv4', 'conv3', 'conv2' and 'full' raise NotImplementedError: the gradient stops at
        pool4."""
        if x.dim() != 4:
            raise ValueError("EmbedRegionNet.forward_train: images [N][3][H][W]")
        self._tuple_shape(int(x.shape[0]))
        H, W = (int(x.shape[1]), int(x.shape[2])) if x.dtype == torch.uint8 else (int(x.shape[2]), int(x.shape[3]))
        h, w = ops.vgg16_feature_hw(H, W)
        if h % 2 or w % 2:
            raise ValueError(f"EmbedRegionNet.forward_train: the conv5 map of a {H} x {W} image is {h} x {w}, "
                             f"both sides must be even to cut it into quarters")
        if train_layers is not None:
            if train_layers in ("conv4", "conv3", "conv2", "full"):
                raise NotImplementedError(f"EmbedRegionNet.forward_train: train_layers={train_layers!r} is not "
                                          "available: the gradient stops at pool4 (conv5_1 .. conv5_3 and the NetVLAD "
                                          "layer are trainable on the device; conv4 and below are not)")
            if train_layers != "conv5":
                raise ValueError(f"EmbedRegionNet.forward_train: unknown train_layers {train_layers!r}")
            return self._region_head_train(self.base_model.features_train_nhwc(x))
        maps = []

        def keep(feat):
            maps.append(feat)
            return None

        with torch.no_grad():
            _with_range_guard(self.base_model, x, keep)
        return self._region_head_train(maps[-1])

    @torch.no_grad()
    def _compute_region_sim(self, feature_A, feature_B):
        """The reference's entry for callers that hold conv5 maps (netvlad.py:123): feature_A [T][C][h][w] the
        anchors' maps, feature_B [T*n][C][h][w] the pairs' maps (NCHW fp32) -> (score, vlad_A, vlad_B) as
        region_similarity returns them."""
        T = int(self.tuple_size)
        if feature_A.dim() != 4 or feature_B.dim() != 4 or int(feature_A.shape[0]) != T:
            raise ValueError(f"EmbedRegionNet._compute_region_sim: feature_A must hold tuple_size = {T} maps [C][h][w]")
        if int(feature_B.shape[0]) == 0 or int(feature_B.shape[0]) % T:
            raise ValueError(f"EmbedRegionNet._compute_region_sim: {int(feature_B.shape[0])} pair maps are not a "
                             f"positive multiple of tuple_size {T}")
        n = int(feature_B.shape[0]) // T
        maps = torch.cat([feature_A.float().unsqueeze(1), feature_B.float().view(T, n, *feature_B.shape[1:])], dim=1)
        h, w = int(maps.shape[-2]), int(maps.shape[-1])
        if h % 2 or w % 2:
            raise ValueError(f"EmbedRegionNet._compute_region_sim: the map is {h} x {w}, both sides must be even")
        feat = ops.nchw_f32_to_nhwc(maps.flatten(0, 1).contiguous(), "fp32")
        return self._region_head(feat)


_factory = {
    "vgg16": vgg16,
    "netvlad": NetVLAD,
    "embednet": EmbedNet,
    "embednetpca": EmbedNetPCA,
    "embedregionnet": EmbedRegionNet,
}


def names():
    return sorted(_factory.keys())


def create(name, *args, **kwargs):
    """Same factory contract as ibl/models/__init__.py:20-53."""
    if name not in _factory:
        raise KeyError("Unknown model:", name)
    return _factory[name](*args, **kwargs)
