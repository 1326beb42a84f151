"""Training augmentation on the device: `ColorJitter`, `Resize` and `Compose` for raw uint8 batches.

The reference's training transform is ColorJitter(0.7, 0.7, 0.7, 0.5) -> Resize -> ToTensor -> Normalize
(ibl/utils/data/__init__.py:29-35 of the reference, through torchvision and PIL on the host).  Here the loader hands
over raw bytes, the batch crosses to the device as uint8, ops.color_jitter applies the jitter and ops.resize_u8 the
resize — both with PIL's arithmetic, bit for bit — and the normalisation rides behind the last of them:

    get_transformer_train(480, 640, as_uint8=True, resize=False)           # the decoded bytes at their stored size
    augment = Compose(ColorJitter(0.7, 0.7, 0.7, 0.5, out='uint8'), Resize(480, 640))      # the reference's order

Limit, only when the HOST resizes (`get_transformer_train(..., as_uint8=True)` with its default resize=True and a
bare ColorJitter as `augment`): the reference jitters BEFORE Resize, that flow after it.  The two agree bit for bit
exactly when the stored images already have the target size (Pitts: 640 x 480); otherwise both are valid augmentations
of the same distribution that differ in rounding.  With the device resize the order is the reference's.

From the files' bytes (a loader over `Preprocessor(..., raw=True)` with `collate_fn=jpeg.collate_tuples`): `DecodeJpeg`
in front decodes the batch on the device, files of any mix of stored sizes included — the jitter then runs in place on
the decoder's packed buffer (`ops.PackedImages`) and the resize turns that into the dense batch:

    augment = Compose(DecodeJpeg(), ColorJitter(0.7, 0.7, 0.7, 0.5, out='uint8'), Resize(480, 640))"""
from __future__ import annotations

import numbers
from typing import Optional

import torch

from . import ops

BRIGHTNESS, CONTRAST, SATURATION, HUE, SKIP = 0, 1, 2, 3, -1


def _check_range(value, name, center=1.0, bound=(0.0, float("inf")), clip_first_on_zero=True):
    """torchvision's ColorJitter._check_input: a scalar v is [center - v, center + v] (the lower end clipped at 0 for
    everything but hue), a pair is taken as given; a range that is the single point `center` disables the op."""
    if isinstance(value, numbers.Number) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"If {name} is a single number, it must be non negative.")
        value = [center - float(value), center + float(value)]
        if clip_first_on_zero:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        value = [float(value[0]), float(value[1])]
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2.")
    if not bound[0] <= value[0] <= value[1] <= bound[1]:
        raise ValueError(f"{name} values should be between {bound}, but got {value}.")
    if value[0] == value[1] == center:
        return None
    return (value[0], value[1])


def hue_byte(hue: float) -> int:
    """What torchvision adds to PIL's H plane: uint8(hue * 255), truncated toward zero, wrapping mod 256."""
    return int(hue * 255) % 256


class ColorJitter(object):
    """torchvision.transforms.ColorJitter for a raw uint8 batch on the device.

    brightness, contrast, saturation: a scalar v (factor drawn from [max(0, 1 - v), 1 + v]) or a pair (lo, hi);
    hue: a scalar v with 0 <= v <= 0.5 (shift drawn from [-v, v]) or a pair inside [-0.5, 0.5].  A range that
    contains only the identity disables its op.  `generator`: the torch.Generator (CPU) the draws come from; None:
    the global one.  `out`: 'float' (normalised [N][3][H][W] float32, what forward_train takes) or 'uint8'.

    Every image of a batch gets its own order and factors.  The draws follow the current torchvision's
    `ColorJitter.get_params` — one torch.randperm(4), then one torch.empty(1).uniform_(lo, hi) per ENABLED op in the
    order brightness, contrast, saturation, hue.  torchvision is not available where this was written: the order
    of the draws is taken from its published source and could not be verified against a run of it, so the same seed
    is not guaranteed to give torchvision's stream; the distribution is the same either way."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, generator: Optional[torch.Generator] = None,
                 out: str = "float"):
        self.brightness = _check_range(brightness, "brightness")
        self.contrast = _check_range(contrast, "contrast")
        self.saturation = _check_range(saturation, "saturation")
        self.hue = _check_range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip_first_on_zero=False)
        if out not in ops.JITTER_OUT:
            raise ValueError(f"ColorJitter: out must be 'float' or 'uint8', not {out!r}")
        self.generator = generator
        self.out = out
        self.last_records = None    # the records of the last call (None: nothing was jittered)

    @property
    def enabled(self) -> bool:
        return any(r is not None for r in (self.brightness, self.contrast, self.saturation, self.hue))

    def _uniform(self, rng) -> float:
        return float(torch.empty(1).uniform_(rng[0], rng[1], generator=self.generator))

    def draw(self, n: int) -> torch.Tensor:
        """The records of n images, on the host: int32 [n][8] (ops.color_jitter).  A disabled op never appears in a
        record: its place in the drawn order holds -1."""
        ranges = (self.brightness, self.contrast, self.saturation)
        codes = torch.full((n, 4), SKIP, dtype=torch.int32)
        factors = torch.ones((n, 3), dtype=torch.float32)
        shifts = torch.zeros((n,), dtype=torch.int32)
        for i in range(n):
            order = torch.randperm(4, generator=self.generator).tolist()
            for k, rng in enumerate(ranges):
                if rng is not None:
                    factors[i, k] = self._uniform(rng)
            if self.hue is not None:
                shifts[i] = hue_byte(self._uniform(self.hue))
            for place, op in enumerate(order):
                if (self.hue if op == HUE else ranges[op]) is not None:
                    codes[i, place] = op
        return torch.cat((codes, factors.view(torch.int32), shifts[:, None]), dim=1).contiguous()

    def __call__(self, u8_batch, records: Optional[torch.Tensor] = None):
        """u8_batch [N][H][W][3] uint8 on the device -> the jittered batch (`out`).  `records`: host or device
        records to use instead of drawing (a replay).  With every op disabled nothing but the plain normalisation
        (or copy) is launched.
        An `ops.PackedImages` (what `DecodeJpeg` makes of a MixedJpegBatch) is jittered IN PLACE, every image at its
        stored size, and handed on: the stage needs out='uint8' then, the Resize behind it normalises."""
        packed = isinstance(u8_batch, ops.PackedImages)
        if packed and self.out != "uint8":
            raise ValueError("ColorJitter: a packed batch of mixed sizes is jittered in place and needs out='uint8' "
                             "(the Resize behind it hands float on)")
        if records is None:
            if not self.enabled:
                self.last_records = None
                return u8_batch if packed else ops.color_jitter(u8_batch, None, out=self.out)
            records = self.draw(len(u8_batch) if packed else u8_batch.shape[0])
        self.last_records = records
        if packed:
            return ops.jitter_packed(u8_batch, records.to(u8_batch.device))
        return ops.color_jitter(u8_batch, records.to(u8_batch.device), out=self.out)

    def __repr__(self):
        return (f"{self.__class__.__name__}(brightness={self.brightness}, contrast={self.contrast}, "
                f"saturation={self.saturation}, hue={self.hue})")


def aspect_size(height: int, width: int, h: int, w: int):
    """The target (height, width) of the reference's test transform for Tokyo queries (`keep_aspect`): the shorter
    side of an h x w image becomes max(height, width), the other one int(s * long / short) — the arithmetic of
    ibl.utils.data._TestTransform, in the same types."""
    s = max(height, width)
    if w <= h:
        return int(s * h / w), s
    return s, int(s * w / h)


class Resize(object):
    """The reference's Resize for a raw uint8 batch on the device: `img.resize((width, height), Image.BILINEAR)` of
    every image, PIL's bits (ops.resize_u8).  keep_aspect=True: the target of every batch is computed from its own
    size as the test transform does for Tokyo queries (`aspect_size`).  `out`: 'float' (normalised [N][3][H'][W']
    float32, what forward_train takes) or 'uint8' ([N][H'][W'][3], what the uint8 stems and a further stage take)."""

    def __init__(self, height: int, width: int, keep_aspect: bool = False, out: str = "float"):
        if isinstance(height, bool) or isinstance(width, bool) or \
                not isinstance(height, numbers.Integral) or not isinstance(width, numbers.Integral):
            raise TypeError(f"Resize: height and width must be integers, got {height!r}, {width!r}")
        if height < 1 or width < 1:
            raise ValueError(f"Resize: the target size must be positive, got {height} x {width}")
        if out not in ops.JITTER_OUT:
            raise ValueError(f"Resize: out must be 'float' or 'uint8', not {out!r}")
        self.height, self.width = int(height), int(width)
        self.keep_aspect = bool(keep_aspect)
        self.out = out

    def target(self, h: int, w: int):
        """(height, width) of the result for a source of h x w."""
        if self.keep_aspect:
            return aspect_size(self.height, self.width, int(h), int(w))
        return self.height, self.width

    def __call__(self, u8_batch) -> torch.Tensor:
        if isinstance(u8_batch, ops.PackedImages):      # mixed stored sizes: only the resized images form a batch
            if self.keep_aspect:
                raise ValueError("Resize: a packed batch of mixed sizes cannot be resized with keep_aspect=True: the "
                                 "images of one batch would get different sizes")
            return ops.resize_packed(u8_batch, (self.height, self.width), out=self.out)
        if u8_batch.dim() != 4:
            raise ValueError(f"Resize expects [N][H][W][3], got {tuple(u8_batch.shape)}")
        return ops.resize_u8(u8_batch, self.target(u8_batch.shape[1], u8_batch.shape[2]), out=self.out)

    def __repr__(self):
        return (f"{self.__class__.__name__}(height={self.height}, width={self.width}, "
                f"keep_aspect={self.keep_aspect}, out={self.out!r})")


class DecodeJpeg(object):
    """The first stage of a chain that starts from the files' bytes: a `jpeg.MixedJpegBatch` on the device (files of
    any mix of stored sizes; `jpeg.collate_tuples`, `jpeg.collate_mixed`) becomes an `ops.PackedImages` — the packed
    pixel buffer, the sizes, the device's geometry table and the per-image status, which stays on the device
    (`last_status`; nothing is read back here) — and a `jpeg.JpegBatch` of one size the dense uint8 batch
    [N][H][W][3].  scan: the route of `ops.decode_jpeg` ("auto", "serial", "chunked")."""

    out = "uint8"

    def __init__(self, scan: str = "auto"):
        from . import jpeg
        if scan not in jpeg.SCAN_ROUTES:
            raise ValueError(f"DecodeJpeg: scan must be one of {jpeg.SCAN_ROUTES}, not {scan!r}")
        self.scan = scan
        self.last_status = None     # int32 [N] on the device: the statuses of the last call

    def __call__(self, batch):
        from . import jpeg
        if isinstance(batch, jpeg.MixedJpegBatch):
            images = ops.decode_jpeg_packed(batch, scan=self.scan)
            self.last_status = images.status
            return images
        if isinstance(batch, jpeg.JpegBatch):
            pixels, self.last_status = ops.decode_jpeg(batch, check=False, scan=self.scan)
            return pixels
        raise ValueError(f"DecodeJpeg decodes a MixedJpegBatch or a JpegBatch (a loader over Preprocessor(..., "
                         f"raw=True) with collate_fn=openibl_amd.jpeg.collate_tuples / collate_mixed / collate), got "
                         f"{type(batch).__name__}")

    def __repr__(self):
        return f"{self.__class__.__name__}(scan={self.scan!r})"


class Compose(object):
    """Chains stages on a device batch: Compose(a, b)(x) = b(a(x)).  Every stage but the last must hand uint8 on
    (out='uint8').  The reference's training transform is
    Compose(ColorJitter(0.7, 0.7, 0.7, 0.5, out='uint8'), Resize(480, 640)).
    Keyword arguments of a call go to the FIRST stage (the `records=` of a ColorJitter replay); `records=` reaches
    the ColorJitter stage wherever it stands — behind a DecodeJpeg for instance:
    Compose(DecodeJpeg(), ColorJitter(0.7, 0.7, 0.7, 0.5, out='uint8'), Resize(480, 640)) is the whole chain from the
    files' bytes."""

    def __init__(self, *stages):
        if not stages:
            raise ValueError("Compose needs at least one stage")
        for k, stage in enumerate(stages):
            if not callable(stage):
                raise TypeError(f"Compose: stage {k} is not callable: {stage!r}")
            if k + 1 < len(stages) and getattr(stage, "out", "uint8") != "uint8":
                raise ValueError(f"Compose: stage {k} ({stage!r}) hands float on; every stage but the last needs "
                                 f"out='uint8'")
        self.stages = tuple(stages)

    def __call__(self, batch, **first_stage_args) -> torch.Tensor:
        at = 0
        if "records" in first_stage_args and not isinstance(self.stages[0], ColorJitter):
            at = next((k for k, s in enumerate(self.stages) if isinstance(s, ColorJitter)), 0)
        for k, stage in enumerate(self.stages):
            batch = stage(batch, **first_stage_args) if k == at else stage(batch)
        return batch

    def __repr__(self):
        return f"{self.__class__.__name__}({', '.join(repr(s) for s in self.stages)})"
