"""Data-side helpers test.py imports (ibl/utils/data/__init__.py): IterLoader and the test/train
transforms, written without torchvision (absent from this image): PIL resize + to-tensor +
mean/std normalisation with the reference's constants (std = 1/255, i.e. mean-subtracted 0..255
pixels)."""
from __future__ import absolute_import

import numpy as np
import torch

from .dataset import Dataset
from .preprocessor import Preprocessor

MEAN = [0.48501960784313836, 0.4579568627450961, 0.4076039215686255]
STD = [0.00392156862745098, 0.00392156862745098, 0.00392156862745098]


class IterLoader:
    def __init__(self, loader, length=None):
        self.loader = loader
        self.length = length
        self.iter = None

    def __len__(self):
        return self.length if self.length is not None else len(self.loader)

    def new_epoch(self):
        self.iter = iter(self.loader)

    def next(self):
        try:
            return next(self.iter)
        except (StopIteration, TypeError):
            self.iter = iter(self.loader)
            return next(self.iter)


class _TestTransform(object):
    """Resize((h, w)) — or Resize(max(h, w)) on the shorter side for Tokyo queries — then
    ToTensor and Normalize.  resize=False (only with as_uint8=True): the decoded bytes at their stored size, for a
    resize on the device (openibl_amd.augment.Resize, the `input_resize` of extract_features)."""

    def __init__(self, height, width, keep_aspect=False, as_uint8=False, resize=True):
        if not resize and not as_uint8:
            raise ValueError("resize=False hands over the decoded bytes at their stored size: it needs as_uint8=True")
        self.size = (height, width)
        self.keep_aspect = keep_aspect
        self.as_uint8 = as_uint8
        self.resize = resize
        self.mean = torch.tensor(MEAN, dtype=torch.float32).view(3, 1, 1)
        self.std = torch.tensor(STD, dtype=torch.float32).view(3, 1, 1)

    def __call__(self, img):
        if not self.resize:
            return torch.from_numpy(np.array(img, dtype=np.uint8))
        from PIL import Image
        if self.keep_aspect:
            s = max(self.size)
            w, h = img.size
            if w <= h:
                nw, nh = s, int(s * h / w)
            else:
                nw, nh = int(s * w / h), s
        else:
            nh, nw = self.size
        img = img.resize((nw, nh), Image.BILINEAR)
        if self.as_uint8:   # raw [H][W][3] bytes: the model normalises them inside its first kernel
            return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy())
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
        return (x - self.mean) / self.std


def get_transformer_test(height, width, tokyo=False, as_uint8=False, resize=True):
    """as_uint8=True (extension): skip ToTensor + Normalize and hand the decoded uint8 HWC image to
    the model, which applies exactly that arithmetic on the GPU — same descriptors, 4x less PCIe.
    resize=False (extension, only with as_uint8=True, ValueError otherwise): skip the host's Resize too and hand
    over the decoded bytes at their stored size; `extract_features(..., input_resize=(height, width))` — or an
    openibl_amd.augment.Resize(height, width, keep_aspect=tokyo, out='uint8') — resizes them on the device with
    PIL's bits.  Images of different stored sizes then need a batch size of 1 or a loader that groups them."""
    return _TestTransform(height, width, keep_aspect=tokyo, as_uint8=as_uint8, resize=resize)


def get_transformer_train(height, width, as_uint8=False, resize=True):
    """The host half of the training transform.  The reference's is ColorJitter(0.7, 0.7, 0.7, 0.5), Resize,
    ToTensor, Normalize on the host; here the colour jitter runs on the device (openibl_amd.augment.ColorJitter, the
    `augment` of ibl.trainers).  as_uint8=True (extension): the resized raw [H][W][3] bytes, which a trainer with
    `augment` set jitters and normalises on the device — the batch crosses PCIe as uint8.  The default is the test
    transform, Resize + ToTensor + Normalize without jitter: what a trainer without `augment` takes.
    resize=False (extension, only with as_uint8=True, ValueError otherwise): the decoded bytes at their stored size,
    for `augment=Compose(ColorJitter(..., out='uint8'), Resize(height, width))` — the reference's order, jitter
    BEFORE the resize, PIL's bits in both.  (With the host's resize the jitter runs behind it: the reference's bits
    only when the stored images already have the target size, otherwise the two differ in rounding.)"""
    return _TestTransform(height, width, as_uint8=as_uint8, resize=resize)
