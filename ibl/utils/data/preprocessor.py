"""`Preprocessor(records, root, transform)`: the torch Dataset examples/test.py wraps its record
lists in (test.py:40-54).  Item i is `(image, fname, pid, utm_x, utm_y)`; an index list yields the
list of items (the tuple samplers of the reference ask for several images at once).

raw=True (extension): item 0 is the FILE'S BYTES as a 1-D uint8 tensor — nothing is decoded and no transform applies
(ValueError if one is given) — for a loader with `collate_fn=openibl_amd.jpeg.collate`, whose batches
`extract_features(..., input_decode=True)` decodes on the device."""
from __future__ import absolute_import

import os

from torch.utils.data import Dataset as _TorchDataset


def _open_rgb(path):
    from PIL import Image      # imported on first use: the package imports without Pillow
    with Image.open(path) as im:
        return im.convert('RGB')


class Preprocessor(_TorchDataset):
    def __init__(self, dataset, root=None, transform=None, raw=False):
        super(Preprocessor, self).__init__()
        if raw and transform is not None:
            raise ValueError("raw=True hands over the file's bytes: no transform applies to them")
        self.dataset, self.root, self.transform, self.raw = dataset, root, transform, raw

    def __len__(self):
        return len(self.dataset)

    def _item(self, i):
        record = self.dataset[i]
        fname = record[0]
        path = fname if self.root is None else os.path.join(self.root, fname)
        if self.raw:
            import numpy as np
            import torch
            return (torch.from_numpy(np.fromfile(path, dtype=np.uint8)),) + tuple(record)
        image = _open_rgb(path)
        if self.transform is not None:
            image = self.transform(image)
        return (image,) + tuple(record)

    def __getitem__(self, indices):
        many = isinstance(indices, (tuple, list))
        return list(map(self._item, indices)) if many else self._item(indices)
