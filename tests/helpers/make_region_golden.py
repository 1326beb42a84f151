"""Generate tests/golden/region_*.npz by running THE REFERENCE's EmbedRegionNet training branch.

Run in the build container only (`python tests/helpers/make_region_golden.py`): the reference tree is imported
through oracle.refshim, exactly as oracle/make_golden.py does, and does not exist on the GPU box.

What is exercised, through the reference's own code objects:
  models.create('embedregionnet', base, net_vlad, tuple_size=1) in .train() under torch.no_grad()
  -> EmbedRegionNet.forward -> _forward_train -> _compute_region_sim     (ibl/models/netvlad.py:123-198)
The reference's view() arithmetic only runs with tuple_size == 1 on a current torch, so the
fixtures hold one tuple each: image 0 is the anchor, the others are its pairs.

The fixtures hold the reference's outputs, the seeds and the shapes; the images are regenerated from the seed by
openibl_amd.synth.images on both sides.  `score` is stored in full, the region vectors at a column stride
(`vlad_stride`, like `feat_stride` of desc_480x640.npz) to keep the files small.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from oracle import refshim  # noqa: E402

refshim.install()  # puts the reference FIRST on sys.path: `import ibl` below is the reference

from openibl_amd import synth  # noqa: E402

OUT = ROOT / "tests" / "golden"
WEIGHT_SEED = 0
VLAD_STRIDE = 8


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import models

    torch.set_num_threads(8)
    sd = synth.embednetpca_state(WEIGHT_SEED)
    full = refshim.reference_model(sd)
    region = models.create("embedregionnet", full.base_model, full.net_vlad, tuple_size=1).train()

    def run(name, n_pairs, h, w, seed):
        x = synth.images(1 + n_pairs, h, w, seed=seed)
        with torch.no_grad():
            score, vlad_a, vlad_b = region(x)
        assert tuple(score.shape) == (1, n_pairs, 9, 9) and tuple(vlad_b.shape) == (1, n_pairs, 9, 64 * 512)
        np.savez_compressed(
            OUT / f"{name}.npz",
            weight_seed=WEIGHT_SEED, image_seed=seed, shape=np.array([1 + n_pairs, 3, h, w]), tuple_size=1,
            vlad_stride=VLAD_STRIDE, score=score.numpy(),
            vlad_A=np.ascontiguousarray(vlad_a.numpy()[..., ::VLAD_STRIDE]),
            vlad_B=np.ascontiguousarray(vlad_b.numpy()[..., ::VLAD_STRIDE]))
        print(name, "score", tuple(score.shape), "diag of pair 0", score[0, 0].diagonal().tolist()[:3],
              "file", (OUT / f"{name}.npz").stat().st_size, "bytes")

    run("region_small", 3, 64, 96, seed=31)
    run("region_480x640", 2, 480, 640, seed=32)


if __name__ == "__main__":
    main()
