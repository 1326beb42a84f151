"""Generate tests/golden/netvlad_backward_*.npz by running THE REFERENCE's NetVLAD head under torch autograd.

Run in the build container only (`python tests/helpers/make_netvlad_backward_golden.py`): the reference tree is
imported through oracle.refshim, exactly as oracle/make_golden.py does, and does not exist on the GPU box.

What is exercised, through the reference's own code objects, in fp32 on the CPU:
  EmbedNet(stub base, NetVLAD(64, 512, normalize_input=...)).forward          (ibl/models/netvlad.py:44-61, 63-82)
  vlad_x.backward(G)
The stub base returns (x.amax((2, 3)), x): the conv5 map IS the input, so x.grad is the gradient the device kernels
return as grad_feat (here NCHW, as the reference's layout is).

The fixtures hold the reference's outputs, the seed and the shape; the inputs are regenerated from the seed on both
sides (tests/helpers/netvlad_grad_ref.draw_inputs).  dW, dC and dX are stored in full (dX in NHWC), vlad_x at a column
stride to keep a file under 500 KB.  The generator prints the rel-L2 error of the reference's fp32 gradients against
the float64 helper and asserts <= 1e-5: those figures are the unit of the device tests' bars.
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

sys.path.insert(0, str(ROOT / "tests"))
from helpers import netvlad_grad_ref as ref  # noqa: E402

OUT = ROOT / "tests" / "golden"
VLAD_STRIDE = 8
CASES = (("netvlad_backward_2x3x5_norm", 41, 2, 3, 5, True),
         ("netvlad_backward_3x4x6_raw", 42, 3, 4, 6, False))


class _StubBase(torch.nn.Module):
    def forward(self, x):
        return x.amax((2, 3)), x


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl.models import netvlad as ref_netvlad

    torch.set_num_threads(8)
    for name, seed, N, h, w_, normalize in CASES:
        x, w, c, G = ref.draw_inputs(seed, N, h, w_)
        layer = ref_netvlad.NetVLAD(num_clusters=64, dim=512, normalize_input=normalize)
        with torch.no_grad():
            layer.conv.weight.copy_(torch.from_numpy(w)[:, :, None, None])
            layer.centroids.copy_(torch.from_numpy(c))
        model = ref_netvlad.EmbedNet(_StubBase(), layer).train()
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        _, vlad_x = model(xt)
        vlad_x.backward(torch.from_numpy(G))
        got = {"Y": vlad_x.detach().numpy(),
               "dW": layer.conv.weight.grad.reshape(64, 512).numpy(),
               "dC": layer.centroids.grad.numpy(),
               "dX": xt.grad.permute(0, 2, 3, 1).contiguous().numpy()}
        want = ref.head_and_grads(x, w, c, G, normalize)
        err = {k: ref.rel_l2(got[k], want[k]) for k in ("Y", "dW", "dC", "dX")}
        print(name, " ".join(f"{k} {v:.3e}" for k, v in err.items()))
        assert max(err.values()) <= 1e-5, err
        path = OUT / f"{name}.npz"
        np.savez_compressed(path, seed=seed, shape=np.array([N, h, w_, 512]), normalize_input=int(normalize),
                            vlad_stride=VLAD_STRIDE, vlad_x=np.ascontiguousarray(got["Y"][:, ::VLAD_STRIDE]),
                            dW=got["dW"], dC=got["dC"], dX=got["dX"],
                            ref_err=np.array([err["dW"], err["dC"], err["dX"]]))
        assert path.stat().st_size < 500_000, path.stat().st_size
        print(name, "file", path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
