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

Three more cases in the regime a training run is in (inputs: draw_trained_inputs / draw_tuple_inputs of the helper; dX
at every fifth pixel of an image, `dx_stride`, with the regime figures alpha, mean_max_a, min_A):
  netvlad_backward_trained_2x12x16    the weights _init_params sets: the generator runs the reference's own
                                      _init_params() on the recipe's centroids and descriptors and asserts its
                                      conv.weight and centroids are the recipe's within 1e-6
  netvlad_backward_saturated_2x8x8    those weights times 4: max_k a_pk = 1.0000.  dW tends to zero there and its
                                      relative error means little even for the reference: its ref_err is stored and
                                      printed, not asserted
  netvlad_backward_tuple_1x4x8x8      one tuple of four near-identical maps under the triplet loss's gradient: the
                                      images' dC contributions cancel.  The jitter starts at 0.05 and is raised
                                      until the reference's own dC is within 1e-5 of float64: 0.05 (cancellation
                                      sum_n |dC_n| / |sum_n dC_n| = 99.6) 2.30e-5, 0.07 (59.0) 1.49e-5, 0.1 (32.7)
                                      7.15e-6.  Kept: jitter 0.1, cancellation 32.7, both in the fixture
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
DX_STRIDE = 5          # the new cases: every fifth pixel of an image (co-prime with the kernels' 32-pixel chunks)
CASES = (("netvlad_backward_2x3x5_norm", 41, 2, 3, 5, True),
         ("netvlad_backward_3x4x6_raw", 42, 3, 4, 6, False))
# (name, seed, N, h, w_, sharpen): ref.draw_trained_inputs(seed, N, h, w_, sharpen, populate=True)
TRAINED_CASES = (("netvlad_backward_trained_2x12x16", 51, 2, 12, 16, 1.0),
                 ("netvlad_backward_saturated_2x8x8", 52, 2, 8, 8, 4.0))
# (name, seed, B, n, h, w_): ref.draw_tuple_inputs(seed, B, n, h, w_, jitter), the jitter found below
TUPLE_CASE = ("netvlad_backward_tuple_1x4x8x8", 60, 1, 4, 8, 8)
TUPLE_JITTERS = (0.05, 0.07, 0.1, 0.14, 0.2)      # cancellation about 100, 60, 33, 19, 10.6
KEYS = ("dW", "dC", "dX")


class _StubBase(torch.nn.Module):
    def forward(self, x):
        return x.amax((2, 3)), x


def _reference_autograd(ref_netvlad, layer, x, G):
    """The reference's EmbedNet over the stub base, vlad_x.backward(G): its fp32 outputs, dX in NHWC."""
    layer.zero_grad()
    model = ref_netvlad.EmbedNet(_StubBase(), layer).train()
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    _, vlad_x = model(xt)
    vlad_x.backward(torch.from_numpy(G))
    return {"Y": vlad_x.detach().numpy(),
            "dW": layer.conv.weight.grad.reshape(64, 512).numpy().copy(),
            "dC": layer.centroids.grad.numpy().copy(),
            "dX": xt.grad.permute(0, 2, 3, 1).contiguous().numpy()}


def _layer(ref_netvlad, w, c, normalize):
    layer = ref_netvlad.NetVLAD(num_clusters=64, dim=512, normalize_input=normalize)
    with torch.no_grad():
        layer.conv.weight.copy_(torch.from_numpy(w)[:, :, None, None])
        layer.centroids.copy_(torch.from_numpy(c))
    return layer


def _save(name, arrays):
    """Write the fixture unless the file already holds exactly these arrays (an .npz carries a timestamp)."""
    path = OUT / f"{name}.npz"
    if path.exists():
        old = dict(np.load(path, allow_pickle=False))
        if old.keys() == arrays.keys() and all(np.array_equal(old[k], np.asarray(v)) for k, v in arrays.items()):
            print(name, "reproduces the committed fixture,", path.stat().st_size, "bytes")
            assert path.stat().st_size < 500_000
            return
    np.savez_compressed(path, **arrays)
    assert path.stat().st_size < 500_000, path.stat().st_size
    print(name, "file", path.stat().st_size, "bytes")


def _errors(name, got, want):
    err = {k: ref.rel_l2(got[k], want[k]) for k in ("Y",) + KEYS}
    print(name, " ".join(f"{k} {v:.3e}" for k, v in err.items()))
    return err


def _new_fixture(got, err, seed, shape, info, **extra):
    """dW, dC in full; dX at every DX_STRIDE-th pixel of an image, vlad_x at a column stride.  ref_err is over the
    full arrays (the unit of the device tests' bars), ref_err_dx_stored over the stored rows of dX."""
    N, h, w_ = shape
    dxs = got["dX"].reshape(N, h * w_, 512)[:, ::DX_STRIDE]
    return dict(seed=seed, shape=np.array([N, h, w_, 512]), normalize_input=1, vlad_stride=VLAD_STRIDE,
                dx_stride=DX_STRIDE, vlad_x=np.ascontiguousarray(got["Y"][:, ::VLAD_STRIDE]), dW=got["dW"],
                dC=got["dC"], dX=np.ascontiguousarray(dxs), ref_err=np.array([err[k] for k in KEYS]),
                ref_err_dx_stored=err["dX_stored"], alpha=info["alpha"], mean_max_a=info["mean_max_a"],
                min_A=info["min_A"], **extra)


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl.models import netvlad as ref_netvlad

    torch.set_num_threads(8)
    for name, seed, N, h, w_, normalize in CASES:
        x, w, c, G = ref.draw_inputs(seed, N, h, w_)
        got = _reference_autograd(ref_netvlad, _layer(ref_netvlad, w, c, normalize), x, G)
        want = ref.head_and_grads(x, w, c, G, normalize)
        err = _errors(name, got, want)
        assert max(err.values()) <= 1e-5, err
        _save(name, dict(seed=seed, shape=np.array([N, h, w_, 512]), normalize_input=int(normalize),
                         vlad_stride=VLAD_STRIDE, vlad_x=np.ascontiguousarray(got["Y"][:, ::VLAD_STRIDE]),
                         dW=got["dW"], dC=got["dC"], dX=got["dX"],
                         ref_err=np.array([err["dW"], err["dC"], err["dX"]])))

    def stored_dx_err(got, want, N, P):
        return ref.rel_l2(got["dX"].reshape(N, P, 512)[:, ::DX_STRIDE], want["dX"].reshape(N, P, 512)[:, ::DX_STRIDE])

    for name, seed, N, h, w_, sharpen in TRAINED_CASES:
        x, w, c, G, info = ref.draw_trained_inputs(seed, N, h, w_, sharpen=sharpen, populate=True)
        print(name, {k: v for k, v in info.items() if k != "descs"})
        layer = ref_netvlad.NetVLAD(num_clusters=64, dim=512, normalize_input=True)
        if sharpen == 1.0:
            # the recipe IS the reference's initialisation: its own _init_params from the recipe's centres and
            # normalised descriptors gives the recipe's w and c
            layer.clsts = c.astype(np.float64)
            layer.traindescs = info["descs"]
            layer._init_params()
            e_w = ref.rel_l2(layer.conv.weight.detach().reshape(64, 512).numpy(), w)
            e_c = ref.rel_l2(layer.centroids.detach().numpy(), c)
            print(name, f"_init_params of the reference against the recipe: w {e_w:.3e} c {e_c:.3e}, "
                        f"alpha {layer.alpha:.9g} against {info['alpha']:.9g}")
            assert e_w <= 1e-6 and e_c <= 1e-6, (e_w, e_c)
        else:
            layer = _layer(ref_netvlad, w, c, True)
        got = _reference_autograd(ref_netvlad, layer, x, G)
        want = ref.head_and_grads(x, w, c, G, True)
        err = _errors(name, got, want)
        err["dX_stored"] = stored_dx_err(got, want, N, h * w_)
        judged = {k: v for k, v in err.items() if not (sharpen != 1.0 and k == "dW")}   # dW -> 0 as the softmax saturates
        assert max(judged.values()) <= 1e-5, err
        _save(name, _new_fixture(got, err, seed, (N, h, w_), info, sharpen=sharpen))

    name, seed, B, n, h, w_ = TUPLE_CASE
    kept = None
    for jitter in TUPLE_JITTERS:
        x, w, c, G, info = ref.draw_tuple_inputs(seed, B, n, h, w_, jitter)
        got = _reference_autograd(ref_netvlad, _layer(ref_netvlad, w, c, True), x, G)
        want = ref.head_and_grads(x, w, c, G, True)
        err = _errors(f"{name} jitter {jitter} cancellation {info['cancellation']:.1f}", got, want)
        err["dX_stored"] = stored_dx_err(got, want, B * n, h * w_)
        if max(err.values()) <= 1e-5 and info["cancellation"] >= 10.0:
            kept = (jitter, got, err, info)
            break
    assert kept is not None, "no jitter with a cancellation of 10 or more at which the reference is within 1e-5"
    jitter, got, err, info = kept
    print(name, {k: v for k, v in info.items()}, "jitter", jitter)
    _save(name, _new_fixture(got, err, seed, (B * n, h, w_), info, jitter=jitter, tuple=np.array([B, n]),
                             cancellation=info["cancellation"], loss=info["loss"]))


if __name__ == "__main__":
    main()
