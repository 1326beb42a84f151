"""Generate tests/golden/netvlad_k.npz by running THE REFERENCE's NetVLAD head for cluster counts other than 64.

Run in the build container only (`python tests/helpers/make_netvlad_k_golden.py`): the reference tree is imported
through oracle.refshim, exactly as make_netvlad_backward_golden.py does, and does not exist on the GPU box.

What is exercised, through the reference's own code objects, on the CPU, once in float32 and once in float64:
  NetVLAD(K, 512, normalize_input=...).forward                                   -> vlad_raw   (netvlad.py:44-61)
  EmbedNet(stub base, that layer).forward, vlad_x.backward(G)                    -> vlad_norm, dW, dC, dX (:63-82)
The stub base returns (x.amax((2, 3)), x): the conv5 map IS the input.

Cases (the smallest at which each path of the K-general kernels can go wrong; KP = K rounded up to 32):
  k16_2x3x5_norm      K = 16, N = 2, 3 x 5     a half-empty column tile, P < one 32-pixel chunk
  k48_3x6x8_norm      K = 48, N = 3, 6 x 8     P = 48: one full and one partial chunk; K no multiple of 32, no power of 2
  k128_2x5x7_norm     K = 128, N = 2, 5 x 7    four column tiles
  k32_1x8x8_raw       K = 32, N = 1, 8 x 8     normalize_input=False
  k32_tuple_4x4x4     K = 32, one tuple of 1 + 1 + 2 near-identical 4 x 4 maps under the triplet loss's gradient: the
                      images' dC contributions nearly cancel (the regime the fp64 parts of the backward exist for)
  k32_saturated_2x8x8 K = 32, the weights _init_params would set times 4: the softmax is near one-hot
The inputs of a case are regenerated from what the file holds of it — seed, shape, K and the recipe's parameters —
by tests/helpers/netvlad_grad_ref (draw_inputs / draw_tuple_inputs / draw_trained_inputs with K=...), on both sides.

Per case and quantity q in (vlad_raw, vlad_norm, dW, dC, dX; dX in NHWC) the file holds, from the float64 run,
  <case>.<q>       the flattened array at every STRIDE-th element (29: co-prime with every tile size), float64
  <case>.<q>_max   max |q| over the FULL array: the denominator of the relative max-norm
and <case>.ref_err[5]: max |fp32 run - float64 run| / max |float64 run| over the full arrays, the reference's own
fp32 error — the unit of the device test's bars (8 x).  The float64 run is checked against the numpy float64 helper
(<= 1e-11 in the same norm).
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
from helpers.netvlad_k_cases import CASES, QUANTITIES, STRIDE, draw_case  # noqa: E402

OUT = ROOT / "tests" / "golden" / "netvlad_k.npz"


class _StubBase(torch.nn.Module):
    def forward(self, x):
        return x.amax((2, 3)), x


def _reference(ref_netvlad, K, x, w, c, G, normalize, dtype):
    """The reference's layer and EmbedNet over the stub base in `dtype`: the five quantities as float64 arrays."""
    layer = ref_netvlad.NetVLAD(num_clusters=K, dim=512, normalize_input=normalize).to(dtype)
    with torch.no_grad():
        layer.conv.weight.copy_(torch.from_numpy(w).to(dtype)[:, :, None, None])
        layer.centroids.copy_(torch.from_numpy(c).to(dtype))
    model = ref_netvlad.EmbedNet(_StubBase(), layer).train()
    xt = torch.from_numpy(x).to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    with torch.no_grad():
        raw = layer(xt.detach())
    _, vlad_x = model(xt)
    vlad_x.backward(torch.from_numpy(G).to(dtype))
    out = {"vlad_raw": raw, "vlad_norm": vlad_x.detach(), "dW": layer.conv.weight.grad.reshape(K, 512),
           "dC": layer.centroids.grad, "dX": xt.grad.permute(0, 2, 3, 1).contiguous()}
    return {k: v.double().numpy().copy() for k, v in out.items()}


def rel_max(got, want) -> float:
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl.models import netvlad as ref_netvlad

    torch.set_num_threads(8)
    arrays = {}
    for case in CASES:
        name = case["name"]
        x, w, c, G, info = draw_case(case)
        K, normalize = case["K"], case["normalize"]
        f64 = _reference(ref_netvlad, K, x, w, c, G, normalize, torch.float64)
        f32 = _reference(ref_netvlad, K, x, w, c, G, normalize, torch.float32)
        mine = ref.head_and_grads(x, w, c, G, normalize)
        for q, k in (("vlad_norm", "Y"), ("dW", "dW"), ("dC", "dC"), ("dX", "dX")):
            e = rel_max(mine[k].reshape(f64[q].shape), f64[q])
            # (dW tends to zero as the softmax saturates: two float64 evaluations of it agree to fewer digits)
            assert e <= (1e-7 if case["kind"] == "trained" and q == "dW" else 1e-11), (name, q, e)
        err = np.array([rel_max(f32[q], f64[q]) for q in QUANTITIES])
        print(name, " ".join(f"{q} {e:.3e}" for q, e in zip(QUANTITIES, err)),
              {k: (round(v, 4) if isinstance(v, float) else v) for k, v in info.items()})
        arrays[f"{name}.ref_err"] = err
        for q in QUANTITIES:
            arrays[f"{name}.{q}"] = np.ascontiguousarray(f64[q].ravel()[::STRIDE])
            arrays[f"{name}.{q}_max"] = np.abs(f64[q]).max()
        for k in ("seed", "K", "N", "h", "w", "normalize", "kind", "jitter", "sharpen"):
            arrays[f"{name}.{k}"] = np.asarray(case[k])
        for k, v in info.items():
            arrays[f"{name}.{k}"] = np.asarray(v)
    if OUT.exists():
        old = dict(np.load(OUT, allow_pickle=False))
        if old.keys() == arrays.keys() and all(np.array_equal(old[k], np.asarray(v)) for k, v in arrays.items()):
            print("reproduces the committed fixture,", OUT.stat().st_size, "bytes")
            return
    np.savez_compressed(OUT, **arrays)
    assert OUT.stat().st_size < 500_000, OUT.stat().st_size
    print("file", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
