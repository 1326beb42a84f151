"""Generate tests/golden/conv5_backward.npz by running THE REFERENCE's conv5 layers and its EmbedNet under torch
autograd in fp32 on the CPU.

Run in the build container only (`python tests/helpers/make_conv5_backward_golden.py`): the reference tree is imported
through oracle.refshim, exactly as oracle/make_golden.py does, and does not exist on the GPU box.

Layer cases, (N, h, w) = (2, 2, 3) and (3, 5, 7): the reference's own `VGG(16, pretrained=False).base[24:]` (conv5_1,
ReLU, conv5_2, ReLU, conv5_3: ibl/models/vgg.py:41-42) with the drawn weights of tests/helpers/conv_grad_ref
.draw_inputs loaded, `y.backward(G)`.  Stored per case: the three bias gradients and grad_in in full (NHWC), y at a
channel stride, each weight gradient for output channels 0..3, and `ref_err`: the rel-L2 error of the reference's fp32 result against the
float64 helper for dX, dW1..3, db1..3 (over the FULL tensors).

End-to-end case: the reference's EmbedNet(vgg16(pretrained=False), NetVLAD(64, 512)) with synth.embednetpca_state(0)
on synth.images(12, 32, 48, seed) as 3 tuples x 4 images, Trainer._get_loss(vlad, 'triplet', 3, 4) with the scripts'
margin 0.1 ** 0.5, loss.backward().  Stored: the same slices of the six conv5 gradients, every 8th cluster row of
NetVLAD's dW / dC, the loss, vlad_x at a column stride, and `ref_err` for dW1..3, db1..3, dWv, dCv (over the FULL
tensors).  Random fp32 data does not compress: the strides keep the file under 1 MB.

The generator asserts every ref_err <= 1.25e-5: the device tests' bars are 8 x these figures, capped at 1e-4.
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
from helpers import conv_grad_ref as ref  # noqa: E402

OUT = ROOT / "tests" / "golden" / "conv5_backward.npz"
LAYER_CASES = ((51, 2, 2, 3), (52, 3, 5, 7))
E2E = dict(seed=77, B=3, n=4, H=32, W=48)
VLAD_STRIDE = 64
Y_STRIDE = 8
HEAD_STRIDE = 8
REF_ERR_MAX = 1.25e-5


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import models as ref_models
    from ibl.trainers import Trainer
    from openibl_amd import synth

    torch.set_num_threads(8)
    store = {}
    for seed, N, h, w in LAYER_CASES:
        x, ws, bs, G = ref.draw_inputs(seed, N, h, w)
        torch.manual_seed(0)
        tail = ref_models.create("vgg16", pretrained=False).base[24:]
        convs = [m for m in tail if isinstance(m, torch.nn.Conv2d)]
        assert len(tail) == 5 and len(convs) == 3
        with torch.no_grad():
            for c, wi, bi in zip(convs, ws, bs):
                c.weight.copy_(torch.from_numpy(wi))
                c.bias.copy_(torch.from_numpy(bi))
        xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        y = tail(xt)
        y.backward(torch.from_numpy(G).permute(0, 3, 1, 2).contiguous())
        got = {"y": y.detach().permute(0, 2, 3, 1).contiguous().numpy(),
               "dX": xt.grad.permute(0, 2, 3, 1).contiguous().numpy()}
        for i, c in enumerate(convs):
            got[f"dW{i + 1}"] = c.weight.grad.numpy()
            got[f"db{i + 1}"] = c.bias.grad.numpy()
        want = ref.chain_grads(x, ws, bs, G)
        err = np.array([ref.rel_l2(got[k], want[k]) for k in ref.GRAD_KEYS])
        name = f"layer_{N}x{h}x{w}"
        print(name, "y", f"{ref.rel_l2(got['y'], want['y']):.3e}",
              " ".join(f"{k} {v:.3e}" for k, v in zip(ref.GRAD_KEYS, err)))
        assert err.max() <= REF_ERR_MAX, err
        store[f"{name}_seed"] = np.array(seed)
        store[f"{name}_shape"] = np.array([N, h, w, 512])
        store[f"{name}_y_stride"] = np.array(Y_STRIDE)
        store[f"{name}_y"] = np.ascontiguousarray(got["y"][..., ::Y_STRIDE])
        store[f"{name}_dX"] = got["dX"]
        for i in range(3):
            store[f"{name}_dW{i + 1}"] = np.ascontiguousarray(got[f"dW{i + 1}"][:ref.W_ROWS])
            store[f"{name}_db{i + 1}"] = got[f"db{i + 1}"]
        store[f"{name}_ref_err"] = err

    state = {k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")}
    B, n = E2E["B"], E2E["n"]
    images = synth.images(B * n, E2E["H"], E2E["W"], seed=E2E["seed"])
    torch.manual_seed(0)
    base = ref_models.create("vgg16", pretrained=False)
    pool = ref_models.create("netvlad", dim=base.feature_dim)
    model = ref_models.create("embednet", base, pool)
    model.load_state_dict(state)
    model.train()
    trainer = Trainer(model, margin=0.1 ** 0.5)
    _, vlad = model(images)
    loss = trainer._get_loss(vlad, "triplet", B, n)
    loss.backward()
    got = {"dWv": pool.conv.weight.grad.reshape(64, 512).numpy(), "dCv": pool.centroids.grad.numpy()}
    for i, li in enumerate((24, 26, 28)):
        got[f"dW{i + 1}"] = base.base[li].weight.grad.numpy()
        got[f"db{i + 1}"] = base.base[li].bias.grad.numpy()
    assert all(p.grad is not None for p in model.parameters())     # pretrained=False: the reference freezes nothing
    want = ref.embednet_grads(images, state, B, n)
    err = np.array([ref.rel_l2(got[k], want[k]) for k in ref.E2E_KEYS])
    print("e2e loss", float(loss), "float64", want["loss"], "vlad", f"{ref.rel_l2(vlad.detach().numpy(), want['vlad']):.3e}")
    print("e2e", " ".join(f"{k} {v:.3e}" for k, v in zip(ref.E2E_KEYS, err)))
    assert float(loss) > 0 and err.max() <= REF_ERR_MAX, err
    store["e2e_seed"] = np.array(E2E["seed"])
    store["e2e_shape"] = np.array([B, n, E2E["H"], E2E["W"]])
    store["e2e_loss"] = np.array(float(loss))
    store["e2e_vlad_stride"] = np.array(VLAD_STRIDE)
    store["e2e_vlad"] = np.ascontiguousarray(vlad.detach().numpy()[:, ::VLAD_STRIDE])
    store["e2e_head_stride"] = np.array(HEAD_STRIDE)
    store["e2e_dWv"] = np.ascontiguousarray(got["dWv"][::HEAD_STRIDE])
    store["e2e_dCv"] = np.ascontiguousarray(got["dCv"][::HEAD_STRIDE])
    for i in range(3):
        store[f"e2e_dW{i + 1}"] = np.ascontiguousarray(got[f"dW{i + 1}"][:ref.W_ROWS])
        store[f"e2e_db{i + 1}"] = got[f"db{i + 1}"]
    store["e2e_ref_err"] = err
    np.savez_compressed(OUT, **store)
    assert OUT.stat().st_size < 1_000_000, OUT.stat().st_size
    print("file", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
