"""Generate tests/golden/region_backward.npz by running THE REFERENCE's SFRS region head and SFRSTrainer under torch
autograd on the CPU, in fp32 and — the same objects after .double() — in float64.

Run in the build container only (`python tests/helpers/make_region_backward_golden.py`): the reference tree is imported
through oracle.refshim, exactly as oracle/make_golden.py does, and does not exist on the GPU box.

Head cases, through the reference's own EmbedRegionNet(stub base, NetVLAD(64, 512))._compute_region_sim
(ibl/models/netvlad.py:123-186) with tuple_size 1, the first map the anchor (inputs: tests/helpers/netvlad_grad_ref and
region_grad_ref from the stored seeds):
  trained_3x4x6    draw_trained_inputs, normalised input; loss = sum(vec G) + sum(score Gs), G and Gs of draw_G
  raw_3x4x6        draw_inputs, normalize_input=False; the same loss
  tuple_1x4x8x8    draw_tuple_inputs(seed, 1, 4, 8, 8, 0.1); the reference's SFRSTrainer loss at generation 0 from ONE
                   model call: SFRSTrainer._get_loss(A, P, Neg, 1, 'sare_ind') on region 0 (temp 0.07) + 0.5 x the soft
                   term of ibl/trainers.py:256-257 on score[:, :, 0] against the label of draw_label
Stored per case: every 7th element of dW and dC (row-major), dX at a pixel stride, Y at a column stride — the reference's fp32
autograd — and `ref_err`: the rel-L2 error of the fp32 dW | dC | dX against the float64 run, over the FULL tensors.

End-to-end case `e2e`: the reference's EmbedRegionNet(vgg16(pretrained=False), NetVLAD) in train() with
synth.embednetpca_state(0), model_cache a deep copy, synth.images(6, 64, 96, seed): inputs_easy = images 0..3 (one
tuple: anchor, positive, two negatives), inputs_diff = images 0, 4, 5.  The reference's own
SFRSTrainer(margin 0.1 ** 0.5, neg_num 2)._forward(easy, diff, 'triplet', gen=0), loss_hard + 0.5 loss_soft.  Stored:
the first two output channels of the three conv5 weight gradients, the three bias gradients, every 8th row of NetVLAD's
dW / dC — each from the fp32 run (`e2e_*`) and from the float64 run (`e2e64_*`: what the device test compares with; the
reference is not on the GPU box) — both losses of both runs and `e2e_ref_err` over the FULL tensors.

Scores cases (T, n) = (1, 1), (1, 3), (2, 2), (1, 10), L = 32768, inputs of draw_vectors: the error of torch's fp32
bmm backward (the product of netvlad.py:182, under sum(score Gs)) against float64, `scores_ref_err`.

The generator asserts every ref_err <= 1.25e-5: the device tests' bars are 8 x these figures, capped at 1e-4.
"""
from __future__ import annotations

import copy
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from oracle import refshim  # noqa: E402

refshim.install()  # puts the reference FIRST on sys.path: `import ibl` below is the reference

sys.path.insert(0, str(ROOT / "tests"))
from helpers import netvlad_grad_ref as nref  # noqa: E402
from helpers import region_grad_ref as ref  # noqa: E402

OUT = ROOT / "tests" / "golden" / "region_backward.npz"
HEAD_STRIDE = 8          # e2e: every 8th cluster row of NetVLAD's dW / dC
FLAT_STRIDE = 7          # head cases: every 7th ELEMENT of dW / dC (co-prime with 512: every row and column is sampled)
Y_STRIDE = 64
W_ROWS = 2
REF_ERR_MAX = 1.25e-5
# name -> (seed, kind, N, h, w, normalize, dx stride)
HEAD_CASES = {"trained_3x4x6": (71, "trained", 3, 4, 6, True, 5),
              "raw_3x4x6": (72, "raw", 3, 4, 6, False, 5),
              "tuple_1x4x8x8": (73, "tuple", 4, 8, 8, True, 7)}
TUPLE_JITTER = 0.1
E2E = dict(seed=79, H=64, W=96, neg_num=2)
SCORES_CASES = ((81, 1, 1), (82, 1, 3), (83, 2, 2), (84, 1, 10))
KEYS = ("dW", "dC", "dX")
E2E_KEYS = ("dW1", "dW2", "dW3", "db1", "db2", "db3", "dWv", "dCv")


class _StubBase(torch.nn.Module):
    def forward(self, x):
        return x.amax((2, 3)), x


def draw_head_case(name):
    seed, kind, N, h, w_, normalize, _ = HEAD_CASES[name]
    if kind == "trained":
        x, w, c, _, _ = nref.draw_trained_inputs(seed, N, h, w_)
    elif kind == "raw":
        x, w, c, _ = nref.draw_inputs(seed, N, h, w_)
    else:
        x, w, c, _, _ = nref.draw_tuple_inputs(seed, 1, N, h, w_, TUPLE_JITTER)
    return x, w, c


def _head_run(ref_netvlad, trainer, name, dtype):
    """One head case through the reference in `dtype`: Y, dW, dC, dX (NHWC) as numpy."""
    seed, kind, N, h, w_, normalize, _ = HEAD_CASES[name]
    x, w, c = draw_head_case(name)
    layer = ref_netvlad.NetVLAD(num_clusters=64, dim=512, normalize_input=normalize)
    with torch.no_grad():
        layer.conv.weight.copy_(torch.from_numpy(w)[:, :, None, None])
        layer.centroids.copy_(torch.from_numpy(c))
    model = ref_netvlad.EmbedRegionNet(_StubBase(), layer, tuple_size=1).train().to(dtype)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().to(dtype).requires_grad_(True)
    score, vlad_A, vlad_B = model._compute_region_sim(xt[:1], xt[1:])
    vec = torch.cat((vlad_A, vlad_B), dim=1)                     # [1][N][9][L]
    if kind == "tuple":
        label = torch.from_numpy(ref.draw_label(seed, 1, N - 1)).to(dtype)
        hard = trainer._get_loss(vlad_A[:, 0, 0], vlad_B[:, 0, 0], vlad_B[:, 1:, 0], 1, "sare_ind")
        log_sim = torch.nn.functional.log_softmax(score[:, :, 0].contiguous().view(1, -1) / trainer.temp[0], dim=1)
        soft = (-label * log_sim).mean(0).sum()
        loss = hard + 0.5 * soft
    else:
        G, Gs = ref.draw_G(seed + 100, N, 1)
        loss = (vec[0] * torch.from_numpy(G).to(dtype)).sum() + (score * torch.from_numpy(Gs).to(dtype)).sum()
    loss.backward()
    return {"Y": vec[0].detach().numpy(), "score": score.detach().numpy(), "loss": float(loss.detach()),
            "dW": layer.conv.weight.grad.reshape(64, 512).numpy().copy(), "dC": layer.centroids.grad.numpy().copy(),
            "dX": xt.grad.permute(0, 2, 3, 1).contiguous().numpy()}


def _e2e_run(ref_models, SFRSTrainer, dtype):
    from openibl_amd import synth
    state = {k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")}
    images = synth.images(6, E2E["H"], E2E["W"], seed=E2E["seed"]).to(dtype)
    torch.manual_seed(0)
    base = ref_models.create("vgg16", pretrained=False)
    pool = ref_models.create("netvlad", dim=base.feature_dim)
    model = ref_models.create("embedregionnet", base, pool, tuple_size=1)
    model.load_state_dict(state)
    model = model.to(dtype).train()
    cache = copy.deepcopy(model).train()
    trainer = SFRSTrainer(model, cache, margin=0.1 ** 0.5, neg_num=E2E["neg_num"], temp=[0.07, 0.07])
    easy = images[None, :4]
    diff = torch.cat((images[None, :1], images[None, 4:]), dim=1)
    loss_hard, loss_soft = trainer._forward(easy, diff, "triplet", 0)
    (loss_hard + 0.5 * loss_soft).backward()
    out = {"loss_hard": float(loss_hard.detach()), "loss_soft": float(loss_soft.detach()),
           "dWv": pool.conv.weight.grad.reshape(64, 512).numpy(), "dCv": pool.centroids.grad.numpy()}
    for i, li in enumerate((24, 26, 28)):
        out[f"dW{i + 1}"] = base.base[li].weight.grad.numpy()
        out[f"db{i + 1}"] = base.base[li].bias.grad.numpy()
    return out


def _e2e_part(k, a):
    return a[:W_ROWS] if k in ("dW1", "dW2", "dW3") else a[::HEAD_STRIDE] if k in ("dWv", "dCv") else a


def _scores_run(Y, Gs, T, dtype):
    v = torch.from_numpy(Y).to(dtype).requires_grad_(True)
    N, B, L = v.shape
    vv = v.view(T, -1, B, L)
    anchors, pairs = vv[:, :1].expand(T, N // T - 1, B, L), vv[:, 1:]
    score = torch.bmm(anchors.reshape(-1, B, L), pairs.reshape(-1, B, L).transpose(1, 2))
    (score.view(T, -1, B, B) * torch.from_numpy(Gs).to(dtype)).sum().backward()
    return v.grad.numpy()


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import models as ref_models
    from ibl.models import netvlad as ref_netvlad
    from ibl.trainers import SFRSTrainer

    torch.set_num_threads(8)
    store = {}
    trainer = SFRSTrainer(None, None, temp=[0.07])
    for name, (seed, kind, N, h, w_, normalize, dxs) in HEAD_CASES.items():
        got, want = _head_run(ref_netvlad, trainer, name, torch.float32), _head_run(ref_netvlad, trainer, name,
                                                                                      torch.float64)
        err = np.array([ref.rel_l2(got[k], want[k]) for k in KEYS])
        print(name, "loss", got["loss"], "float64", want["loss"], "Y", f"{ref.rel_l2(got['Y'], want['Y']):.3e}",
              " ".join(f"{k} {v:.3e}" for k, v in zip(KEYS, err)))
        assert err.max() <= REF_ERR_MAX, err
        store[f"{name}_seed"] = np.array(seed)
        store[f"{name}_shape"] = np.array([N, h, w_, 512])
        store[f"{name}_normalize_input"] = np.array(int(normalize))
        store[f"{name}_loss"] = np.array(got["loss"])
        store[f"{name}_y_stride"] = np.array(Y_STRIDE)
        store[f"{name}_Y"] = np.ascontiguousarray(got["Y"][:, :, ::Y_STRIDE])
        store[f"{name}_score"] = got["score"]
        store[f"{name}_head_stride"] = np.array(FLAT_STRIDE)
        store[f"{name}_dW"] = np.ascontiguousarray(got["dW"].ravel()[::FLAT_STRIDE])
        store[f"{name}_dC"] = np.ascontiguousarray(got["dC"].ravel()[::FLAT_STRIDE])
        store[f"{name}_dx_stride"] = np.array(dxs)
        store[f"{name}_dX"] = np.ascontiguousarray(got["dX"].reshape(N, h * w_, 512)[:, ::dxs])
        store[f"{name}_ref_err"] = err
    store["tuple_1x4x8x8_jitter"] = np.array(TUPLE_JITTER)

    got, want = _e2e_run(ref_models, SFRSTrainer, torch.float32), _e2e_run(ref_models, SFRSTrainer, torch.float64)
    err = np.array([ref.rel_l2(got[k], want[k]) for k in E2E_KEYS])
    print("e2e loss_hard", got["loss_hard"], want["loss_hard"], "loss_soft", got["loss_soft"], want["loss_soft"])
    print("e2e", " ".join(f"{k} {v:.3e}" for k, v in zip(E2E_KEYS, err)))
    assert got["loss_hard"] > 0 and err.max() <= REF_ERR_MAX, err
    store["e2e_seed"] = np.array(E2E["seed"])
    store["e2e_shape"] = np.array([6, E2E["H"], E2E["W"], E2E["neg_num"]])
    store["e2e_losses"] = np.array([got["loss_hard"], got["loss_soft"]])
    store["e2e64_losses"] = np.array([want["loss_hard"], want["loss_soft"]])
    store["e2e_head_stride"] = np.array(HEAD_STRIDE)
    store["e2e_w_rows"] = np.array(W_ROWS)
    for k in E2E_KEYS:
        store[f"e2e_{k}"] = np.ascontiguousarray(_e2e_part(k, got[k]))
        store[f"e2e64_{k}"] = np.ascontiguousarray(_e2e_part(k, want[k]))
    store["e2e_ref_err"] = err

    serr = []
    for seed, T, n in SCORES_CASES:
        Y, Gs = ref.draw_vectors(seed, T, n)
        e = ref.rel_l2(_scores_run(Y, Gs, T, torch.float32), _scores_run(Y, Gs, T, torch.float64))
        h = ref.rel_l2(ref.scores_backward(Y, Gs, T), _scores_run(Y, Gs, T, torch.float64))
        print(f"scores T={T} n={n}: fp32 bmm backward {e:.3e}; the float64 helper against torch float64 {h:.3e}")
        assert e <= REF_ERR_MAX and h <= 1e-12
        serr.append(e)
    store["scores_cases"] = np.array(SCORES_CASES)
    store["scores_ref_err"] = np.array(serr)
    np.savez_compressed(OUT, **store)
    assert OUT.stat().st_size < 1_000_000, OUT.stat().st_size
    print("file", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
