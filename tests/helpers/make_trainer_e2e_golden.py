"""Generate tests/golden/trainer_e2e.npz by running THE REFERENCE's Trainer and SFRSTrainer end to end under torch
autograd on the CPU, in fp32 and — the same objects after .double() — in float64: every loss type, two tuples per
batch, SFRS generations 0 and 1, and three optimiser steps.

Run in the build container only (`python tests/helpers/make_trainer_e2e_golden.py`): the reference tree is imported
through oracle.refshim, exactly as tests/helpers/make_region_backward_golden.py does, and does not exist on the GPU box.

Common settings: the reference's own vgg16(pretrained=False) + NetVLAD(64, 512) with synth.embednetpca_state(0)
(without pca_layer) in train(); the layers below conv5 frozen as VGG.__init__ freezes them under pretrained weights
(`frozen` cases: the whole backbone); margin 0.1 ** 0.5; batch i of a case is
synth.images(B * per_tuple, H, W, seed + i).view(B, per_tuple, 3, H, W), what `_loader` of tests/test_gpu_trainers.py
draws.  SFRS batches: per_tuple = 2 + neg_num + n_diff = 6, inputs_easy = images 0..3 of every tuple, inputs_diff =
images 0, 4, 5; temp = [0.07, 0.06]; model_cache a deep copy of the student; loss = loss_hard + 0.5 loss_soft.

The reference's EmbedRegionNet cannot run with tuple_size > 1 (two of its .view calls raise).  This project defines
"T > 1 is the T = 1 result per tuple, stacked" (test_tuples_are_independent_and_batch_mates_do_not_matter), so a
tuple_size = 1 reference model is wrapped in `_PerTuple`, whose forward calls the reference once per tuple chunk and
concatenates the three outputs along dim 0; the wrapper is `model` / `model_cache` of the reference's unmodified
SFRSTrainer.

Single-step cases (SINGLE_TRAINER, SINGLE_SFRS): Trainer._forward(images [2][4][3][32][48], True, loss_type) for
'sare_ind', 'sare_joint' and 'sare_joint' with the backbone frozen; SFRSTrainer._forward(easy, diff, loss_type, gen) at
64 x 96 for the three loss types x gen 0, 1.  Stored per case: the float64 loss(es) and the fp32 ones, samples of the
float64 gradients dW1..3 (output channel 0), db1..3 (full), dWv, dCv (every 8th row) rounded to float32, and `ref_err`:
the reference's own fp32-against-float64 rel-L2 over the FULL tensors (`loss_ref_err`: relative, per loss).

Trajectory case (TRAJ): three iterations on three different batches — SFRSTrainer 'triplet', gen 1, lambda_soft 0.5 —
with the reference scripts' optimiser, SGD(momentum 0.9, weight_decay 1e-3) over the parameters that require
gradients, and the body of the reference's train(): _forward, zero_grad, backward, step.  Stored: the per-iteration
losses (float64 and fp32), their `loss_ref_err`, the chosen lr and the STALE losses: the float64 loss of every
iteration's batch under the INITIAL weights, what a cache that ignores optimizer.step() would produce.

Two things that were planned for this file are NOT in it, because the reference itself does not meet the conditions
below (`--findings` prints the figures):
  * a Trainer 'sare_ind' trajectory.  The synthetic images' descriptors are nearly equidistant, the loss sits at
    ln 2 = 0.6931 and hardly moves: at lr 1e-1 a stale step is 29 and 14 loss bars away in iterations 2 and 3 (0.2 and
    0.4 at 1e-3), and of 20 other seed triples none reached 100 in both;
  * the parameter UPDATES (after three steps minus initial) of either trajectory.  An fp32 parameter is rounded at
    every step, 2^-24 |p| per element, and with lr <= 1e-1 the update is 1e-4 .. 1e-3 of the parameter: the
    reference's own fp32 update is 9.3e-6 .. 1.25e-5 (conv5 weights), 5.6e-5 (biases), 7.8e-5 (NetVLAD conv) and
    1.6e-5 (centroids) off the float64 one at lr 1e-1 (SFRSTrainer; 2.3e-5 .. 8.0e-5 for Trainer), and 10 x / 100 x
    that at 1e-2 / 1e-3.

Asserted here (the fixture's contract):
  * every ref_err (gradients, losses) <= 1.25e-5: the device bars are min(8 x these, 1e-4);
  * no triplet hinge argument lies within 1e-3 of zero in float64, and every triplet case (every iteration of a
    triplet trajectory) has at least one active term;
  * generation 1: for every (tuple, negative) the float64 gap between the best and the second-best region score is
    >= 1e-3 (the project's own bound on a device score is 2.1e-4); the picks are stored, and the fp32 run makes the same;
  * sensitivity: lr starts at the scripts' 1e-3 and is raised by factors of 10 until the stale loss of iterations 2 and
    3 differs from the true one by >= 100 x that iteration's loss bar, max(1e-5, 8 |fp32 - float64| / float64), or the
    generator fails at lr > 1e-1.

Picks: with these weights and images the reference picks region 0 (the whole image) for every negative.
`--probe-picks` is the one attempt made at another pick: head parameters in the trained regime, built from
the case's own conv5 maps with netvlad_grad_ref._trained_params; it prints the picks and stores nothing.  Scores are
never altered and the reference's internals are never hooked.  The gather for non-zero regions is covered by the
`_regions` cases of tuple_loss.npz and by the spy in test_sfrs_trainer_train_steps_the_student_only.
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
from helpers import trainer_e2e_ref as cases  # noqa: E402
from helpers import tuple_loss_ref as tref  # noqa: E402
from helpers.trainer_e2e_ref import (HEAD_KEYS, ITERS, KEYS, LAMBDA_SOFT, LRS, MARGIN, MOMENTUM, SFRS_SHAPE,  # noqa: E402
                                     SINGLE_SFRS, SINGLE_TRAINER, TEMP, TRAINER_SHAPE, TRAJ, WEIGHT_DECAY, batch, split)

OUT = ROOT / "tests" / "golden" / "trainer_e2e.npz"
W_ROWS = 1
HEAD_STRIDE = 8
REF_ERR_MAX = 1.25e-5
HINGE_GAP = 1e-3
PICK_GAP = 1e-3
SENSITIVITY = 100.0
# loss_soft of the SFRS single-step cases by generation, float64 to 4 decimals: the figures the cases were specified
# with, reproduced here.  (The loss_hard figures given with them, 0.3471 | 0.7236 | 1.1390, are NOT: this generator gets
# 0.3175 | 0.6932 | 1.0988, and tests/test_trainer_e2e_golden_cpu.py recomputes these from the oracle to 1e-9.)
ISSUE_SOFT = {0: 2.4523, 1: 2.3266}


class _PerTuple(torch.nn.Module):
    """A tuple_size = 1 reference EmbedRegionNet run once per tuple, the three outputs concatenated along dim 0."""

    def __init__(self, model, tuples):
        super().__init__()
        self.model = model
        self.tuples = tuples

    def forward(self, x):
        outs = [self.model(chunk) for chunk in x.chunk(self.tuples)]
        return tuple(torch.cat(parts, dim=0) for parts in zip(*outs))


def rel_l2(got, want) -> float:
    return nref.rel_l2(got, want)


def part(k, a):
    """The stored sample of a gradient of tensor k."""
    return cases.part(k, a, W_ROWS, HEAD_STRIDE)


def build(ref_models, arch, dtype, frozen=False, tuples=1):
    """The reference model of a case in `dtype` and train(), and the dict of its trainable tensors by gradient key."""
    from openibl_amd import synth
    state = {k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")}
    torch.manual_seed(0)
    base = ref_models.create("vgg16", pretrained=False)
    pool = ref_models.create("netvlad", dim=base.feature_dim)
    model = ref_models.create(arch, base, pool, tuple_size=1) if arch == "embedregionnet" else \
        ref_models.create(arch, base, pool)
    model.load_state_dict(state)
    layers = list(base.base.children())
    for l in (layers if frozen else layers[:24]):          # VGG.__init__ under pretrained weights, train_layers conv5
        for p in l.parameters():
            p.requires_grad = False
    model = model.to(dtype).train()
    tensors = {"dWv": pool.conv.weight, "dCv": pool.centroids}
    if not frozen:
        for i, li in enumerate((24, 26, 28)):
            tensors[f"dW{i + 1}"], tensors[f"db{i + 1}"] = base.base[li].weight, base.base[li].bias
    assert {id(p) for p in model.parameters() if p.requires_grad} == {id(p) for p in tensors.values()}
    if arch == "embedregionnet":
        model = _PerTuple(model, tuples).train()
    return model, tensors


def as_matrix(k, t):
    t = t.detach().numpy().astype(np.float64)
    return t.reshape(64, 512) if k == "dWv" else t


def grads_of(tensors):
    return {k: as_matrix(k, p.grad).copy() for k, p in tensors.items()}


def sfrs_probe(model, easy, margin, gen):
    """What the hard loss of this model on this batch stands on, under no_grad through the model's own forward:
    (picks [B][neg], pick gaps [B][neg], hinge arguments [B][neg] of the triplet loss on the picked regions)."""
    B, n = easy.shape[:2]
    with torch.no_grad():
        sim, vlad_a, vlad_b = model(easy.view(B * n, *easy.shape[2:]))
    score = sim[:, 1:, 0].double().numpy()                          # [B][neg][9]
    order = np.sort(score, axis=-1)
    picks, gaps = score.argmax(-1), order[..., -1] - order[..., -2]
    if gen == 0:
        picks = np.zeros_like(picks)
    vb = vlad_b.double().numpy()
    neg = vb[np.arange(B)[:, None], 1 + np.arange(n - 2)[None, :], picks]
    hinge = tref.hinge_arguments(vlad_a[:, 0, 0].double().numpy(), vb[:, 0, 0], neg, margin)
    return picks, gaps, hinge


def check_probe(name, loss_type, gen, probe):
    picks, gaps, hinge = probe
    if gen == 1:
        assert gaps.min() >= PICK_GAP, (name, gaps)
    if loss_type == "triplet":
        assert np.abs(hinge).min() >= HINGE_GAP and (hinge > 0).any(), (name, hinge)


def trainer_single(ref_models, Trainer, loss_type, frozen, dtype):
    model, tensors = build(ref_models, "embednet", dtype, frozen)
    loss = Trainer(model, margin=MARGIN)._forward(batch(TRAINER_SHAPE, 0).to(dtype), True, loss_type)
    loss.backward()
    assert all(p.grad is None for p in model.parameters() if not p.requires_grad)
    return {"losses": np.array([float(loss.detach())]), **grads_of(tensors)}


def sfrs_models(ref_models, dtype):
    B = SFRS_SHAPE["B"]
    model, tensors = build(ref_models, "embedregionnet", dtype, tuples=B)
    cache = copy.deepcopy(model).train()
    return model, cache, tensors


def sfrs_single(ref_models, SFRSTrainer, loss_type, gen, dtype):
    model, cache, tensors = sfrs_models(ref_models, dtype)
    trainer = SFRSTrainer(model, cache, margin=MARGIN, neg_num=SFRS_SHAPE["neg_num"], temp=TEMP)
    easy, diff = split(batch(SFRS_SHAPE, 0).to(dtype), SFRS_SHAPE["neg_num"])
    probe = sfrs_probe(model, easy, MARGIN, gen)
    loss_hard, loss_soft = trainer._forward(easy, diff, loss_type, gen)
    (loss_hard + LAMBDA_SOFT * loss_soft).backward()
    assert all(p.grad is None for p in cache.parameters())
    return {"losses": np.array([float(loss_hard.detach()), float(loss_soft.detach())]), "probe": probe,
            **grads_of(tensors)}


def trajectory(ref_models, trainers, which, loss_type, gen, lr, dtype, step=True):
    """ITERS iterations of the body of the reference's train().  step=False: every batch under the INITIAL weights
    (the stale losses).  -> losses [ITERS][1 or 2], updates by key, the probes of the SFRS iterations."""
    if which == "Trainer":
        model, tensors = build(ref_models, "embednet", dtype)
        trainer = trainers.Trainer(model, margin=MARGIN)
    else:
        model, cache, tensors = sfrs_models(ref_models, dtype)
        trainer = trainers.SFRSTrainer(model, cache, margin=MARGIN, neg_num=SFRS_SHAPE["neg_num"], temp=TEMP)
        cache_before = [p.detach().clone() for p in cache.parameters()]
    initial = {k: as_matrix(k, p).copy() for k, p in tensors.items()}
    optimizer = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=lr, momentum=MOMENTUM,
                                weight_decay=WEIGHT_DECAY)
    trainer.model.train()
    losses, probes = [], []
    for i in range(ITERS):
        if which == "Trainer":
            loss = trainer._forward(batch(TRAINER_SHAPE, i).to(dtype), True, loss_type)
            losses.append([float(loss.detach())])
        else:
            easy, diff = split(batch(SFRS_SHAPE, i).to(dtype), SFRS_SHAPE["neg_num"])
            probes.append(sfrs_probe(model, easy, MARGIN, gen))
            loss_hard, loss_soft = trainer._forward(easy, diff, loss_type, gen)
            loss = loss_hard + loss_soft * LAMBDA_SOFT
            losses.append([float(loss_hard.detach()), float(loss_soft.detach())])
        if step:
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
    if which != "Trainer":
        assert all(torch.equal(p.detach(), q) for p, q in zip(cache.parameters(), cache_before))
    return np.array(losses), {k: as_matrix(k, p) - initial[k] for k, p in tensors.items()}, probes


def total(losses):
    """[ITERS][1 or 2] -> the loss that is differentiated, per iteration: loss | loss_hard + 0.5 loss_soft."""
    return losses[:, 0] if losses.shape[1] == 1 else losses[:, 0] + LAMBDA_SOFT * losses[:, 1]


def loss_bars(l32, l64):
    """max(1e-5, 8 x the reference's fp32-against-float64 difference), relative, elementwise."""
    return np.maximum(1e-5, 8.0 * np.abs(l32 - l64) / np.abs(l64))


def store_single(store, name, shape, got, want, keys):
    err = np.array([rel_l2(got[k], want[k]) for k in keys])
    lerr = np.abs(got["losses"] - want["losses"]) / np.abs(want["losses"])
    print(name, "losses", got["losses"], "float64", want["losses"], "loss err", lerr)
    print("  ", " ".join(f"{k} {v:.3e}" for k, v in zip(keys, err)))
    assert (want["losses"] > 0).all() and err.max() <= REF_ERR_MAX and lerr.max() <= REF_ERR_MAX, (name, err, lerr)
    store[f"{name}_shape"] = np.array(shape)
    store[f"{name}_losses"], store[f"{name}_losses32"] = want["losses"], got["losses"]
    store[f"{name}_loss_ref_err"], store[f"{name}_ref_err"] = lerr, err
    for k in keys:
        store[f"{name}_{k}"] = part(k, want[k]).astype(np.float32)


def probe_picks(ref_models):
    """The one attempt at a generation-1 pick other than region 0: the head in the trained regime."""
    model, _, _ = sfrs_models(ref_models, torch.float64)
    easy, _ = split(batch(SFRS_SHAPE, 0).double(), SFRS_SHAPE["neg_num"])
    inner = model.model
    with torch.no_grad():
        _, feat = inner.base_model(easy.view(-1, *easy.shape[2:]))
    N, C, h, w = feat.shape
    x = feat.permute(0, 2, 3, 1).reshape(N, h * w, C).numpy().astype(np.float32)
    rs = np.random.RandomState(0)
    centres = rs.randn(64, C)
    d = x.reshape(-1, C).astype(np.float64)
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    cn = centres / np.sqrt((centres * centres).sum(1, keepdims=True))
    labels = (d @ cn.T).argmax(1).reshape(N, h * w)             # each pixel to its nearest random direction
    wv, cv, alpha, _ = nref._trained_params(x, centres, labels, 1.0)
    with torch.no_grad():
        inner.net_vlad.conv.weight.copy_(torch.from_numpy(wv).double()[:, :, None, None])
        inner.net_vlad.centroids.copy_(torch.from_numpy(cv).double())
    picks, gaps, _ = sfrs_probe(model, easy, MARGIN, 1)
    print(f"trained-regime head (alpha {alpha:.1f}): picks {picks.tolist()}, gaps {np.round(gaps, 4).tolist()}")


def search_lr(ref_models, trainers, name, which, loss_type, gen):
    """lr from the scripts' 1e-3 upwards by factors of 10, until the stale losses of iterations 2 and 3 are SENSITIVITY
    loss bars away or LRS is used up -> (lr, float64 losses, fp32 losses, stale losses, the sensitivity ratios per
    iteration, the float64 and fp32 probes, the update errors of the fp32 run by key)."""
    f32, f64 = torch.float32, torch.float64
    stale, _, _ = trajectory(ref_models, trainers, which, loss_type, gen, LRS[0], f64, step=False)
    for lr in LRS:
        l64, u64, probes = trajectory(ref_models, trainers, which, loss_type, gen, lr, f64)
        l32, u32, probes32 = trajectory(ref_models, trainers, which, loss_type, gen, lr, f32)
        bars = loss_bars(total(l32), total(l64))
        ratio = np.abs(total(l64) - total(stale)) / (bars * np.abs(total(l64)))
        uerr = {k: rel_l2(u32[k], u64[k]) for k in KEYS}
        print(f"{name} lr {lr:g}: losses {l64.tolist()} stale {stale.tolist()} bars {bars} sensitivity {ratio[1:]}")
        print("   fp32 update error", " ".join(f"{k} {v:.3e}" for k, v in uerr.items()))
        if ratio[1:].min() >= SENSITIVITY:
            break
    return lr, l64, l32, stale, ratio, probes, probes32, uerr


def findings(ref_models, trainers):
    """The figures behind the two parts of the issue this fixture does not hold (see the module docstring)."""
    search_lr(ref_models, trainers, "Trainer trajectory", "Trainer", "sare_ind", None)
    search_lr(ref_models, trainers, "SFRSTrainer trajectory", "SFRSTrainer", "triplet", 1)


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import models as ref_models
    from ibl import trainers

    torch.set_num_threads(8)
    if "--probe-picks" in sys.argv:
        return probe_picks(ref_models)
    if "--findings" in sys.argv:
        return findings(ref_models, trainers)
    f32, f64 = torch.float32, torch.float64
    store = {"head_stride": np.array(HEAD_STRIDE), "w_rows": np.array(W_ROWS), "margin": np.array(MARGIN),
             "temp": np.array(TEMP), "lambda_soft": np.array(LAMBDA_SOFT),
             "sgd": np.array([MOMENTUM, WEIGHT_DECAY]),
             "trainer_shape": np.array([TRAINER_SHAPE[k] for k in ("B", "n", "H", "W", "seed")]),
             "sfrs_shape": np.array([SFRS_SHAPE[k] for k in ("B", "neg_num", "n_diff", "H", "W", "seed")])}

    for name, (loss_type, frozen) in SINGLE_TRAINER.items():
        got, want = (trainer_single(ref_models, trainers.Trainer, loss_type, frozen, dt) for dt in (f32, f64))
        store_single(store, name, [int(frozen)], got, want, HEAD_KEYS if frozen else KEYS)

    for name, (loss_type, gen) in SINGLE_SFRS.items():
        got, want = (sfrs_single(ref_models, trainers.SFRSTrainer, loss_type, gen, dt) for dt in (f32, f64))
        store_single(store, name, [gen], got, want, KEYS)
        check_probe(name, loss_type, gen, want["probe"])
        picks, gaps, hinge = want["probe"]
        assert np.array_equal(picks, got["probe"][0]), (name, picks, got["probe"][0])
        print("   picks", picks.tolist(), "pick gaps", gaps.round(4).tolist(), "hinges", hinge.round(4).tolist())
        store[f"{name}_picks"], store[f"{name}_pick_gap"], store[f"{name}_hinge"] = picks, gaps, hinge
        assert abs(want["losses"][1] - ISSUE_SOFT[gen]) < 1e-4, (name, want["losses"])

    for name, (which, loss_type, gen) in TRAJ.items():
        lr, l64, l32, stale, ratio, probes, probes32, _ = search_lr(ref_models, trainers, name, which, loss_type, gen)
        if ratio[1:].min() < SENSITIVITY:
            raise AssertionError(f"{name}: a stale second step is not {SENSITIVITY:g} bars away at lr <= {LRS[-1]:g}")
        assert np.array_equal(stale[0], l64[0])
        lerr = np.abs(l32 - l64) / np.abs(l64)
        print("   loss err", lerr.tolist())
        assert lerr.max() <= REF_ERR_MAX, (name, lerr)
        for i, (p64, p32) in enumerate(zip(probes, probes32)):
            check_probe(f"{name} iteration {i}", loss_type, gen, p64)
            assert np.array_equal(p64[0], p32[0])
        store[f"{name}_picks"] = np.stack([p[0] for p in probes])
        store[f"{name}_pick_gap"] = np.stack([p[1] for p in probes])
        store[f"{name}_hinge"] = np.stack([p[2] for p in probes])
        print("   picks", store[f"{name}_picks"].tolist(), "min pick gap", store[f"{name}_pick_gap"].min(),
              "hinges", store[f"{name}_hinge"].round(4).tolist())
        store[f"{name}_lr"], store[f"{name}_iters"] = np.array(lr), np.array(ITERS)
        store[f"{name}_losses"], store[f"{name}_losses32"], store[f"{name}_stale"] = l64, l32, stale
        store[f"{name}_sensitivity"] = ratio
        store[f"{name}_loss_ref_err"] = lerr

    np.savez_compressed(OUT, **store)
    assert OUT.stat().st_size < 1_000_000, OUT.stat().st_size
    print("file", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
