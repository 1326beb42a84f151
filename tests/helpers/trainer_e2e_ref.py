"""The cases of tests/golden/trainer_e2e.npz (written by tests/helpers/make_trainer_e2e_golden.py from the reference's
own trainers), their batches, and the float64 losses of those cases recomputed from pieces the suite already trusts:
oracle.descriptor for the backbone and the head, helpers/region_ref.py for the region vectors and scores,
helpers/tuple_loss_ref.py for the losses.  Nothing here imports the reference.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np
import torch

from helpers import region_ref
from helpers import tuple_loss_ref as tref
from oracle import descriptor as od

KEYS = ("dW1", "dW2", "dW3", "db1", "db2", "db3", "dWv", "dCv")
HEAD_KEYS = ("dWv", "dCv")
MARGIN = 0.1 ** 0.5
TEMP = [0.07, 0.06]
LAMBDA_SOFT = 0.5
MOMENTUM, WEIGHT_DECAY = 0.9, 1e-3
LRS = (1e-3, 1e-2, 1e-1)
ITERS = 3
TRAINER_SHAPE = dict(B=2, n=4, H=32, W=48, seed=40)
SFRS_SHAPE = dict(B=2, neg_num=2, n_diff=2, H=64, W=96, seed=50)
# name -> (loss_type, frozen backbone)
SINGLE_TRAINER = {"trainer_sare_ind": ("sare_ind", False), "trainer_sare_joint": ("sare_joint", False),
                  "trainer_sare_joint_frozen": ("sare_joint", True)}
# name -> (loss_type, gen)
SINGLE_SFRS = {f"sfrs_{lt}_g{gen}": (lt, gen) for lt in ("triplet", "sare_ind", "sare_joint") for gen in (0, 1)}
# name -> (trainer, loss_type, gen)
TRAJ = {"traj_sfrs": ("SFRSTrainer", "triplet", 1)}


def per_tuple(shape) -> int:
    return shape["n"] if "n" in shape else 2 + shape["neg_num"] + shape["n_diff"]


def batch(shape, i):
    """Batch i of a case, [B][per_tuple][3][H][W] fp32: what `_loader` of tests/test_gpu_trainers.py yields."""
    from openibl_amd import synth
    per = per_tuple(shape)
    x = synth.images(shape["B"] * per, shape["H"], shape["W"], seed=shape["seed"] + i)
    return x.view(shape["B"], per, 3, shape["H"], shape["W"])


def split(imgs, neg_num):
    """SFRSTrainer._parse_data without its .cuda: (inputs_easy, inputs_diff), contiguous."""
    return imgs[:, :neg_num + 2].contiguous(), torch.cat((imgs[:, :1], imgs[:, neg_num + 2:]), dim=1).contiguous()


def part(k, a, w_rows, head_stride):
    """The stored sample of a gradient of tensor k: the first output channels of a conv5 weight, every n-th row of
    the NetVLAD tensors ([64][512]), a bias in full."""
    a = np.asarray(a)
    return np.ascontiguousarray(a[:w_rows] if k in ("dW1", "dW2", "dW3") else a[::head_stride] if k in HEAD_KEYS else a)


def conv5_maps(images, sd):
    """[N][3][H][W] -> the float64 conv5_3 maps [N][512][H/16][W/16]."""
    with torch.no_grad():
        return od.vgg16_conv5(images.double(), sd)


def _head(sd):
    return sd["net_vlad.conv.weight"].double().view(64, 512), sd["net_vlad.centroids"].double()


def trainer_loss64(feat, sd, B, n, loss_type, margin=MARGIN, temp=0.07) -> float:
    """Trainer._forward's loss from the maps of a [B][n] batch: the whole-image descriptor, the score -|a - x|^2."""
    w, c = _head(sd)
    v = od.normalize_vlad(od.netvlad(feat, w, c)).view(B, n, -1).numpy()
    return tref.tuple_loss(v[:, 0], v[:, 1], v[:, 2:], loss_type, "sqdist", margin, temp)[0]


def sfrs_losses64(feat_easy, feat_diff, sd, B, loss_type, gen, margin=MARGIN, temp=TEMP):
    """SFRSTrainer._forward's (loss_hard, loss_soft) with model_cache a copy of the student, tuple by tuple as the
    project defines tuple_size > 1, and the regions picked at generation >= 1 with their gaps to the runner-up:
    -> (loss_hard, loss_soft, picks [B][neg], gaps [B][neg])."""
    w, c = _head(sd)
    vec = region_ref.region_vectors(feat_easy, w, c)                       # [B (2 + neg)][9][L]
    score = region_ref.region_scores(vec, B)[:, 1:, 0].numpy()             # [B][neg][9]: the anchor's whole image
    order = np.sort(score, axis=-1)
    picks, gaps = score.argmax(-1), order[..., -1] - order[..., -2]
    if gen == 0:
        picks = np.zeros_like(picks)
    v = vec.view(B, -1, 9, vec.shape[-1]).numpy()
    neg = v[np.arange(B)[:, None], 2 + np.arange(picks.shape[1])[None, :], picks]
    hard = tref.tuple_loss(v[:, 0, 0], v[:, 1, 0], neg, loss_type, "dot", margin, temp[0])[0]
    sim = region_ref.region_scores(region_ref.region_vectors(feat_diff, w, c), B)[:, :, 0].reshape(B, -1).numpy()
    soft = tref.soft_label_loss(sim, sim, temp[0], temp[gen])[0]
    return hard, soft, picks, gaps
