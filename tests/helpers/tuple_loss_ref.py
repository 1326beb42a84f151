"""The tuple losses and the soft-label loss in numpy float64, with their gradients, written from the formulas in the
header of openibl_amd/csrc/loss.hip (not from the reference's text; tests/test_tuple_loss_cpu.py ties them to the
reference's own autograd through tests/golden/tuple_loss.npz), and the seeded inputs of the loss tests.

A tuple: anchor a, positive x_0, negatives x_1 .. x_M.  s_i = |a - x_i|^2 (sqdist), |a - x_i + 1e-6|^2 (triplet: torch's
pairwise_distance), <a, x_i> (dot);  z_i = -s_i (sqdist) | s_i / temp (dot).
  triplet     mean_{b,j} max(0, margin + sqrt(s_0) - sqrt(s_j))
  sare_joint  mean_b  -log_softmax(z_0 .. z_M)[0]
  sare_ind    mean_{b,j} -log_softmax(z_0, z_j)[0]
  soft label  (-softmax(t / tt) log_softmax(s / ts)).mean(0).sum();  d/ds = (softmax(s / ts) - softmax(t / tt)) / (B ts)
"""
from __future__ import annotations

import numpy as np
import torch

PD_EPS = 1e-6
SIGMA_POS = 0.45
MODES = {  # name -> (kind, score, margin, temp, which of the reference's trainers computes it)
    "triplet": ("triplet", "sqdist", 0.1 ** 0.5, 0.07, "Trainer"),
    "triplet_m03": ("triplet", "dot", 0.3, 0.07, "SFRSTrainer"),
    "joint_sqdist": ("sare_joint", "sqdist", 0.3, 0.07, "Trainer"),
    "joint_dot": ("sare_joint", "dot", 0.3, 0.07, "SFRSTrainer"),
    "ind_sqdist": ("sare_ind", "sqdist", 0.3, 0.07, "Trainer"),
    "ind_dot": ("sare_ind", "dot", 0.3, 0.07, "SFRSTrainer"),
}
# name -> (seed, B, M, L, strided)
CASES = {"b1m1l4": (901, 1, 1, 4, False), "b2m3l1000": (902, 2, 3, 1000, False),
         "b3m10l32768": (903, 3, 10, 32768, False), "b2m10l4096_regions": (904, 2, 10, 4096, True)}
# name -> (seed, B, J, temp_student, temp_teacher)
SOFT_CASES = {"b1j1": (911, 1, 1, 0.07, 0.07), "b3j90": (912, 3, 90, 0.07, 0.07), "b2j4096": (913, 2, 4096, 0.07, 0.07),
              "b1j1_t": (914, 1, 1, 0.07, 0.05), "b3j90_t": (915, 3, 90, 0.07, 0.05),
              "b2j4096_t": (916, 2, 4096, 0.07, 0.05)}


def rel_max(got, want) -> float:
    """max |got - want| / max |want| over the tensor (0 / 0 = 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    d, m = float(np.abs(got - want).max()), float(np.abs(want).max())
    return 0.0 if d == 0.0 else d / m if m > 0.0 else float("inf")


def sigmas(M: int) -> torch.Tensor:
    """Noise levels of a tuple's rows: anchor 0, positive 0.45, negative j 0.25 + 0.12 j."""
    return torch.tensor([0.0, SIGMA_POS] + [0.25 + 0.12 * j for j in range(M)], dtype=torch.float32)


def draw_rows(seed: int, B: int, M: int, L: int) -> np.ndarray:
    """x [B][2 + M][L] fp32: row i of tuple t = normalize(base_t + sigma_i noise_ti), base and noise standard normal."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn((B, 1, L), generator=g)
    noise = torch.randn((B, 2 + M, L), generator=g)
    x = base + sigmas(M)[None, :, None] * noise
    return torch.nn.functional.normalize(x, dim=-1).numpy()


def draw_regions(seed: int, B: int, M: int, L: int):
    """The SFRS layout: vec [B][2 + M][9][L] fp32 (rows as draw_rows, fresh noise for each of the 9 regions) and the
    score [B][M][9] fp32 whose argmax names the region of every negative."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn((B, 1, 1, L), generator=g)
    noise = torch.randn((B, 2 + M, 9, L), generator=g)
    vec = torch.nn.functional.normalize(base + sigmas(M)[None, :, None, None] * noise, dim=-1)
    score = torch.rand((B, M, 9), generator=g) * 0.3 + 0.2
    return vec.numpy(), score.numpy()


def select_regions(vec: np.ndarray, score: np.ndarray):
    """(anchors [B][L], positives [B][L], negatives [B][M][L], region [B][M]) of draw_regions' layout: region 0 of the
    anchor and of the positive, the region with the highest score of every negative."""
    arg = score.argmax(-1)
    B, M = arg.shape
    neg = vec[np.arange(B)[:, None], 2 + np.arange(M)[None, :], arg]
    return vec[:, 0, 0], vec[:, 1, 0], neg, arg


def case_rows(name: str):
    """(anchors, positives, negatives) fp32 of a case of CASES, compact."""
    seed, B, M, L, strided = CASES[name]
    if strided:
        return select_regions(*draw_regions(seed, B, M, L))[:3]
    x = draw_rows(seed, B, M, L)
    return x[:, 0], x[:, 1], x[:, 2:]


def draw_soft(seed: int, B: int, J: int):
    """Student and teacher scores [B][J] fp32, uniform in (0.2, 0.5): the range of region similarities."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, J), generator=g) * 0.3 + 0.2).numpy(), (torch.rand((B, J), generator=g) * 0.3 + 0.2).numpy()


def scores(a, p, n, kind: str, score: str):
    """s [B][1 + M] float64 and the differences d [B][1 + M][L] (None for the dot score)."""
    a, p, n = (np.asarray(t, dtype=np.float64) for t in (a, p, n))
    x = np.concatenate((p[:, None], n), axis=1)
    if kind != "triplet" and score == "dot":
        return np.einsum("bl,bil->bi", a, x), None, x
    d = a[:, None] - x + (PD_EPS if kind == "triplet" else 0.0)
    return (d * d).sum(-1), d, x


def hinge_arguments(a, p, n, margin: float) -> np.ndarray:
    """margin + |a - p + eps| - |a - n_j + eps|, [B][M]."""
    s, _, _ = scores(a, p, n, "triplet", "sqdist")
    return margin + np.sqrt(s[:, :1]) - np.sqrt(s[:, 1:])


def tuple_loss(a, p, n, kind: str, score: str = "sqdist", margin: float = 0.3, temp: float = 0.07):
    """-> (loss, grad_a [B][L], grad_p [B][L], grad_n [B][M][L]) in float64."""
    s, d, x = scores(a, p, n, kind, score)
    a = np.asarray(a, dtype=np.float64)
    B, M = s.shape[0], s.shape[1] - 1
    u = np.zeros_like(s)
    if kind == "triplet":
        dist = np.sqrt(s)
        h = margin + dist[:, :1] - dist[:, 1:]
        on = h >= 0.0
        loss = np.where(on, h, 0.0).sum() / (B * M)
        u[:, 1:] = on / (B * M * dist[:, 1:])
        u[:, 0] = -on.sum(1) / (B * M * dist[:, 0])
    else:
        dot = score == "dot"
        z = s / temp if dot else -s
        if kind == "sare_joint":
            zs = z - z.max(1, keepdims=True)
            e = np.exp(zs)
            q = e / e.sum(1, keepdims=True)
            loss = (np.log(e.sum(1)) - zs[:, 0]).sum() / B
            w = q / B
        elif kind == "sare_ind":
            t = z[:, 1:] - z[:, :1]
            loss = (np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))).sum() / (B * M)
            w = np.zeros_like(z)
            w[:, 1:] = 1.0 / (1.0 + np.exp(-t)) / (B * M)
        else:
            raise ValueError(kind)
        w[:, 0] = -w[:, 1:].sum(1)
        u = w / temp if dot else 2.0 * w
    if d is None:
        gx = u[:, :, None] * a[:, None]
        ga = np.einsum("bi,bil->bl", u, x)
    else:
        gx = u[:, :, None] * d
        ga = -gx.sum(1)
    return float(loss), ga, gx[:, 0], gx[:, 1:]


def soft_label_loss(student, teacher, temp_student: float, temp_teacher: float):
    """-> (loss, grad_student [B][J]) in float64."""
    s = np.asarray(student, dtype=np.float64) / temp_student
    t = np.asarray(teacher, dtype=np.float64) / temp_teacher
    s = s - s.max(1, keepdims=True)
    t = t - t.max(1, keepdims=True)
    log_p = s - np.log(np.exp(s).sum(1, keepdims=True))
    q = np.exp(t) / np.exp(t).sum(1, keepdims=True)
    B = s.shape[0]
    return float((-q * log_p).mean(0).sum()), (np.exp(log_p) - q) / (B * temp_student)


def sample(t: np.ndarray, count: int = 400) -> np.ndarray:
    """Every stride-th element of the flattened tensor, the stride odd and such that about `count` remain."""
    flat = np.asarray(t).ravel()
    stride = max(1, flat.size // count) | 1
    return np.ascontiguousarray(flat[::stride])
