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


def scores(a, p, n, kind: str, score: str, dtype=np.float64):
    """s [B][1 + M] in `dtype` (float64, or np.longdouble for the extended-precision twin) and the differences
    d [B][1 + M][L] (None for the dot score)."""
    a, p, n = (np.asarray(t, dtype=dtype) for t in (a, p, n))
    x = np.concatenate((p[:, None], n), axis=1)
    if kind != "triplet" and score == "dot":
        return np.einsum("bl,bil->bi", a, x), None, x
    d = a[:, None] - x + (PD_EPS if kind == "triplet" else 0.0)
    return (d * d).sum(-1), d, x


def hinge_arguments(a, p, n, margin: float) -> np.ndarray:
    """margin + |a - p + eps| - |a - n_j + eps|, [B][M]."""
    s, _, _ = scores(a, p, n, "triplet", "sqdist")
    return margin + np.sqrt(s[:, :1]) - np.sqrt(s[:, 1:])


def coefficients(s, kind: str, score: str = "sqdist", margin: float = 0.3, temp: float = 0.07):
    """(loss, u [B][1 + M]) of the scores s, in the dtype of s: the table the forward kernel leaves."""
    with np.errstate(over="ignore", under="ignore"):         # exp(-800) = 0 and 1 / (1 + exp(800)) = 0 are meant
        return _coefficients(s, kind, score, margin, temp)


def _coefficients(s, kind, score, margin, temp):
    B, M = s.shape[0], s.shape[1] - 1
    u = np.zeros_like(s)
    if kind == "triplet":
        dist = np.sqrt(s)
        h = margin + dist[:, :1] - dist[:, 1:]
        on = h >= 0.0
        loss = np.where(on, h, 0.0).sum() / (B * M)
        u[:, 1:] = on / (B * M * dist[:, 1:])
        u[:, 0] = -on.sum(1) / (B * M * dist[:, 0])
        return loss, u
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
    return loss, (w / temp if dot else 2.0 * w)


def tuple_loss(a, p, n, kind: str, score: str = "sqdist", margin: float = 0.3, temp: float = 0.07, dtype=np.float64):
    """-> (loss, grad_a [B][L], grad_p [B][L], grad_n [B][M][L]) in `dtype` (the loss a Python float for float64)."""
    s, d, x = scores(a, p, n, kind, score, dtype)
    a = np.asarray(a, dtype=dtype)
    loss, u = coefficients(s, kind, score, margin, temp)
    if d is None:
        gx = u[:, :, None] * a[:, None]
        ga = np.einsum("bi,bil->bl", u, x)
    else:
        gx = u[:, :, None] * d
        ga = -gx.sum(1)
    return (float(loss) if dtype is np.float64 else loss), ga, gx[:, 0], gx[:, 1:]


def soft_label_loss(student, teacher, temp_student: float, temp_teacher: float, dtype=np.float64):
    """-> (loss, grad_student [B][J]) in `dtype`.  Both softmaxes are exp(x - max) / sum: identical tables at equal
    temperatures give a gradient of exactly zero."""
    s = np.asarray(student, dtype=dtype) / temp_student
    t = np.asarray(teacher, dtype=dtype) / temp_teacher
    s = s - s.max(1, keepdims=True)
    t = t - t.max(1, keepdims=True)
    with np.errstate(under="ignore"):
        zs = np.exp(s).sum(1, keepdims=True)
        log_p = s - np.log(zs)
        q = np.exp(t) / np.exp(t).sum(1, keepdims=True)
        B = s.shape[0]
        loss = (-q * log_p).mean(0).sum()
        return (float(loss) if dtype is np.float64 else loss), (np.exp(s) / zs - q) / (B * temp_student)


def sample(t: np.ndarray, count: int = 400) -> np.ndarray:
    """Every stride-th element of the flattened tensor, the stride odd and such that about `count` remain."""
    flat = np.asarray(t).ravel()
    stride = max(1, flat.size // count) | 1
    return np.ascontiguousarray(flat[::stride])


# ---- the edge suite (tests/test_gpu_tuple_loss_edges.py): limits, ragged shapes, saturation --------------------------
FP32_TERM = 2.0 ** -23          # one fp32 rounding (2^-24), doubled
UNDERFLOW = 1e-30               # a coefficient or a loss is exactly 0 or at least this: nothing in fp32's flush band
GAP_LOW, GAP_HIGH = 60.0, 800.0  # a logit gap is <= 60 (weight >= 1e-26) or >= 800 (exp underflows to exactly 0)
HINGE_GAP = 1e-3
HOT = 60.0                      # the score of a one-hot row of the soft-label cases: 60 / 0.07 = 857 above the rest

# name -> (seed, B, M, L, regime).  'rows': draw_rows with its hinges cleared (clear_hinges); 'r1' / 'r2': rows built
# to prescribed logits (draw_regime); 'r3': coincident rows; 'r4_mixed': one tuple switched off next to one switched on
EDGE_CASES = {
    "g1_b4m64l8": (921, 4, 64, 8, "rows"), "g1_b70m3l8": (922, 70, 3, 8, "rows"),
    "g1_b300m2l8": (923, 300, 2, 8, "rows"), "g1_b513m1l4": (924, 513, 1, 4, "rows"),
    "g2_b65535m1l4": (925, 65535, 1, 4, "rows"),
    **{f"g3_l{L}": (930 + i, 2, 3, L, "rows") for i, L in enumerate((2, 3, 5, 7, 33, 36, 8196, 8200, 513 * 4 - 1))},
    # one column: seeds at which the anchor's gradient does not cancel to (a rounding error around) zero in every tuple
    "g3_l1": (1005, 2, 3, 1, "rows"), "g4_l1": (1010, 2, 3, 1, "rows"),
    "g4_l33": (942, 2, 2, 33, "rows"), "g4_l36": (943, 2, 2, 36, "rows"), "g5_l1000": (944, 2, 3, 1000, "rows"),
    "r1": (951, 2, 6, 256, "r1"), "r2": (952, 2, 6, 256, "r2"), "r3": (953, 2, 6, 256, "r3"),
    "r4_off": (954, 2, 6, 256, "rows"), "r4_on": (954, 2, 6, 256, "rows"), "r4_mixed": (955, 2, 6, 256, "r4_mixed"),
    "r5": (956, 2, 6, 256, "rows"),
    "r1_big": (957, 2, 10, 32768, "r1"), "r2_big": (958, 2, 10, 32768, "r2"),
}
EDGE_MARGIN = {"r4_off": -10.0, "r4_on": 10.0}                  # every hinge inactive | active; triplet modes only
EDGE_TRIPLET_ONLY = ("r4_off", "r4_on", "r4_mixed")
# stored in tests/golden/tuple_loss_edges.npz.  'r4_off' is not: torch's triplet_margin_loss refuses a margin <= 0, so
# the reference cannot run it; its switched-off tuple next to a switched-on one ('r4_mixed') is stored
EDGE_GOLDEN = ("r1", "r2", "r3", "r4_on", "r4_mixed", "r5")
EDGE_SAMPLE = 150                                               # values stored per gradient (sample's count)
EDGE_SCALE = {"r5": -2.0}                                       # the upstream gradient of the stored gradients
# Logits of the negatives against the positive's (z_j - z_0), tuple b uses list b % 2, a case its first M entries.
# Measured from the row's largest logit every gap is <= 60 or >= 800, and so is every |z_j - z_0|.
R_TARGETS = {
    "r1": ((850, 845, 803, 30, -20, -810, 849, 40, -830, 802), (805, 801, 860, 55, -5, -55, 858, 20, -840, 810)),
    "r2": ((-3, -30, -55, -805, -850, -1700, -10, -45, -900, -1000),
           (-1, -20, -59, -801, -900, -1650, -5, -50, -1200, -810)),
}
REGIME_NORM = 8.0               # the norm of every row of the dot-score regimes: |z| = |<a, x>| / 0.07 <= 914
REGIME_TEMP = 0.07

# name -> (seed, B, J, temp_student, temp_teacher, regime).  'uniform': draw_soft; 'same': the student IS the teacher;
# the others put HOT into otherwise uniform rows: 'teacher_onehot', 'student_other' (both one-hot, different indices),
# 'both_same', 'mixed' (rows of the three kinds and a plain one in turn), 'same_sat': mixed rows, student = teacher
EDGE_SOFT = {
    **{f"s1_b3j{J}": (960 + i, 3, J, 0.07, 0.05, "uniform") for i, J in enumerate((2, 255, 256, 257, 511, 513))},
    "s1_b300j3": (966, 300, 3, 0.07, 0.05, "uniform"), "s1_b257j1": (967, 257, 1, 0.07, 0.05, "uniform"),
    "s1_b65535j1": (968, 65535, 1, 0.07, 0.05, "uniform"),
    **{f"s2_{r}{tag}": (970 + 4 * k + i, 3 if r != "mixed" else 8, 90 if r != "mixed" else 300, 0.07, tt, r)
       for k, (tag, tt) in enumerate((("", 0.07), ("_t", 0.05)))
       for i, r in enumerate(("teacher_onehot", "student_other", "both_same", "mixed"))},
    **{f"s3_b3j{J}": (980 + i, 3, J, 0.07, 0.07, "same") for i, J in enumerate((2, 255, 256, 257, 511, 513))},
    "s3_b300j3": (986, 300, 3, 0.07, 0.07, "same"), "s3_b257j1": (987, 257, 1, 0.07, 0.07, "same"),
    "s3_sat": (988, 8, 300, 0.07, 0.07, "same_sat"),
}
EDGE_SOFT_GOLDEN = tuple(k for k in EDGE_SOFT if k != "s1_b65535j1")

_edge_cache = {}


def clear_hinges(x: np.ndarray, margins=(0.1 ** 0.5, 0.3), gap: float = 2.0 * HINGE_GAP) -> np.ndarray:
    """x [B][2 + M][L] fp32, in place: a negative whose hinge argument lies within `gap` of 0 under either margin is
    scaled by 1.25 until none does (thousands of tuples cannot all miss the band by the choice of a seed)."""
    for _ in range(20):
        bad = np.zeros((x.shape[0], x.shape[1] - 2), dtype=bool)
        for m in margins:
            bad |= np.abs(hinge_arguments(x[:, 0], x[:, 1], x[:, 2:], m)) < gap
        if not bad.any():
            return x
        x[:, 2:][bad] *= np.float32(1.25)
    raise AssertionError("clear_hinges did not settle")


def draw_regime(seed: int, B: int, M: int, L: int, regime: str, score: str) -> np.ndarray:
    """x [B][2 + M][L] fp32 whose logits are R_TARGETS[regime] up to the fp32 rounding of the rows.
    dot:    a = 8 e, x_i = alpha_i e + sqrt(64 - alpha_i^2) r_i with r_i a unit vector orthogonal to e, so that
            <a, x_i> / 0.07 = z_i, the z_i centred on 0: every row has norm 8.
    sqdist: a standard normal (unnormalised), x_i = a + sqrt(D_i) r_i with r_i a unit vector: |a - x_i|^2 = D_i,
            D_i = 50 + max_k z_k - z_i (from 50 up to about 1.8e3)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn((B, 1, L), generator=g, dtype=torch.float64).numpy()
    noise = torch.randn((B, 1 + M, L), generator=g, dtype=torch.float64).numpy()
    t = np.array([[0.0] + [float(v) for v in R_TARGETS[regime][b % 2][:M]] for b in range(B)])
    if score == "dot":
        e = base / np.linalg.norm(base, axis=-1, keepdims=True)
        r = noise - (noise * e).sum(-1, keepdims=True) * e
        r /= np.linalg.norm(r, axis=-1, keepdims=True)
        z = t - 0.5 * (t.max(1, keepdims=True) + t.min(1, keepdims=True))
        alpha = (z * REGIME_TEMP / REGIME_NORM)[:, :, None]
        assert np.abs(alpha).max() < REGIME_NORM
        a, x = REGIME_NORM * e, alpha * e + np.sqrt(REGIME_NORM ** 2 - alpha ** 2) * r
    else:
        r = noise / np.linalg.norm(noise, axis=-1, keepdims=True)
        D = (50.0 + t.max(1, keepdims=True) - t)[:, :, None]
        a, x = base, base + np.sqrt(D) * r
    return np.concatenate((a, x), axis=1).astype(np.float32)


def edge_modes(name: str):
    """The modes of ref.MODES a case runs in."""
    return ("triplet", "triplet_m03") if name in EDGE_TRIPLET_ONLY else tuple(MODES)


def edge_mode(name: str, mode: str):
    """(kind, score, margin, temp, trainer) of a case's mode: MODES with the case's margin, where it has one."""
    kind, score, margin, temp, which = MODES[mode]
    return kind, score, EDGE_MARGIN.get(name, margin), temp, which


def edge_rows(name: str, mode: str):
    """(anchors, positives, negatives) fp32 of an edge case; the 'r1' / 'r2' regimes have one set of rows for the dot
    score and one for the squared distance (the triplet modes use the latter).  Drawn once, to be left unchanged."""
    seed, B, M, L, regime = EDGE_CASES[name]
    kind, score = MODES[mode][:2]
    data = "dot" if regime in R_TARGETS and kind != "triplet" and score == "dot" else "sqdist"
    key = (seed, B, M, L, regime, data)
    if key not in _edge_cache:
        if regime in R_TARGETS:
            x = draw_regime(seed, B, M, L, regime, data)
        else:
            x = draw_rows(seed, B, M, L).copy()
            if regime == "r3":
                x[0, 1] = x[0, 0]           # tuple 0: the positive is the anchor,
                x[0, 2] = x[0, 0]           #   negative 0 is the anchor (and so the positive),
                x[0, 5] = x[0, 4]           #   negatives 2 and 3 are one row
                x[1, 2] = x[1, 1]           # tuple 1: negative 0 is the positive,
                x[1, 5] = x[1, 4]           #   negatives 2 and 3 are one row,
                x[1, 6] = x[1, 0]           #   negative 4 is the anchor
            elif regime == "r4_mixed":
                x[0, 2:] *= np.float32(30.0)    # tuple 0: every negative far away, every hinge inactive
                x[1, 1] *= np.float32(30.0)     # tuple 1: the positive far away, every hinge active
            else:
                if L == 1:                      # normalised rows of one column are all +-1: give them magnitudes
                    x *= (0.6 + 0.15 * np.arange(2 + M, dtype=np.float32))[None, :, None]
                clear_hinges(x)
        x.setflags(write=False)
        _edge_cache[key] = x
    x = _edge_cache[key]
    return x[:, 0], x[:, 1], x[:, 2:]


def edge_S(a, p, n, kind: str, score: str, temp: float) -> float:
    """S of the bar: the largest sum_e |term_e| over the rows of the case — sum |a_e x_e| / temp for the dot score,
    sum d_e^2 for the squared distance and the triplet — and at least 1."""
    a, p, n = (np.asarray(t, dtype=np.float64) for t in (a, p, n))
    if kind != "triplet" and score == "dot":
        x = np.concatenate((p[:, None], n), axis=1)
        return max(1.0, float(np.abs(a[:, None] * x).sum(-1).max()) / temp)
    return max(1.0, float(scores(a, p, n, kind, score)[0].max()))


def reassociation_term(L: int, S: float) -> float:
    """4 L 2^-53 S: an fp64 sum over L terms re-associated (error of a score <= L 2^-53 S), times the 2 of a softmax
    weight's sensitivity to its logits, times 2 for the two logits of a gap."""
    return 4.0 * L * 2.0 ** -53 * S


def edge_bar(name: str, mode: str) -> float:
    """The bar of a case and mode for the loss (relative) and each gradient (rel_max): 2^-23 + 4 L 2^-53 S."""
    kind, score, _, temp, _ = edge_mode(name, mode)
    return FP32_TERM + reassociation_term(EDGE_CASES[name][3], edge_S(*edge_rows(name, mode), kind, score, temp))


def edge_want(name: str, mode: str, dtype=np.float64):
    """(loss, da, dp, dn) of an edge case and mode, once per session for float64."""
    key = ("want", name, mode)
    if dtype is not np.float64 or key not in _edge_cache:
        kind, score, margin, temp, _ = edge_mode(name, mode)
        got = tuple_loss(*edge_rows(name, mode), kind, score, margin, temp, dtype)
        if dtype is not np.float64:
            return got
        _edge_cache[key] = got
    return _edge_cache[key]


def edge_soft(name: str):
    """(student, teacher) fp32 [B][J] of a case of EDGE_SOFT."""
    seed, B, J, _, _, regime = EDGE_SOFT[name]
    key = ("soft", name)
    if key not in _edge_cache:
        s, t = (v.copy() for v in draw_soft(seed, B, J))
        k = np.arange(B) % J
        other = (k + 1) % J
        for b in range(B):
            row = regime if regime not in ("mixed", "same_sat") else \
                ("teacher_onehot", "student_other", "both_same", "uniform")[b % 4]
            if row in ("teacher_onehot", "student_other", "both_same"):
                t[b, k[b]] = HOT
            if row == "both_same":
                s[b, k[b]] = HOT
            if row == "student_other":
                assert other[b] != k[b]
                s[b, other[b]] = HOT
        if regime in ("same", "same_sat"):
            s = t.copy()
        s.setflags(write=False), t.setflags(write=False)
        _edge_cache[key] = (s, t)
    return _edge_cache[key]


def soft_bar_terms(name: str):
    """(2^-23, 4 2^-53 S + 2^-53 J) of a soft-label case, S = max |x| / temp over both tables and at least 1: no long
    sum stands in front of the logits, the softmax sums have J terms."""
    _, _, J, ts, tt, _ = EDGE_SOFT[name]
    s, t = edge_soft(name)
    S = max(1.0, float(np.abs(s).max()) / ts, float(np.abs(t).max()) / tt)
    return FP32_TERM, 4.0 * 2.0 ** -53 * S + 2.0 ** -53 * J
