"""The SFRS region head (EmbedRegionNet._compute_region_sim, ibl/models/netvlad.py:123-186) and its gradients in numpy
float64: the yardstick of oibl_region_vlad_backward and oibl_region_scores_backward.

Notation of helpers/netvlad_grad_ref; q(p) the quarter of pixel p (q0 top-left, q1 top-right, q2 bottom-left, q3
bottom-right), S_r the quarters of region r in the order REGIONS, eps = 1e-12:
    forward   V_q,k = sum_{p in q} a_pk xh_p - A_q,k c_k,  A_q,k = sum_{p in q} a_pk
              R_r = sum_{q in S_r} V_q,  t_r,k = max(|R_r,k|, eps),  U_r,k = R_r,k / t_r,k
              g_r = max(|U_r|_F, eps),  Y_r = U_r / g_r
              score[t, j, a, b] = <Y[t, 0][a], Y[t, 1 + j][b]>
    backward  dU_r = (G_r - Y_r <Y_r, G_r>) / g_r,  dR_r,k = (dU_r,k - U_r,k <U_r,k, dU_r,k>) / t_r,k
              dV_q = sum_{r : q in S_r} dR_r,  dC_k = -sum_q A_q,k dV_q,k
              da_pk = <dV_q(p),k, xh_p> - <dV_q(p),k, c_k>,  ds_pk = a_pk (da_pk - sum_j a_pj da_pj)
              dW_k = sum_p ds_pk xh_p,  dxh_p = sum_k (a_pk dV_q(p),k + ds_pk w_k)
              dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p
    scores    dY[t, 0][a] = sum_j sum_b Gs[t, j, a, b] Y[t, 1 + j][b],  dY[t, 1 + j][b] = sum_a Gs[t, j, a, b] Y[t, 0][a]
Where a max(., eps) is active the denominator is a constant (torch's clamp_min): that step's projection is dropped.
"""
from __future__ import annotations

import numpy as np

from . import netvlad_grad_ref as nref

EPS = 1e-12
REGIONS = ((0, 1, 2, 3), (0, 1), (2, 3), (0, 2), (1, 3), (0,), (1,), (2,), (3,))
rel_l2 = nref.rel_l2


def quarter_of(h: int, w_: int) -> np.ndarray:
    """[h][w] -> the quarter index of every pixel."""
    rows = (np.arange(h) >= h // 2).astype(np.int64)
    cols = (np.arange(w_) >= w_ // 2).astype(np.int64)
    return 2 * rows[:, None] + cols[None, :]


def scores(Y, T: int):
    """Y [T*(1+n)][9][L] -> score [T][n][9][9] in float64."""
    Y = np.asarray(Y, dtype=np.float64)
    v = Y.reshape(T, -1, 9, Y.shape[-1])
    return np.einsum("tal,tjbl->tjab", v[:, 0], v[:, 1:])


def scores_backward(Y, Gs, T: int):
    """dL/dY [T*(1+n)][9][L] from Gs = dL/dscore [T][n][9][9], in float64."""
    Y = np.asarray(Y, dtype=np.float64)
    Gs = np.asarray(Gs, dtype=np.float64)
    v = Y.reshape(T, -1, 9, Y.shape[-1])
    d = np.empty_like(v)
    d[:, 0] = np.einsum("tjab,tjbl->tal", Gs, v[:, 1:])
    d[:, 1:] = np.einsum("tjab,tal->tjbl", Gs, v[:, 0])
    return d.reshape(Y.shape)


def forward(x, w, c, normalize_input=True):
    """x [N][h][w][C] -> Y [N][9][K*C] float64."""
    N = np.shape(x)[0]
    K, C = np.shape(w)
    return head_and_grads(x, w, c, np.zeros((N, 9, K * C)), normalize_input)["Y"]


def head_and_grads(x, w, c, G, normalize_input=True, Gs=None, T=None):
    """x [N][h][w][C], w [K][C], c [K][C], G [N][9][K*C] = the direct dL/dY; with Gs [T][n][9][9] = dL/dscore the
    scores' backward is added to it.  -> dict of float64 arrays: Y [N][9][K*C], score (with T), dW, dC [K][C], dX like
    x, dY the total gradient that entered the head."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    N, h, w_, C = x.shape
    K = w.shape[0]
    assert h % 2 == 0 and w_ % 2 == 0
    qmap = quarter_of(h, w_).reshape(-1)
    xs = x.reshape(N, h * w_, C)
    keep = []
    Y = np.empty((N, 9, K, C))
    for n in range(N):
        xn = xs[n]
        if normalize_input:
            nrm = np.sqrt((xn * xn).sum(1, keepdims=True))
            r = np.maximum(nrm, EPS)
            r_free = nrm >= EPS
        else:
            r = np.ones((xn.shape[0], 1))
            r_free = np.zeros((xn.shape[0], 1), dtype=bool)
        xh = xn / r
        s = xh @ w.T
        e = np.exp(s - s.max(1, keepdims=True))
        a = e / e.sum(1, keepdims=True)
        Aq = np.stack([a[qmap == q].sum(0) for q in range(4)])
        Vq = np.stack([a[qmap == q].T @ xh[qmap == q] - Aq[q][:, None] * c for q in range(4)])
        regs = []
        for ri, members in enumerate(REGIONS):
            R = Vq[list(members)].sum(0)
            tn = np.sqrt((R * R).sum(1, keepdims=True))
            t = np.maximum(tn, EPS)
            U = R / t
            gn = np.sqrt((U * U).sum())
            g = max(gn, EPS)
            Y[n, ri] = U / g
            regs.append((tn, t, U, gn, g))
        keep.append((r, r_free, xh, a, Aq, regs))
    Yf = Y.reshape(N, 9, K * C)
    out = {"Y": Yf}
    dY = np.asarray(G, dtype=np.float64).reshape(N, 9, K * C).copy()
    if Gs is not None:
        out["score"] = scores(Yf, T)
        dY += scores_backward(Yf, Gs, T)
    out["dY"] = dY
    dYr = dY.reshape(N, 9, K, C)
    dW = np.zeros((K, C))
    dC = np.zeros((K, C))
    dX = np.empty_like(xs)
    for n in range(N):
        r, r_free, xh, a, Aq, regs = keep[n]
        dVq = np.zeros((4, K, C))
        for ri, members in enumerate(REGIONS):
            tn, t, U, gn, g = regs[ri]
            Gr = dYr[n, ri]
            dU = Gr / g
            if gn >= EPS:
                dU = dU - Y[n, ri] * (Y[n, ri] * Gr).sum() / g
            dR = dU / t - np.where(tn >= EPS, U * (U * dU).sum(1, keepdims=True) / t, 0.0)
            for q in members:
                dVq[q] += dR
        dC -= (Aq[:, :, None] * dVq).sum(0)
        da = np.empty_like(a)
        for q in range(4):                                         # every pixel against its own quarter's dV
            da[qmap == q] = xh[qmap == q] @ dVq[q].T - (dVq[q] * c).sum(1)[None, :]
        ds = a * (da - (a * da).sum(1, keepdims=True))
        dW += ds.T @ xh
        dxh = ds @ w
        for q in range(4):
            dxh[qmap == q] += a[qmap == q] @ dVq[q]
        if normalize_input:
            dX[n] = (dxh - np.where(r_free, xh * (xh * dxh).sum(1, keepdims=True), 0.0)) / r
        else:
            dX[n] = dxh
    out.update(dW=dW, dC=dC, dX=dX.reshape(x.shape))
    return out


def draw_G(seed: int, N: int, T: int, K: int = 64, C: int = 512):
    """G [N][9][K*C] ~ N(0,1) and Gs [T][N/T - 1][9][9] ~ N(0,1), in this order from one RandomState(seed), float32."""
    rs = np.random.RandomState(seed)
    G = rs.randn(N, 9, K * C).astype(np.float32)
    Gs = rs.randn(T, N // T - 1, 9, 9).astype(np.float32)
    return G, Gs


def sfrs_loss_and_grads(Y, score, label, B: int, temp: float = 0.07, lambda_soft: float = 0.5):
    """SFRSTrainer's loss at generation 0 (ibl/trainers.py:247-257) from ONE model call, in float64:
    loss_hard = _get_loss(A, P, Neg, B, 'sare_ind') on region 0 (:298-315; pair 0 the positive, pairs 1.. the
    negatives), loss_soft = the soft cross-entropy of score[:, :, 0] / temp against `label` [B][n 9].
    -> (loss_hard + lambda_soft loss_soft, G [B (1+n)][9][L] the direct dL/dY, Gs [B][n][9][9] = dL/dscore)."""
    Y = np.asarray(Y, dtype=np.float64)
    v = Y.reshape(B, -1, 9, Y.shape[-1])
    n = v.shape[1] - 1
    G = np.zeros_like(v)
    M = B * (n - 1)
    hard = 0.0
    for b in range(B):
        A, P = v[b, 0, 0], v[b, 1, 0]
        pos = A @ P
        for j in range(2, n + 1):
            neg = A @ v[b, j, 0]
            z = (neg - pos) / temp
            hard += np.logaddexp(0.0, z) / M
            sg = 1.0 / (1.0 + np.exp(-z)) / temp / M
            G[b, 0, 0] += sg * (v[b, j, 0] - P)
            G[b, 1, 0] -= sg * A
            G[b, j, 0] += sg * A
    z = np.asarray(score, dtype=np.float64)[:, :, 0].reshape(B, -1) / temp
    z = z - z.max(1, keepdims=True)
    logq = z - np.log(np.exp(z).sum(1, keepdims=True))
    label = np.asarray(label, dtype=np.float64)
    soft = -(label * logq).mean(0).sum()
    dz = (np.exp(logq) * label.sum(1, keepdims=True) - label) / B
    Gs = np.zeros((B, n, 9, 9))
    Gs[:, :, 0] = lambda_soft * dz.reshape(B, n, 9) / temp
    return hard + lambda_soft * soft, G.reshape(Y.shape), Gs


def draw_label(seed: int, B: int, n: int, temp: float = 0.07):
    """The soft label of the tuple case: softmax(u / temp) over the n 9 scores, u ~ U(0.2, 0.5) [B][n 9], float32."""
    u = np.random.RandomState(seed).uniform(0.2, 0.5, (B, n * 9))
    e = np.exp((u - u.max(1, keepdims=True)) / temp)
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def draw_vectors(seed: int, T: int, n: int, L: int = 32768):
    """Inputs of a scores case: Y [T (1+n)][9][L] unit rows of N(0,1) and Gs [T][n][9][9] ~ N(0,1), in this order from
    one RandomState(seed), float32."""
    rs = np.random.RandomState(seed)
    Y = rs.randn(T * (1 + n), 9, L)
    Y = (Y / np.sqrt((Y * Y).sum(2, keepdims=True))).astype(np.float32)
    Gs = rs.randn(T, n, 9, 9).astype(np.float32)
    return Y, Gs


_drawn = {}


def golden_head_case(name: str, z):
    """A head case of tests/golden/region_backward.npz (`z`, the loaded file) regenerated from its seed, once per
    session: ((x, w, c, G, Gs, normalize_input), want).  G [N][9][K*C] and Gs [1][N-1][9][9] are the fp32 gradients a
    device call is given — drawn (draw_G) or, in the tuple case, the gradients of the SFRS generation-0 loss at the
    float64 forward — and `want` their float64 head_and_grads, plus want["loss"] and want["exact"]: the same from the
    UNROUNDED loss gradients, which is what the reference's autograd computes (`want` itself elsewhere)."""
    if name not in _drawn:
        seed = int(z[f"{name}_seed"])
        N, h, w_, _ = map(int, z[f"{name}_shape"])
        normalize = bool(z[f"{name}_normalize_input"])
        if name.startswith("trained"):
            x, w, c, _, _ = nref.draw_trained_inputs(seed, N, h, w_)
        elif name.startswith("raw"):
            x, w, c, _ = nref.draw_inputs(seed, N, h, w_)
        else:
            x, w, c, _, _ = nref.draw_tuple_inputs(seed, 1, N, h, w_, float(z[f"{name}_jitter"]))
        if name.startswith("tuple"):
            Y = forward(x, w, c, normalize)
            loss, G64, Gs64 = sfrs_loss_and_grads(Y, scores(Y, 1), draw_label(seed, 1, N - 1), 1)
            G, Gs = G64.astype(np.float32), Gs64.astype(np.float32)
            exact = head_and_grads(x, w, c, G64, normalize, Gs=Gs64, T=1)
        else:
            G, Gs = draw_G(seed + 100, N, 1)
            loss, exact = None, None
        want = head_and_grads(x, w, c, G, normalize, Gs=Gs, T=1)
        want["loss"] = loss if loss is not None else float((want["Y"] * G).sum() + (want["score"] * Gs).sum())
        want["exact"] = want if exact is None else exact
        _drawn[name] = ((x, w, c, G, Gs, normalize), want)
    return _drawn[name]
