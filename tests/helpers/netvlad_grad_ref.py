"""The NetVLAD descriptor head and its gradients in numpy float64: the yardstick of the device backward.

Forward (ibl/models/netvlad.py:44-61, 78-80), per image, x_p the P rows of the NHWC map, eps = 1e-12:
    r_p = max(|x_p|, eps), xh_p = x_p / r_p (normalize_input False: xh = x)
    s_pk = w_k . xh_p, a_p = softmax_k(s_p), A_k = sum_p a_pk
    V_k = sum_p a_pk xh_p - A_k c_k, t_k = max(|V_k|, eps), U_k = V_k / t_k
    g = max(|U|_F, eps), Y = U / g
Backward, G = dL/dY:
    dU = (G - Y <Y, G>) / g,  dV_k = (dU_k - U_k <U_k, dU_k>) / t_k,  dC_k = -A_k dV_k
    da_pk = <dV_k, xh_p> - <dV_k, c_k>,  ds_pk = a_pk (da_pk - sum_j a_pj da_pj)
    dW_k = sum_p ds_pk xh_p,  dxh_p = sum_k (a_pk dV_k + ds_pk w_k),  dx_p = (dxh_p - xh_p <xh_p, dxh_p>) / r_p
Where a max(., eps) is active the denominator is a constant, as torch's clamp_min treats it: the projection term of
that step is dropped (an all-zero pixel gets dx_p = dxh_p / eps).
"""
from __future__ import annotations

import numpy as np

EPS = 1e-12


def head_and_grads(x, w, c, G, normalize_input=True):
    """x [N][P][C] (or [N][h][w][C]), w [K][C], c [K][C], G [N][K*C] -> dict of float64 arrays:
    Y [N][K*C], dW [K][C], dC [K][C], dX shaped like x, and the regime of the case: a [N][P][K] the soft-assignment,
    A [N][K] its column sums, dCn [N][K][C] the images' contributions to dC."""
    shape = np.shape(x)
    x = np.asarray(x, dtype=np.float64).reshape(shape[0], -1, shape[-1])
    w = np.asarray(w, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    N, P, C = x.shape
    K = w.shape[0]
    G = np.asarray(G, dtype=np.float64).reshape(N, K, C)
    Y = np.empty((N, K, C))
    dW = np.zeros((K, C))
    dC = np.zeros((K, C))
    dX = np.empty_like(x)
    a_all = np.empty((N, P, K))
    A_all = np.empty((N, K))
    dCn = np.empty((N, K, C))
    for n in range(N):
        xn = x[n]
        if normalize_input:
            nrm = np.sqrt((xn * xn).sum(1, keepdims=True))
            r = np.maximum(nrm, EPS)
            r_free = nrm >= EPS
        else:
            r = np.ones((P, 1))
            r_free = np.zeros((P, 1), dtype=bool)      # no normalisation: no projection
        xh = xn / r
        s = xh @ w.T
        e = np.exp(s - s.max(1, keepdims=True))
        a = e / e.sum(1, keepdims=True)
        A = a.sum(0)
        V = a.T @ xh - A[:, None] * c
        tn = np.sqrt((V * V).sum(1, keepdims=True))
        t = np.maximum(tn, EPS)
        U = V / t
        gn = np.sqrt((U * U).sum())
        g = max(gn, EPS)
        Y[n] = U / g
        dU = G[n] / g
        if gn >= EPS:
            dU = dU - Y[n] * (Y[n] * G[n]).sum() / g
        dV = dU / t
        dV = dV - np.where(tn >= EPS, U * (U * dU).sum(1, keepdims=True) / t, 0.0)
        a_all[n], A_all[n], dCn[n] = a, A, -A[:, None] * dV
        dC += dCn[n]
        da = xh @ dV.T - (dV * c).sum(1)[None, :]
        ds = a * (da - (a * da).sum(1, keepdims=True))
        dW += ds.T @ xh
        dxh = a @ dV + ds @ w
        if normalize_input:
            dX[n] = (dxh - np.where(r_free, xh * (xh * dxh).sum(1, keepdims=True), 0.0)) / r
        else:
            dX[n] = dxh
    return {"Y": Y.reshape(N, K * C), "dW": dW, "dC": dC, "dX": dX.reshape(shape), "a": a_all, "A": A_all, "dCn": dCn}


def rel_l2(got, want) -> float:
    got = np.asarray(got, dtype=np.float64).ravel()
    want = np.asarray(want, dtype=np.float64).ravel()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def draw_inputs(seed: int, N: int, h: int, w_: int, K: int = 64, C: int = 512):
    """The inputs of a case from its seed: x ~ 3 N(0,1) [N][h][w][C], w ~ 0.1 N(0,1), c ~ U(0,1), G ~ N(0,1), in this
    order from one np.random.RandomState, as float32."""
    rs = np.random.RandomState(seed)
    x = (3.0 * rs.randn(N, h, w_, C)).astype(np.float32)
    w = (0.1 * rs.randn(K, C)).astype(np.float32)
    c = rs.rand(K, C).astype(np.float32)
    G = rs.randn(N, K * C).astype(np.float32)
    return x, w, c, G


def _trained_params(x, centres, labels, sharpen):
    """c, w and the regime figures of a trained-like case from its fp32 maps x [M][P][C] (see draw_trained_inputs)."""
    K, C = centres.shape
    xd = x.astype(np.float64).reshape(-1, C)
    d = xd / np.sqrt((xd * xd).sum(1, keepdims=True))              # the normalised descriptors ("traindescs")
    lab = labels.reshape(-1)
    c = centres / np.sqrt((centres * centres).sum(1, keepdims=True))
    for k in range(K):
        if (lab == k).any():
            c[k] = d[lab == k].mean(0)
    c = c.astype(np.float32)                                       # the centroids ("clsts") are these fp32 values
    cd = c.astype(np.float64)
    ca = cd / np.sqrt((cd * cd).sum(1, keepdims=True))
    dots = np.sort(ca @ d.T, axis=0)[::-1]
    alpha = float(-np.log(0.01) / np.mean(dots[0] - dots[1]))
    w = (sharpen * (alpha * ca)).astype(np.float32)
    return w, c, alpha, d


def _regime(x, w, c):
    out = head_and_grads(x, w, c, np.zeros((x.shape[0], w.size)), True)
    return {"mean_max_a": float(out["a"].max(2).mean()), "min_A": float(out["A"].min())}


def draw_trained_inputs(seed: int, N: int, h: int, w_: int, sharpen: float = 1.0, populate: bool = True,
                        K: int = 64, C: int = 512):
    """Inputs that look like a conv5_3 map behind its ReLU under the weights NetVLAD._init_params sets
    (ibl/models/netvlad.py:34-42), for normalize_input=True: (x [N][h][w][C], w [K][C], c [K][C], G [N][K*C], info),
    the arrays float32.  From one np.random.RandomState(seed), in this order, P = h * w_:
        centres = randn(K, C)
        labels[n] = permutation(arange(P) % K) (populate) or randint(0, K, P)           for n = 0 .. N-1
        noise = randn(N, P, C);  scale = uniform(0.5, 20, (N, P, 1));  G = randn(N, K * C)
        x = fp32(relu(centres[labels] + 0.5 noise) * scale)          non-negative, about half exact zeros
    then in float64, from the fp32 x: d_p = x_p / |x_p| over all N P pixels, c_k = fp32(mean of the d_p with label k;
    centres_k / |centres_k| where no pixel has it), ca_k = c_k / |c_k|, dots = ca d^T sorted descending per pixel,
        alpha = -ln(0.01) / mean_p(dots[0] - dots[1]),  w = fp32(sharpen * alpha * ca)
    which is _init_params with clsts = c and traindescs = d, times `sharpen`.  info: alpha, and from the float64
    forward under (w, c) mean_max_a = mean_{n,p} max_k a_pk and min_A = min_{n,k} A_k; plus `descs` = d."""
    rs = np.random.RandomState(seed)
    P = h * w_
    centres = rs.randn(K, C)
    labels = np.stack([rs.permutation(np.arange(P) % K) if populate else rs.randint(0, K, P) for _ in range(N)])
    noise = rs.randn(N, P, C)
    scale = rs.uniform(0.5, 20.0, (N, P, 1))
    G = rs.randn(N, K * C).astype(np.float32)
    x = (np.maximum(centres[labels] + 0.5 * noise, 0.0) * scale).astype(np.float32).reshape(N, h, w_, C)
    w, c, alpha, d = _trained_params(x, centres, labels, sharpen)
    info = {"alpha": alpha, **_regime(x, w, c), "descs": d}
    return x, w, c, G, info


def triplet_loss_and_grad(Y, B, n, margin=0.3, eps=1e-6):
    """The reference's triplet loss (ibl/trainers.py:82-95: F.triplet_margin_loss, p = 2, mean over the B (n - 2)
    triplets, pairwise_distance's eps added to the difference) of Y [B n][L] in float64, and dL/dY."""
    Y = np.asarray(Y, dtype=np.float64).reshape(B, n, -1)
    G = np.zeros_like(Y)
    loss, T = 0.0, B * (n - 2)
    for b in range(B):
        u = Y[b, 0] - Y[b, 1] + eps
        dap = np.sqrt((u * u).sum())
        for j in range(2, n):
            v = Y[b, 0] - Y[b, j] + eps
            dan = np.sqrt((v * v).sum())
            li = dap - dan + margin
            if li > 0:
                loss += li / T
                G[b, 0] += (u / dap - v / dan) / T
                G[b, 1] -= u / dap / T
                G[b, j] += v / dan / T
    return loss, G.reshape(B * n, -1)


def draw_tuple_inputs(seed: int, B: int, n: int, h: int, w_: int, jitter: float, K: int = 64, C: int = 512):
    """B tuples of n near-identical trained-like maps under the gradient of the reference's triplet loss: the case
    in which the images' contributions to dC cancel.  (x [B n][h][w][C], w, c, G [B n][K*C], info), float32.  From
    one np.random.RandomState(seed), in this order, P = h * w_:
        centres = randn(K, C);  labels[b] = permutation(arange(P) % K);  noise = randn(B, P, C)
        scale = uniform(0.5, 20, (B, P, 1));  member = randn(B, n, P, C)
        x[b, m] = fp32(relu(centres[labels[b]] + 0.5 noise[b] + jitter member[b, m]) * scale[b])
    w, c as in draw_trained_inputs (sharpen 1) from all B n maps, a member's pixels carrying its tuple's labels.
    G = fp32(dL/dY), L the triplet loss (margin 0.3) of the float64 Y of this helper; its rows sum to zero within a
    tuple up to the fp32 rounding (asserted).  info: alpha, mean_max_a, min_A, loss, and cancellation =
    sum_n |dC_n|_F / |sum_n dC_n|_F in float64."""
    rs = np.random.RandomState(seed)
    P = h * w_
    centres = rs.randn(K, C)
    labels = np.stack([rs.permutation(np.arange(P) % K) for _ in range(B)])
    noise = rs.randn(B, P, C)
    scale = rs.uniform(0.5, 20.0, (B, P, 1))
    member = rs.randn(B, n, P, C)
    pre = (centres[labels] + 0.5 * noise)[:, None] + jitter * member
    x = (np.maximum(pre, 0.0) * scale[:, None]).astype(np.float32).reshape(B * n, h, w_, C)
    w, c, alpha, _ = _trained_params(x, centres, np.repeat(labels[:, None], n, 1), 1.0)
    fwd = head_and_grads(x, w, c, np.zeros((B * n, K * C)), True)
    loss, G64 = triplet_loss_and_grad(fwd["Y"], B, n)
    G = G64.astype(np.float32)
    assert loss > 0 and np.abs(G).max() > 0
    assert np.abs(G.astype(np.float64).reshape(B, n, -1).sum(1)).max() <= 1e-6 * np.abs(G).max()
    out = head_and_grads(x, w, c, G, True)
    cancellation = float(np.sqrt((out["dCn"] ** 2).sum((1, 2))).sum() / np.sqrt((out["dC"] ** 2).sum()))
    info = {"alpha": alpha, "mean_max_a": float(out["a"].max(2).mean()), "min_A": float(out["A"].min()),
            "loss": float(loss), "cancellation": cancellation}
    return x, w, c, G, info
