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
    Y [N][K*C], dW [K][C], dC [K][C], dX shaped like x."""
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
        dC += -A[:, None] * dV
        da = xh @ dV.T - (dV * c).sum(1)[None, :]
        ds = a * (da - (a * da).sum(1, keepdims=True))
        dW += ds.T @ xh
        dxh = a @ dV + ds @ w
        if normalize_input:
            dX[n] = (dxh - np.where(r_free, xh * (xh * dxh).sum(1, keepdims=True), 0.0)) / r
        else:
            dX[n] = dxh
    return {"Y": Y.reshape(N, K * C), "dW": dW, "dC": dC, "dX": dX.reshape(shape)}


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
