"""float64 evaluation (torch on the CPU, F.conv2d) of what csrc/conv_backward.hip and EmbedNet.forward_train(x,
train_layers='conv5') compute: a 3x3 / pad 1 convolution (+ ReLU) and its three gradients, the chain conv5_1 -> ReLU ->
conv5_2 -> ReLU -> conv5_3 of ibl/models/vgg.py:41-42, 61-62, and the whole EmbedNet under the triplet loss of
Trainer._get_loss (ibl/trainers.py:82-95).  Written from the formulas; tests/test_conv_backward_cpu.py ties it to the
reference's own fp32 autograd (tests/golden/conv5_backward.npz).

Activations are NHWC ([N][h][w][C]) on the outside, as the device kernels take them; weights are the state dict's
[Cout][Cin][3][3]."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

C = 512
GRAD_KEYS = ("dX", "dW1", "dW2", "dW3", "db1", "db2", "db3")
E2E_KEYS = ("dW1", "dW2", "dW3", "db1", "db2", "db3", "dWv", "dCv")
W_ROWS = 4            # output channels of a weight gradient a fixture stores


def rel_l2(got, want) -> float:
    got = np.asarray(got, dtype=np.float64).ravel()
    want = np.asarray(want, dtype=np.float64).ravel()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def draw_inputs(seed: int, N: int, h: int, w: int):
    """The inputs of a layer case from its seed, as float32, in this order from one np.random.RandomState:
    x [N][h][w][512] = max(N(0,1), 0) (a pooled post-ReLU map: half of it exact zeros), three weights ~ N(0, sqrt(2 /
    (9 * 512))) (VGG.reset_params' kaiming fan_out), three biases ~ 0.1 N(0,1), G [N][h][w][512] ~ N(0,1).
    Returns (x, [w1, w2, w3], [b1, b2, b3], G)."""
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.standard_normal((N, h, w, C)), 0.0).astype(np.float32)
    ws = [(rs.standard_normal((C, C, 3, 3)) * np.sqrt(2.0 / (9 * C))).astype(np.float32) for _ in range(3)]
    bs = [(0.1 * rs.standard_normal((C,))).astype(np.float32) for _ in range(3)]
    G = rs.standard_normal((N, h, w, C)).astype(np.float32)
    return x, ws, bs, G


def _nchw64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def conv_forward(x, w, b, relu: bool):
    """x NHWC, w OIHW, b -> conv3x3(pad 1) + b (+ ReLU), NHWC float64."""
    y = F.conv2d(_nchw64(x), torch.from_numpy(w).double(), torch.from_numpy(b).double(), padding=1)
    return _nhwc(F.relu(y) if relu else y)


def layer_grads(x, w, G, out_act=None):
    """One layer: dZ = G where out_act > 0 (all of G without out_act) -> {"dW", "db", "dX"} float64."""
    dz = np.asarray(G, dtype=np.float64)
    if out_act is not None:
        dz = dz * (np.asarray(out_act) > 0)
    xt = _nchw64(x).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    bt = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    F.conv2d(xt, wt, bt, padding=1).backward(_nchw64(dz))
    return {"dW": wt.grad.numpy(), "db": bt.grad.numpy(), "dX": _nhwc(xt.grad)}


def chain_grads(x, ws, bs, G):
    """conv5_1 -> ReLU -> conv5_2 -> ReLU -> conv5_3 on x and the backward of G through it ->
    {"y", "dX", "dW1..3", "db1..3"} float64 (activations NHWC)."""
    xt = _nchw64(x).requires_grad_(True)
    wt = [torch.from_numpy(w).double().requires_grad_(True) for w in ws]
    bt = [torch.from_numpy(b).double().requires_grad_(True) for b in bs]
    t = xt
    for i in range(3):
        t = F.conv2d(t, wt[i], bt[i], padding=1)
        if i < 2:
            t = F.relu(t)
    t.backward(_nchw64(G))
    out = {"y": _nhwc(t.detach()), "dX": _nhwc(xt.grad)}
    for i in range(3):
        out[f"dW{i + 1}"] = wt[i].grad.numpy()
        out[f"db{i + 1}"] = bt[i].grad.numpy()
    return out


def tuple_loss(vlad, B: int, n: int, margin: float = 0.1 ** 0.5):
    """Trainer._get_loss(..., 'triplet') (ibl/trainers.py:82-95); margin: the scripts' default 0.1 ** 0.5."""
    out = vlad.view(B, n, -1)
    L = out.size(-1)
    neg = out[:, 2:]
    anc = out[:, 0].unsqueeze(1).expand_as(neg).contiguous().view(-1, L)
    pos = out[:, 1].unsqueeze(1).expand_as(neg).contiguous().view(-1, L)
    return F.triplet_margin_loss(anc, pos, neg.contiguous().view(-1, L), margin=margin, p=2, reduction="mean")


_POOL_AFTER = (1, 3, 6, 9)      # conv indices (0-based) followed by a 2x2 max-pool; conv 12 has neither ReLU nor pool


def embednet_grads(images, state, B: int, n: int, margin: float = 0.1 ** 0.5):
    """The whole EmbedNet (vgg16 cfg D without its last ReLU / pool, NetVLAD(64, 512), intra + L2 normalisation) in
    float64 on `images` [B*n][3][H][W] with the state dict `state` (keys base_model.base.*, net_vlad.*), the triplet
    loss over B tuples of n images, and its gradients for the six conv5 tensors and the two NetVLAD tensors ->
    {"loss", "vlad", "dW1..3", "db1..3", "dWv" [64][512], "dCv" [64][512]} float64."""
    convs = [i for i in range(29) if f"base_model.base.{i}.weight" in state]
    assert len(convs) == 13 and convs[10:] == [24, 26, 28]
    wt = [state[f"base_model.base.{i}.weight"].double().clone() for i in convs]
    bt = [state[f"base_model.base.{i}.bias"].double().clone() for i in convs]
    for t in wt[10:] + bt[10:]:
        t.requires_grad_(True)
    wv = state["net_vlad.conv.weight"].double().clone().requires_grad_(True)
    cv = state["net_vlad.centroids"].double().clone().requires_grad_(True)
    t = images.double()
    with torch.no_grad():
        for i in range(10):
            t = F.relu(F.conv2d(t, wt[i], bt[i], padding=1))
            if i in _POOL_AFTER:
                t = F.max_pool2d(t, 2, 2)
    for i in range(10, 13):
        t = F.conv2d(t, wt[i], bt[i], padding=1)
        if i < 12:
            t = F.relu(t)
    # NetVLAD.forward (ibl/models/netvlad.py:44-61) and the two normalisations of EmbedNet.forward (:78-80)
    N_, K = t.shape[0], wv.shape[0]
    xh = F.normalize(t, p=2, dim=1)
    soft = F.softmax(F.conv2d(xh, wv).view(N_, K, -1), dim=1)
    xf = xh.view(N_, C, -1)
    vlad = torch.einsum("nkp,ncp->nkc", soft, xf) - soft.sum(-1).unsqueeze(-1) * cv.unsqueeze(0)
    vlad = F.normalize(vlad, p=2, dim=2).view(N_, -1)
    vlad = F.normalize(vlad, p=2, dim=1)
    loss = tuple_loss(vlad, B, n, margin)
    loss.backward()
    out = {"loss": float(loss.detach()), "vlad": vlad.detach().numpy(), "dWv": wv.grad.reshape(K, C).numpy(),
           "dCv": cv.grad.numpy()}
    for i in range(3):
        out[f"dW{i + 1}"] = wt[10 + i].grad.numpy()
        out[f"db{i + 1}"] = bt[10 + i].grad.numpy()
    return out
