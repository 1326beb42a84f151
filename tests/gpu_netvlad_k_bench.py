"""The K-general NetVLAD head at K = 16, 32, 64 and 128 (diagnostic, not a pytest): HIP-event medians of 7 warm batches
at N = 12 and N = 32 on a 30 x 40 x 512 map — forward (vlad_norm) and backward (dW, dC, dX) through
oibl_netvlad_forward_k / oibl_netvlad_backward_k — next to, in the same run, the tuned K = 64 entry points and torch
autograd of the head written with the dense residual[N][K][C][P] on the same device.
    python tests/gpu_netvlad_k_bench.py [output file]"""
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import lib as _lib, ops  # noqa: E402

dev = torch.device("cuda", 0)
C, P = 512, 1200
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_us(fn, warm=3, batches=7):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(batches):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ts)


def dense_head(x_nchw, w, c):
    """The head with one dense residual tensor, as autograd has to keep it (ibl/models/netvlad.py:44-61, 78-80)."""
    xh = F.normalize(x_nchw.flatten(2), dim=1)                              # [N][C][P]
    a = torch.einsum("kc,ncp->nkp", w, xh).softmax(dim=1)                   # [N][K][P]
    res = (xh[:, None] - c[None, :, :, None]) * a[:, :, None]              # [N][K][C][P]
    v = F.normalize(res.sum(-1), dim=2).flatten(1)
    return F.normalize(v, dim=1)


class KHead:
    """The new entry points on buffers allocated once: what ops.netvlad / ops.netvlad_backward do for K != 64, for any K."""

    def __init__(self, N, K):
        self.h = _lib.load()
        self.N, self.K = N, K
        self.fws = torch.empty(self.h.oibl_netvlad_k_workspace_bytes(N, P, K, C), dtype=torch.uint8, device=dev)
        self.bws = torch.empty(self.h.oibl_netvlad_k_backward_workspace_bytes(N, P, K, C, 1), dtype=torch.uint8, device=dev)
        self.y = torch.empty((N, K * C), device=dev)
        self.gw, self.gc = torch.empty((K, C), device=dev), torch.empty((K, C), device=dev)
        self.gx = torch.empty((N, P, C), device=dev)
        self.st = torch.cuda.current_stream(dev).cuda_stream

    def forward(self, x, w, c):
        _lib.check(self.h.oibl_netvlad_forward_k(x.data_ptr(), self.N, P, self.K, C, w.data_ptr(), c.data_ptr(), 1, None,
                                                 self.y.data_ptr(), self.fws.data_ptr(), self.fws.numel(), self.st))

    def backward(self, x, w, c, G):
        _lib.check(self.h.oibl_netvlad_backward_k(x.data_ptr(), self.N, P, self.K, C, w.data_ptr(), c.data_ptr(), 1,
                                                  G.data_ptr(), self.gw.data_ptr(), self.gc.data_ptr(), self.gx.data_ptr(),
                                                  self.bws.data_ptr(), self.bws.numel(), self.st))


g = torch.Generator(device=dev).manual_seed(3)
say(f"K-general NetVLAD head, 30 x 40 x 512 fp32 map, {torch.cuda.get_device_name(0)}; medians of 7 warm batches, us")
for N in (12, 32):
    feat = torch.randn((N, 30, 40, C), generator=g, device=dev) * 3.0
    tuned = {}
    for K in (16, 32, 64, 128):
        w = torch.randn((K, C), generator=g, device=dev) * 0.1
        c = torch.rand((K, C), generator=g, device=dev)
        G = torch.randn((N, K * C), generator=g, device=dev)
        head = KHead(N, K)
        t_f = median_us(lambda: head.forward(feat, w, c))
        t_b = median_us(lambda: head.backward(feat, w, c, G))
        x_nchw = feat.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        wd, cd = w.clone().requires_grad_(True), c.clone().requires_grad_(True)

        def dense_step():
            for t in (x_nchw, wd, cd):
                t.grad = None
            dense_head(x_nchw, wd, cd).backward(G)

        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t_dense = median_us(dense_step, warm=2)
        peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        ws = head.bws.numel() / 2 ** 20
        line = (f"N = {N:2d} K = {K:3d}: forward {t_f:7.1f} | backward dW dC dX {t_b:7.1f} (workspace {ws:5.1f} MiB) | "
                f"torch autograd, dense head forward + backward {t_dense:9.1f} (peak {peak:6.0f} MiB), "
                f"{t_dense / (t_f + t_b):5.1f} x")
        if K == 64:
            t_ft = median_us(lambda: ops.netvlad(feat, w, c, True, want_raw=False, want_norm=True))
            t_bt = median_us(lambda: ops.netvlad_backward(feat, w, c, G, True, want=("w", "c", "x")))
            line += (f" | the tuned K = 64 path: forward {t_ft:7.1f} ({t_f / t_ft:4.2f} x), backward {t_bt:7.1f} "
                     f"({t_b / t_bt:4.2f} x)")
        say(line)
        del x_nchw, wd, cd, head
        torch.cuda.empty_cache()
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
