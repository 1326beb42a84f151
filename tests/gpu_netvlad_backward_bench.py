"""The NetVLAD head's backward at training batches (diagnostic, not a pytest): HIP-event medians of 7 warm batches at
N = 12 and N = 48 on a 30 x 40 x 512 map, with and without grad_feat, next to the forward head and to torch autograd
of the reference's dense head (residual[N][K][C][P] and all) on the same device.
    python tests/gpu_netvlad_backward_bench.py [output file]"""
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import ops, synth  # noqa: E402

dev = torch.device("cuda", 0)
sd = synth.embednetpca_state(0)
cw = sd["net_vlad.conv.weight"].reshape(64, 512).contiguous().to(dev)
cent = sd["net_vlad.centroids"].to(dev)
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
    """The head written with one dense residual tensor, as autograd would have to keep it (what
    ibl/models/netvlad.py:44-61 and 78-80 compute): res[n][k][c][p] = a[n][k][p] * (xh[n][c][p] - cent[k][c])."""
    xh = F.normalize(x_nchw.flatten(2), dim=1)                              # [N][C][P]
    a = torch.einsum("kc,ncp->nkp", w, xh).softmax(dim=1)                   # [N][K][P]
    res = (xh[:, None] - c[None, :, :, None]) * a[:, :, None]              # [N][K][C][P]
    v = F.normalize(res.sum(-1), dim=2).flatten(1)
    return F.normalize(v, dim=1)


g = torch.Generator(device=dev).manual_seed(3)
say(f"NetVLAD head backward, 30 x 40 x 512 fp32 map, {torch.cuda.get_device_name(0)}; medians of 7 warm batches, us")
for N in (12, 48):
    feat = torch.randn((N, 30, 40, 512), generator=g, device=dev) * 3.0
    G = torch.randn((N, 64 * 512), generator=g, device=dev)
    t_fwd = median_us(lambda: ops.netvlad(feat, cw, cent, True, want_raw=False, want_norm=True))
    t_all = median_us(lambda: ops.netvlad_backward(feat, cw, cent, G, True, want=("w", "c", "x")))
    t_par = median_us(lambda: ops.netvlad_backward(feat, cw, cent, G, True, want=("w", "c")))
    x_nchw = feat.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wd, cd = cw.clone().requires_grad_(True), cent.clone().requires_grad_(True)

    def dense_step():
        for t in (x_nchw, wd, cd):
            t.grad = None
        dense_head(x_nchw, wd, cd).backward(G)

    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t_dense = median_us(dense_step, warm=2)
    peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    ws_all = ops._lib.load().oibl_netvlad_backward_workspace_bytes(N, 1200, 64, 512, 1) / 2 ** 20
    ws_par = ops._lib.load().oibl_netvlad_backward_workspace_bytes(N, 1200, 64, 512, 0) / 2 ** 20
    say(f"N = {N:2d}: forward head {t_fwd:7.1f} | backward dW dC dX {t_all:7.1f} (workspace {ws_all:5.1f} MiB) | "
        f"backward dW dC {t_par:7.1f} (workspace {ws_par:5.1f} MiB) | torch autograd, dense head forward + backward "
        f"{t_dense:9.1f} (peak {peak:7.0f} MiB)")
    del x_nchw, wd, cd
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
