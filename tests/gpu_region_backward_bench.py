"""The SFRS region head's backward at training batches (diagnostic, not a pytest): HIP-event medians of 7 warm batches
at N = 12 and N = 48 on a 30 x 40 x 512 map, with and without grad_feat, next to the plain head's backward
(ops.netvlad_backward: the same contractions without the region stage) at the same shapes, the scores' backward at
T = 1, n = 10, torch autograd of the region head written with the dense residual on the same device, and one whole SFRS
step (12 + 11 images of 480 x 640, train_layers='conv5').
    python tests/gpu_region_backward_bench.py [output file]"""
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import models, ops, synth  # noqa: E402

dev = torch.device("cuda", 0)
sd = synth.embednetpca_state(0)
cw = sd["net_vlad.conv.weight"].reshape(64, 512).contiguous().to(dev)
cent = sd["net_vlad.centroids"].to(dev)
L = 64 * 512
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


def dense_region_head(x_nchw, w, c):
    """The region head written with one dense residual tensor per quarter, as autograd would have to keep it (what
    ibl/models/netvlad.py:123-175 computes): res[n q][k][c][p] = a[n q][k][p] * (xh[n q][c][p] - cent[k][c])."""
    N, C, H, W = x_nchw.shape
    xq = x_nchw.view(N, C, 2, H // 2, 2, W // 2).permute(0, 2, 4, 1, 3, 5).reshape(N * 4, C, -1)
    xh = F.normalize(xq, dim=1)                                             # [N 4][C][P/4]
    a = torch.einsum("kc,ncp->nkp", w, xh).softmax(dim=1)                   # [N 4][K][P/4]
    res = (xh[:, None] - c[None, :, :, None]) * a[:, :, None]              # [N 4][K][C][P/4]
    q = res.sum(-1).view(N, 4, 64, C)
    regions = torch.cat([q.sum(1, keepdim=True), torch.stack((q[:, 0] + q[:, 1], q[:, 2] + q[:, 3], q[:, 0] + q[:, 2],
                                                              q[:, 1] + q[:, 3]), dim=1), q], dim=1)
    return F.normalize(F.normalize(regions, dim=3).flatten(2), dim=2)       # [N][9][K C]


g = torch.Generator(device=dev).manual_seed(3)
lib = ops._lib.load()
say(f"SFRS region head backward, 30 x 40 x 512 fp32 map, {torch.cuda.get_device_name(0)}; medians of 7 warm batches, us")
for N in (12, 48):
    feat = torch.randn((N, 30, 40, 512), generator=g, device=dev) * 3.0
    G = torch.randn((N, 9, L), generator=g, device=dev)
    G0 = G[:, 0].contiguous()
    t_fwd = median_us(lambda: ops.region_vlad(feat, cw, cent, True))
    t_all = median_us(lambda: ops.region_vlad_backward(feat, cw, cent, G, True, want=("w", "c", "x")))
    t_par = median_us(lambda: ops.region_vlad_backward(feat, cw, cent, G, True, want=("w", "c")))
    p_all = median_us(lambda: ops.netvlad_backward(feat, cw, cent, G0, True, want=("w", "c", "x")))
    p_par = median_us(lambda: ops.netvlad_backward(feat, cw, cent, G0, True, want=("w", "c")))
    x_nchw = feat.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wd, cd = cw.clone().requires_grad_(True), cent.clone().requires_grad_(True)

    def dense_step():
        for t in (x_nchw, wd, cd):
            t.grad = None
        dense_region_head(x_nchw, wd, cd).backward(G)

    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t_dense = median_us(dense_step, warm=2)
    peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
    ws_all = lib.oibl_region_backward_workspace_bytes(N, 30, 40, 64, 512, 1) / 2 ** 20
    ws_par = lib.oibl_region_backward_workspace_bytes(N, 30, 40, 64, 512, 0) / 2 ** 20
    say(f"N = {N:2d}: region forward {t_fwd:7.1f} | region backward dW dC dX {t_all:7.1f} (workspace {ws_all:5.1f} MiB) | "
        f"dW dC {t_par:7.1f} (workspace {ws_par:5.1f} MiB) | plain head backward dW dC dX {p_all:7.1f}, dW dC {p_par:7.1f} "
        f"| ratio {t_all / p_all:4.2f}, {t_par / p_par:4.2f} | torch autograd, dense region head forward + backward "
        f"{t_dense:9.1f} (peak {peak:7.0f} MiB)")
    del x_nchw, wd, cd
    torch.cuda.empty_cache()

vec = F.normalize(torch.randn((11, 9, L), generator=g, device=dev), dim=2)
Gs = torch.randn((1, 10, 9, 9), generator=g, device=dev)
say(f"scores, T = 1, n = 10: forward {median_us(lambda: ops.region_scores(vec, 1)):6.1f} | backward "
    f"{median_us(lambda: ops.region_scores_backward(vec, Gs, 1)):6.1f}")


def make():
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    m = models.create("embedregionnet", base, pool, tuple_size=1)
    m.load_state_dict({k: v for k, v in sd.items() if not k.startswith("pca_layer")})
    return m.to(dev)


model, cache = make().train(), make().train()
images = synth.images(22, 480, 640, seed=5).to(dev)
easy, diff = images[:12].contiguous(), torch.cat([images[:1], images[12:]], dim=0).contiguous()
params = [p for i in (24, 26, 28) for p in model.base_model.base[i].parameters()] + list(model.net_vlad.parameters())
opt = torch.optim.SGD(params, lr=1e-4, momentum=0.9)
losses = []


def sfrs_step(temp=0.07, margin=0.1 ** 0.5):
    """One generation-0 step of SFRSTrainer.train (ibl/trainers.py:196-204, 235-259) with the 'triplet' loss."""
    _, va, vp = model.forward_train(easy, train_layers="conv5")
    with torch.no_grad():
        label, _, _ = cache.region_similarity(diff)
    sim_diff, _, _ = model.forward_train(diff, train_layers="conv5")
    neg = vp[:, 1:, 0]
    a = va[:, 0, 0].unsqueeze(1).expand_as(neg).reshape(-1, L)
    p = vp[:, 0, 0].unsqueeze(1).expand_as(neg).reshape(-1, L)
    hard = F.triplet_margin_loss(a, p, neg.reshape(-1, L), margin=margin, p=2, reduction="mean")
    log_sim = F.log_softmax(sim_diff[:, :, 0].reshape(1, -1) / temp, dim=1)
    soft = (-F.softmax(label[:, :, 0].reshape(1, -1) / temp, dim=1) * log_sim).mean(0).sum()
    opt.zero_grad()
    (hard + 0.5 * soft).backward()
    opt.step()
    losses.append((float(hard.detach()), float(soft.detach())))


t_step = median_us(sfrs_step, warm=2)
say(f"one SFRS step, 12 + 11 images of 480 x 640, trunk in {model.base_model.effective_precision(easy)}, conv5 + NetVLAD "
    f"trained in fp32 (2 student passes, 1 frozen pass, both losses in torch, backward, SGD): {t_step / 1e3:7.1f} ms; "
    f"loss_hard {losses[0][0]:.4f} -> {losses[-1][0]:.4f}, loss_soft {losses[0][1]:.4f} -> {losses[-1][1]:.4f}")
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
