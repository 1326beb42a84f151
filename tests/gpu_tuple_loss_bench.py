"""The fused losses against the same losses written in torch (diagnostic, not a pytest): HIP-event medians of 7 warm
batches, forward + backward, on the same device in the same run.
  tuple losses   B = 4, M = 10, L = 32768 in the five modes (triplet; SARE joint / ind on -|a - x|^2 and on <a, x> / temp)
  soft label     (B, J) = (4, 90)
  hard loss      generation >= 1, B = 4: one argmax + one gather + one fused call against the reference's per-tuple loop
  whole steps    12 images of 480 x 640, frozen backbone and train_layers='conv5' (forward, triplet loss, backward), and
                 the SFRS step on 12 + 11 images (2 student passes, 1 frozen pass, both losses, backward, SGD) — each
                 with the fused losses and with the torch-written ones
Launch counts come from torch.profiler where it is available.
    python tests/gpu_tuple_loss_bench.py [output file]"""
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import models, ops, synth  # noqa: E402

dev = torch.device("cuda", 0)
L = 64 * 512
TEMP, MARGIN = 0.07, 0.1 ** 0.5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def flush_file():
    if len(sys.argv) > 1:
        Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
        Path(sys.argv[1]).write_text("\n".join(lines) + "\n")


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


def launches(fn):
    """Kernel launches of one call of fn, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA
                   and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower())
    except Exception as e:                                   # a diagnostic: the timings stand without it
        say(f"  (no launch count: {type(e).__name__})")
        return None


def torch_tuple_loss(a, p, n, kind, score):
    """The losses as the README writes them (the reference's formulas in torch)."""
    B, M, _ = n.shape
    if kind == "triplet":
        aa = a.unsqueeze(1).expand_as(n).reshape(-1, L)
        pp = p.unsqueeze(1).expand_as(n).reshape(-1, L)
        return F.triplet_margin_loss(aa, pp, n.reshape(-1, L), margin=MARGIN, p=2, reduction="mean")
    if score == "sqdist":
        z_pos = -((a - p) ** 2).sum(1).view(B, 1)
        z_neg = -((a.unsqueeze(1) - n) ** 2).sum(2)
    else:
        z_pos = (a * p).sum(1).view(B, 1) / TEMP
        z_neg = torch.bmm(n, a.unsqueeze(2)).squeeze(2) / TEMP
    if kind == "sare_joint":
        return (-F.log_softmax(torch.cat((z_pos, z_neg), 1), 1)[:, 0]).mean()
    pair = torch.stack((z_pos.expand_as(z_neg), z_neg), 2).view(-1, 2)
    return (-F.log_softmax(pair, 1)[:, 0]).mean()


def torch_soft(s, t, ts, tt):
    return (-F.softmax(t / tt, dim=1).detach() * F.log_softmax(s / ts, dim=1)).mean(0).sum()


def torch_hard_loop(vec, score, kind):
    """The reference's generation >= 1 loop (ibl/trainers.py:250-254, 261-270) in torch."""
    B, M = score.shape[:2]
    loss = 0
    for t in range(B):
        negatives = vec[t, 2:]
        arg = score[t].argmax(1)[:, None, None].expand_as(negatives).contiguous()
        sel = torch.gather(negatives, 1, arg)[:, 0]
        loss = loss + torch_tuple_loss(vec[t, 0, 0][None].contiguous(), vec[t, 1, 0][None].contiguous(),
                                       sel[None].contiguous(), kind, "dot")
    return loss / B


def fused_hard(vec, score, kind):
    B, M = score.shape[:2]
    arg = score.argmax(-1)
    sel = torch.gather(vec[:, 2:], 2, arg.view(B, M, 1, 1).expand(B, M, 1, L))[:, :, 0]
    return ops.tuple_loss(vec[:, 0, 0], vec[:, 1, 0], sel, kind, margin=MARGIN, temp=TEMP, score="dot")


def fwd_bwd(loss_fn, leaves):
    def step():
        for t in leaves:
            t.grad = None
        loss_fn().backward()
    return step


say(f"fused losses against torch-written ones, {torch.cuda.get_device_name(0)}; medians of 7 warm batches, forward + "
    f"backward, us; launches per forward + backward in brackets")
g = torch.Generator(device=dev).manual_seed(7)
B, M = 4, 10
x = F.normalize(torch.randn((B, 1, L), generator=g, device=dev) +
                torch.tensor([0.0, 0.45] + [0.25 + 0.12 * j for j in range(M)], device=dev)[None, :, None] *
                torch.randn((B, 2 + M, L), generator=g, device=dev), dim=-1).requires_grad_(True)
slower = []
for kind, score in (("triplet", "sqdist"), ("sare_joint", "sqdist"), ("sare_joint", "dot"), ("sare_ind", "sqdist"),
                    ("sare_ind", "dot")):
    fused = fwd_bwd(lambda: ops.tuple_loss(x[:, 0], x[:, 1], x[:, 2:], kind, margin=MARGIN, temp=TEMP, score=score), [x])
    plain = fwd_bwd(lambda: torch_tuple_loss(x[:, 0], x[:, 1], x[:, 2:], kind, score), [x])
    tf, tp = median_us(fused), median_us(plain)
    say(f"  {kind:10s} {score:6s} B = {B}, M = {M}, L = {L}: fused {tf:7.1f} [{launches(fused)}] | torch {tp:7.1f} "
        f"[{launches(plain)}] | ratio {tp / tf:5.2f}")
    if tf > tp:
        slower.append(f"{kind} {score}")
s_ = (torch.rand((4, 90), generator=g, device=dev) * 0.3 + 0.2).requires_grad_(True)
t_ = torch.rand((4, 90), generator=g, device=dev) * 0.3 + 0.2
fused = fwd_bwd(lambda: ops.soft_label_loss(s_, t_, TEMP, 0.06), [s_])
plain = fwd_bwd(lambda: torch_soft(s_, t_, TEMP, 0.06), [s_])
tf, tp = median_us(fused), median_us(plain)
say(f"  soft label (4, 90): fused {tf:7.1f} [{launches(fused)}] | torch {tp:7.1f} [{launches(plain)}] | ratio {tp / tf:5.2f}")
if tf > tp:
    slower.append("soft label")
vec = F.normalize(torch.randn((B, 2 + M, 9, L), generator=g, device=dev), dim=-1).requires_grad_(True)
sc = torch.rand((B, M, 9), generator=g, device=dev)
for kind in ("triplet", "sare_ind", "sare_joint"):
    fused = fwd_bwd(lambda: fused_hard(vec, sc, kind), [vec])
    plain = fwd_bwd(lambda: torch_hard_loop(vec, sc, kind), [vec])
    tf, tp = median_us(fused), median_us(plain)
    say(f"  hard loss, generation >= 1, {kind:10s} B = {B}: argmax + gather + fused {tf:7.1f} [{launches(fused)}] | the "
        f"per-tuple loop in torch {tp:7.1f} [{launches(plain)}] | ratio {tp / tf:5.2f}")
    if tf > tp:
        slower.append(f"hard loss {kind}")
flush_file()
del vec, x
torch.cuda.empty_cache()

sd = {k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")}


def make(arch):
    base = models.create("vgg16", pretrained=False)
    pool = models.create("netvlad", dim=base.feature_dim)
    m = models.create(arch, base, pool, tuple_size=1) if arch == "embedregionnet" else models.create(arch, base, pool)
    m.load_state_dict(sd)
    return m.to(dev).train()


images = synth.images(23, 480, 640, seed=5).to(dev)
x12 = images[:12].contiguous()
net = make("embednet")
for layers, parent in ((None, 4.6), ("conv5", 9.4)):
    def step(fused):
        net.zero_grad(set_to_none=True)
        out = net.forward_train(x12, train_layers=layers)[1].view(1, 12, -1)
        loss = ops.tuple_loss(out[:, 0], out[:, 1], out[:, 2:], "triplet", margin=MARGIN) if fused else \
            torch_tuple_loss(out[:, 0], out[:, 1], out[:, 2:], "triplet", "sqdist")
        loss.backward()
    tf, tp = median_us(lambda: step(True), warm=2), median_us(lambda: step(False), warm=2)
    say(f"one step, 12 images of 480 x 640, trunk in {net.base_model.effective_precision(x12)}, train_layers={layers!r} "
        f"(forward, triplet loss, backward): fused loss {tf / 1e3:6.2f} ms | torch-written loss {tp / 1e3:6.2f} ms "
        f"(the parent commit's figure: {parent} ms)")
    if tf > 1.03 * tp:
        slower.append(f"step {layers}")
del net
torch.cuda.empty_cache()

model, cache = make("embedregionnet"), make("embedregionnet")
easy, diff = images[:12].contiguous(), torch.cat([images[:1], images[12:]], dim=0).contiguous()
params = [p for i in (24, 26, 28) for p in model.base_model.base[i].parameters()] + list(model.net_vlad.parameters())
opt = torch.optim.SGD(params, lr=1e-4, momentum=0.9)


def sfrs_step(fused):
    """One generation-0 step of SFRSTrainer.train with the 'triplet' loss, as tests/gpu_region_backward_bench.py."""
    _, va, vp = model.forward_train(easy, train_layers="conv5")
    with torch.no_grad():
        label, _, _ = cache.region_similarity(diff)
    sim_diff, _, _ = model.forward_train(diff, train_layers="conv5")
    a, p, n = va[:, 0, 0], vp[:, 0, 0], vp[:, 1:, 0]
    s, t = sim_diff[:, :, 0].reshape(1, -1), label[:, :, 0].reshape(1, -1)
    if fused:
        hard = ops.tuple_loss(a, p, n, "triplet", margin=MARGIN, temp=TEMP, score="dot")
        soft = ops.soft_label_loss(s, t, TEMP, TEMP)
    else:
        hard, soft = torch_tuple_loss(a, p, n, "triplet", "dot"), torch_soft(s, t, TEMP, TEMP)
    opt.zero_grad()
    (hard + 0.5 * soft).backward()
    opt.step()
    return float(hard.detach()), float(soft.detach())


tf, tp = median_us(lambda: sfrs_step(True), warm=2), median_us(lambda: sfrs_step(False), warm=2)
say(f"one SFRS step, 12 + 11 images of 480 x 640, conv5 + NetVLAD trained in fp32 (2 student passes, 1 frozen pass, both "
    f"losses, backward, SGD): fused losses {tf / 1e3:6.2f} ms | torch-written losses {tp / 1e3:6.2f} ms (the parent "
    f"commit's figure: 22.6 ms)")
if tf > 1.03 * tp:
    slower.append("SFRS step")
say("slower than the torch-written loss: " + (", ".join(slower) if slower else "none"))
flush_file()
