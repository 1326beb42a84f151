"""The SFRS region head behind the conv5_3 map at the SFRS tuple sizes (diagnostic, not a pytest):
  (a) the region head of csrc/region.hip: ops.region_vlad + ops.region_scores (4 launches, the map read once);
  (b) the same result composed from what the package had before it: the four quarter maps gathered with torch,
      ops.netvlad(want_raw=True) on them, then torch for the region sums, the two normalisations and the bmm;
both in one process, warm, HIP events over enough iterations to be far above the timer's resolution, (b) repeated to
show its run-to-run spread; then the share of a whole EmbedRegionNet.region_similarity call that the head takes.
    python tests/gpu_region_bench.py"""
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


def timed(fn, iters=100):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def new_head(feat, T):
    vec = ops.region_vlad(feat, cw, cent, True)
    return ops.region_scores(vec, T), vec


def composed(feat, T):
    N, h, w, C = feat.shape
    hh, hw = h // 2, w // 2
    q = torch.stack([feat[:, r * hh:(r + 1) * hh, c * hw:(c + 1) * hw] for r in (0, 1) for c in (0, 1)], dim=1)
    raw, _ = ops.netvlad(q.reshape(N * 4, hh, hw, C).contiguous(), cw, cent, True, want_raw=True, want_norm=False)
    raw = raw.view(N, 4, 64, C)
    reg = torch.cat([raw.sum(1, keepdim=True),
                     torch.stack((raw[:, 0] + raw[:, 1], raw[:, 2] + raw[:, 3], raw[:, 0] + raw[:, 2],
                                  raw[:, 1] + raw[:, 3]), dim=1), raw], dim=1)
    vec = F.normalize(F.normalize(reg, p=2, dim=3).view(N, 9, -1), p=2, dim=2)
    v = vec.view(T, N // T, 9, -1)
    a = v[:, :1].expand(-1, N // T - 1, -1, -1).reshape(-1, 9, v.shape[-1])
    score = torch.bmm(a, v[:, 1:].reshape(-1, 9, v.shape[-1]).transpose(1, 2)).view(T, -1, 9, 9)
    return score, vec


g = torch.Generator(device=dev).manual_seed(3)
for N, T in ((12, 1), (48, 4)):
    feat = torch.randn((N, 30, 40, 512), generator=g, device=dev) * 3.0
    sa, va = new_head(feat, T)
    sb, vb = composed(feat, T)
    dv = float(((va - vb).norm(dim=-1) / vb.norm(dim=-1)).max())
    ds = float((sa - sb).abs().max())
    t_vec = timed(lambda: ops.region_vlad(feat, cw, cent, True))
    t_sc = timed(lambda: ops.region_scores(va, T))
    runs_a = [timed(lambda: new_head(feat, T)) for _ in range(5)]
    runs_b = [timed(lambda: composed(feat, T)) for _ in range(5)]
    print(f"N = {N:2d}, tuple_size {T} (30 x 40 x 512 map, fp32): region head {min(runs_a):7.1f} .. {max(runs_a):7.1f} us "
          f"(vectors {t_vec:6.1f} + scores {t_sc:5.1f}) | composed from ops.netvlad + torch "
          f"{min(runs_b):7.1f} .. {max(runs_b):7.1f} us (spread {max(runs_b) - min(runs_b):5.1f}) | "
          f"ratio {min(runs_b) / max(runs_a):.2f}x | max vector rel-L2 between them {dv:.2e}, max |dscore| {ds:.2e}",
          flush=True)

# the share of the head in a whole region_similarity call at the SFRS tuple (1 + 1 + 10 images of 480 x 640)
base = models.create("vgg16", pretrained=False)
net = models.create("embedregionnet", base, models.create("netvlad", dim=base.feature_dim), tuple_size=1)
net.load_state_dict({k: v for k, v in sd.items() if not k.startswith("pca_layer")})
net = net.to(dev).eval()
x = synth.images(12, 480, 640, seed=5).to(dev)
for prec in ("f16mx", "fp32"):
    net.set_precision(prec)
    feat = net.base_model.features_nhwc(x)
    t_all = timed(lambda: net.region_similarity(x), iters=20)
    t_head = timed(lambda: net._region_head(feat), iters=100)
    print(f"region_similarity, 12 images of 480 x 640, {prec}: {t_all / 1e3:7.3f} ms per call "
          f"({t_all / 12e3:.3f} ms per image), of which the region head {t_head:6.1f} us = {100 * t_head / t_all:.1f} %",
          flush=True)
