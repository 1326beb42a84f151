"""conv5 training at training batches (diagnostic, not a pytest): HIP-event medians of 7 warm batches.
  * per layer, a 30 x 40 x 512 map at 12 and 48 images: weight, bias and input gradient of ops.conv3x3_backward alone
    and together, with the fraction of the 155 TFLOP/s fp32 matrix rate the two contractions reach;
  * the whole training step — forward + backward of EmbedNet.forward_train(x, 'conv5') under the triplet loss — next to
    today's frozen forward_train, 12 images of 480 x 640;
  * torch autograd of the same three F.conv2d layers on the same device, with its peak memory (where it runs).
    python tests/gpu_conv_backward_bench.py [output file]"""
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))
from helpers import conv_grad_ref as ref  # noqa: E402
from openibl_amd import models, ops, synth  # noqa: E402

dev = torch.device("cuda", 0)
PEAK = 155e12
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


sd = synth.embednetpca_state(0)
w5 = [sd[f"base_model.base.{i}.weight"].to(dev) for i in (24, 26, 28)]
b5 = [sd[f"base_model.base.{i}.bias"].to(dev) for i in (24, 26, 28)]
g = torch.Generator(device=dev).manual_seed(5)
say(f"conv3x3 backward, 30 x 40 x 512 fp32 map, Cin = Cout = 512, {torch.cuda.get_device_name(0)}; "
    f"medians of 7 warm batches, us")
for N in (12, 48):
    x = torch.randn((N, 30, 40, 512), generator=g, device=dev).clamp_min_(0)
    G = torch.randn((N, 30, 40, 512), generator=g, device=dev)
    act = ops.conv3x3_nhwc(x, ops.pack_conv3x3(w5[0], "fp32"), b5[0], True, False, "fp32")
    t = {k: median_us(lambda k=k: ops.conv3x3_backward(x, w5[0], G, out_act=act, want=k))
         for k in (("w",), ("b",), ("x",), ("w", "b", "x"))}
    t_plain = median_us(lambda: ops.conv3x3_backward(x, w5[0], G, want=("w", "b", "x")))
    t_fwd = median_us(lambda: ops.conv3x3_nhwc(x, ops.pack_conv3x3(w5[0], "fp32"), b5[0], True, False, "fp32"))
    flop = 2.0 * N * 1200 * 512 * 512 * 9
    ws = ops._lib.load().oibl_conv3x3_backward_workspace_bytes(N, 30, 40, 512, 512, 1) / 2 ** 20
    say(f"N = {N:2d}: dW {t[('w',)]:8.1f} ({flop / t[('w',)] / 1e-6 / PEAK * 100:4.1f} % of 155 TFLOP/s) | db {t[('b',)]:7.1f} | "
        f"dX {t[('x',)]:8.1f} ({flop / t[('x',)] / 1e-6 / PEAK * 100:4.1f} %) | dW db dX {t[('w', 'b', 'x')]:8.1f} "
        f"(without out_act {t_plain:8.1f}; workspace {ws:6.1f} MiB) | forward layer (pack + conv) {t_fwd:8.1f}")

    # torch autograd of the three layers on the same device
    try:
        xt = x.permute(0, 3, 1, 2).contiguous()
        wt = [w.clone().requires_grad_(True) for w in w5]
        bt = [b.clone().requires_grad_(True) for b in b5]
        Gt = G.permute(0, 3, 1, 2).contiguous()

        def torch_step():
            for p in wt + bt:
                p.grad = None
            a = xt
            for i in range(3):
                a = F.conv2d(a, wt[i], bt[i], padding=1)
                if i < 2:
                    a = F.relu(a)
            a.backward(Gt)

        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t_torch = median_us(torch_step, warm=2)
        peak = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        xd = x.clone()
        wd = [w.clone().requires_grad_(True) for w in w5]
        bd = [b.clone().requires_grad_(True) for b in b5]

        def own_step():
            for p in wd + bd:
                p.grad = None
            a = xd
            for i in range(3):
                a = ops.conv3x3_train(a, wd[i], bd[i], relu=i < 2)
            a.backward(G)

        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t_own = median_us(own_step, warm=2)
        peak_own = (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20
        say(f"        three layers forward + backward: conv3x3_train {t_own:9.1f} (peak {peak_own:6.0f} MiB beyond the "
            f"inputs, workspaces kept) | torch autograd of F.conv2d {t_torch:9.1f} (peak {peak:6.0f} MiB)")
        del wt, bt, wd, bd
    except Exception as e:  # torch's convolution backend may be missing on a machine
        say(f"        torch autograd of F.conv2d did not run here: {type(e).__name__}: {str(e)[:120]}")
    torch.cuda.empty_cache()

say("whole training step, EmbedNet on 12 images of 480 x 640 (3 tuples x 4), triplet loss, forward + backward, us")
state = {k: v for k, v in sd.items() if not k.startswith("pca_layer")}
imgs = synth.images(12, 480, 640, seed=7).to(dev)
for prec in ("f16mx", "fp32"):
    model = models.EmbedNet(models.vgg16(pretrained=False), models.NetVLAD())
    model.load_state_dict(state)
    model = model.to(dev).set_precision(prec).train()

    def step(layers):
        model.zero_grad(set_to_none=True)
        ref.tuple_loss(model.forward_train(imgs, train_layers=layers)[1], 3, 4).backward()

    t_frozen = median_us(lambda: step(None))
    t_conv5 = median_us(lambda: step("conv5"))
    t_eval = median_us(lambda: model(imgs))
    say(f"  {prec:6s}: frozen backbone (NetVLAD only) {t_frozen:9.1f} | train_layers='conv5' {t_conv5:9.1f} | "
        f"eval forward {t_eval:9.1f}")
    del model
    torch.cuda.empty_cache()
if len(sys.argv) > 1:
    Path(sys.argv[1]).parent.mkdir(parents=True, exist_ok=True)
    Path(sys.argv[1]).write_text("\n".join(lines) + "\n")
