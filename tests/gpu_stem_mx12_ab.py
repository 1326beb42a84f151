"""Stem alone, batch 32 of 480x640: 12-wave kernel (hook 1) against the 16-wave kernel (hook 0), and role stamps."""
import sys
from pathlib import Path
import torch
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from openibl_amd import ops, lib
dev = torch.device("cuda", 0)
L = lib.debug_hooks()
N, H, W = 32, 480, 640
g = torch.Generator().manual_seed(0)
x = torch.randn((N, 3, H, W), generator=g).to(dev)
w1 = (torch.randn((64, 3, 3, 3), generator=g) * 0.2).to(dev)
b1 = torch.zeros(64, device=dev)
w2 = ops.pack_conv3x3((torch.randn((64, 64, 3, 3), generator=g) * 0.05).to(dev), "f16mx")
b2 = torch.zeros(64, device=dev)
buf = torch.zeros(8, dtype=torch.int64, device=dev)
tiles = N * ((H + 7) // 8) * ((W + 31) // 32) / 256
outs = {}
for rep in range(3):
    for mode in (1, 0):
        L.oibl_debug_set_stem_mx12(mode)
        for _ in range(5):
            o = ops.vgg16_stem_mx(x, w1, b1, w2, b2)
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(20):
            o = ops.vgg16_stem_mx(x, w1, b1, w2, b2)
        e.record()
        torch.cuda.synchronize()
        outs[mode] = o
        L.oibl_debug_set_prof_buffer(buf.data_ptr())
        ops.vgg16_stem_mx(x, w1, b1, w2, b2)
        torch.cuda.synchronize()
        L.oibl_debug_set_prof_buffer(None)
        t = buf.cpu().tolist()
        print(f"mx12={mode}: {s.elapsed_time(e) / 20:.3f} ms | consumer passes {t[0] / tiles:7.0f} waits {t[1] / tiles:6.0f} "
              f"epilogue {t[2] / tiles:6.0f} | producer work {t[4] / tiles:7.0f} waits {t[5] / tiles:6.0f} ticks/tile", flush=True)
print("equal:", torch.equal(outs[0], outs[1]))
L.oibl_debug_set_stem_mx12(1)
