"""The device colour jitter at the training shape (diagnostic, not a pytest): 12 and 48 images of 480 x 640, both
output kinds, ColorJitter(0.7, 0.7, 0.7, 0.5) records.  In one process, warm, the median of 7 with the spread:
  (a) ops.color_jitter by HIP events, and the bytes/s it achieves against the bytes its launches must move (the
      partial-sum launch reads the batch once, the apply launch reads it again and writes the output);
  (b) the same call with parts of the work taken out — no records (the plain normalisation), records without the
      hue op, records with hue alone — which says whether memory or arithmetic bounds the pass;
  (c) PIL on the host, one thread, the same records on the same images, per image;
  (d) a Trainer step (conv5 + NetVLAD trainable, one tuple of 12 images, 480 x 640: parse, forward, backward, SGD
      step, by the wall clock with the device drained) fed float tuples without `augment` and uint8 tuples with it.
    python tests/gpu_color_jitter_bench.py"""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from helpers import color_jitter_ref as ref  # noqa: E402
from openibl_amd import ops, synth  # noqa: E402
from openibl_amd.augment import ColorJitter  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W = 480, 640
REPS = 7


def spread(runs, unit):
    return f"median {statistics.median(runs):9.4f} {unit} (min {min(runs):.4f}, max {max(runs):.4f})"


def events(fn, reps=REPS):
    fn()
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        runs.append(s.elapsed_time(e))
    return runs


def images(n, seed):
    """Smooth structure plus noise, as a photograph has: every hue sector, dark and saturated pixels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 120 * np.sin(xx / 37.0 + c) * np.cos(yy / 53.0 - c) for c in range(3)], -1)
    return np.clip(base[None] + rng.normal(0, 25, (n, H, W, 3)), 0, 255).astype(np.uint8)


def device_bench(n):
    x_host = images(n, n)
    x = torch.from_numpy(x_host).to(dev)
    jit = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(n))
    rec_host = jit.draw(n)
    rec = rec_host.to(dev)
    no_hue, only_hue = rec_host.clone(), rec_host.clone()
    no_hue[:, :4][no_hue[:, :4] == 3] = -1
    only_hue[:, :4][only_hue[:, :4] != 3] = -1
    px = n * H * W
    print(f"---- {n} images of {H} x {W} ----", flush=True)
    for out, out_bytes in (("float", 12), ("uint8", 3)):
        for label, r, reads in (("full jitter", rec, 2), ("no hue op", no_hue.to(dev), 2),
                                ("hue op alone", only_hue.to(dev), 1), ("no records (plain pass)", None, 1)):
            runs = events(lambda: ops.color_jitter(x, r, out=out))
            moved = px * (3 * reads + out_bytes)
            med = statistics.median(runs)
            print(f"ops.color_jitter out={out:5s} {label:24s}: {spread(runs, 'ms')}; {moved / 1e6:7.1f} MB moved, "
                  f"{moved / med / 1e6:7.1f} GB/s; {px / med / 1e3:7.1f} Mpixel/s", flush=True)
    # the bits, once, at this shape too
    got = ops.color_jitter(x[:2], rec[:2], out="uint8").cpu().numpy()
    print(f"bit-equal to PIL on the first two images: {np.array_equal(got, ref.pil_jitter_records(x_host[:2], rec_host[:2].numpy()))}",
          flush=True)
    return x_host, rec_host


def host_bench(x_host, rec_host):
    runs = []
    for i in range(REPS):
        args = ref.unpack_record(rec_host[i].numpy())
        t0 = time.perf_counter()
        ref.pil_jitter(x_host[i], *args)
        runs.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(runs)
    print(f"PIL on the host, one thread, one image of {H} x {W} (array -> Image -> four ops -> array): "
          f"{spread(runs, 'ms')}; {1e3 / med:.1f} images/s per thread", flush=True)


def trainer_bench():
    from ibl import models
    from ibl.trainers import Trainer
    B, per_tuple = 1, 12
    base = models.create("vgg16", pretrained=False, train_layers="conv5")
    pool = models.create("netvlad", dim=base.feature_dim)
    model = models.create("embednet", base, pool)
    model.load_state_dict({k: v for k, v in synth.embednetpca_state(0).items() if not k.startswith("pca_layer")})
    for layer in list(base.base.children())[:type(base)._fix_layers["conv5"]]:
        for p in layer.parameters():
            p.requires_grad_(False)
    model = model.to(dev).train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-6, momentum=0.9)
    raw = torch.from_numpy(images(B * per_tuple, 99)).view(B, per_tuple, H, W, 3)
    u8_batch = [(raw[:, j].contiguous().pin_memory(), ["name"] * B) for j in range(per_tuple)]
    flt = ref.host_normalize(raw.view(-1, H, W, 3)).view(B, per_tuple, 3, H, W)
    f32_batch = [(flt[:, j].contiguous().pin_memory(), ["name"] * B) for j in range(per_tuple)]
    jit = ColorJitter(0.7, 0.7, 0.7, 0.5, generator=torch.Generator().manual_seed(5))
    print(f"---- Trainer step, {B} tuple of {per_tuple} images of {H} x {W}, precision {getattr(model.base_model, 'precision', '?')} ----",
          flush=True)
    for label, augment, batch in (("float tuples, no augment", None, f32_batch), ("uint8 tuples, augment", jit, u8_batch),
                                  ("float tuples, no augment", None, f32_batch), ("uint8 tuples, augment", jit, u8_batch)):
        trainer = Trainer(model, margin=0.1 ** 0.5, gpu=dev.index, augment=augment)

        def step(parse_only=False):
            inputs = trainer._parse_data(batch)
            if parse_only:
                return
            loss = trainer._forward(inputs, True, "triplet")
            opt.zero_grad()
            loss.backward()
            opt.step()
        for _ in range(3):
            step()
        whole, parse = [], []
        for _ in range(REPS):
            for runs, flag in ((whole, False), (parse, True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(flag)
                torch.cuda.synchronize()
                runs.append((time.perf_counter() - t0) * 1e3)
        print(f"{label:26s}: step {spread(whole, 'ms')}; of it _parse_data (stack, copy to the device"
              f"{', jitter' if augment else ''}) {spread(parse, 'ms')}", flush=True)


if __name__ == "__main__":
    print(f"{torch.cuda.get_device_name(dev)}, torch {torch.__version__}", flush=True)
    x12, r12 = device_bench(12)
    device_bench(48)
    host_bench(x12, r12)
    trainer_bench()
