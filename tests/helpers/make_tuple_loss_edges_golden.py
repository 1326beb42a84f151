"""Generate tests/golden/tuple_loss_edges.npz by running THE REFERENCE's losses under torch autograd on the CPU, in
float64, on the regime cases of the edge suite (tests/helpers/tuple_loss_ref.EDGE_GOLDEN and EDGE_SOFT_GOLDEN, at their
small shapes): hard negatives dominating (r1), the positive dominating (r2), coincident rows (r3), whole tuples
switched on by a margin of +10 or off by their geometry (r4; torch refuses the margin of -10 that switches a whole
case off), an upstream gradient of -2 (r5), and the soft-label loss at the edges of its 256-thread stride (s1), with
one-hot teachers and students (s2) and with the student equal to the teacher (s3).

Run in the build container only (`python tests/helpers/make_tuple_loss_edges_golden.py`): the reference tree is
imported through oracle.refshim, as tests/helpers/make_tuple_loss_golden.py does, and does not exist on the GPU box.

  Trainer(margin)._get_loss(outputs [B (2 + M)][L], loss_type, B, 2 + M)            triplet, joint_sqdist, ind_sqdist
  SFRSTrainer(margin, temp=[0.07])._get_loss(anchors, positives, negatives, B, .)  triplet_m03, joint_dot, ind_dot
  the soft term of SFRSTrainer._forward (ibl/trainers.py:256-257) on score tables [B][J]
Stored per case and mode: the float64 loss and samples (tuple_loss_ref.sample, EDGE_SAMPLE values) of the three float64 gradients of
EDGE_SCALE[case] x loss (1 where the case has no scale).  Data only: no fp32 error is stored, the device's bar in these
regimes is derived (2^-23 + 4 L 2^-53 S), not taken from the reference's fp32 run.  tests/test_tuple_loss_cpu.py holds
the float64 helper to these numbers, so the conventions that matter here — clamp_min at an inactive hinge, the 1e-6 of
pairwise_distance between coincident rows, log_softmax where one term carries the sum — are the reference's."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))

from oracle import refshim  # noqa: E402

refshim.install()  # puts the reference FIRST on sys.path: `import ibl` below is the reference

sys.path.insert(0, str(ROOT / "tests"))
from helpers import tuple_loss_ref as ref  # noqa: E402

OUT = ROOT / "tests" / "golden" / "tuple_loss_edges.npz"


def _run_rows(trainers, name, mode, scale):
    """The reference in float64 on the case's rows -> (loss, ga, gp, gn) of scale x loss as numpy."""
    kind, _, margin, temp, which = ref.edge_mode(name, mode)
    a, p, n = (torch.from_numpy(np.ascontiguousarray(t)).double() for t in ref.edge_rows(name, mode))
    B, M, L = n.shape
    if which == "Trainer":
        out = torch.cat((a[:, None], p[:, None], n), dim=1).reshape(B * (2 + M), L).requires_grad_(True)
        loss = trainers.Trainer(None, margin=margin)._get_loss(out, kind, B, 2 + M)
        (scale * loss).backward()
        g = out.grad.view(B, 2 + M, L)
        return float(loss.detach()), g[:, 0].numpy(), g[:, 1].numpy(), g[:, 2:].numpy()
    a, p, n = a.requires_grad_(True), p.requires_grad_(True), n.requires_grad_(True)
    loss = trainers.SFRSTrainer(None, None, margin=margin, neg_num=M, temp=[temp])._get_loss(a, p, n, B, kind)
    (scale * loss).backward()
    return float(loss.detach()), a.grad.numpy(), p.grad.numpy(), n.grad.numpy()


def _soft_run(s, t, ts, tt):
    s = torch.from_numpy(np.ascontiguousarray(s)).double().requires_grad_(True)
    t = torch.from_numpy(np.ascontiguousarray(t)).double()
    F = torch.nn.functional
    log_sim = F.log_softmax(s / ts, dim=1)
    loss = (-F.softmax(t / tt, dim=1).detach() * log_sim).mean(0).sum()
    loss.backward()
    return float(loss.detach()), s.grad.numpy()


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import trainers

    torch.set_num_threads(8)
    store = {}
    for name in ref.EDGE_GOLDEN:
        seed, B, M, L, _ = ref.EDGE_CASES[name]
        scale = ref.EDGE_SCALE.get(name, 1.0)
        store[f"{name}_seed"], store[f"{name}_shape"] = np.array(seed), np.array([B, M, L])
        store[f"{name}_scale"] = np.array(scale)
        for mode in ref.edge_modes(name):
            loss, ga, gp, gn = _run_rows(trainers, name, mode, scale)
            assert np.isfinite(loss) and all(np.isfinite(g).all() for g in (ga, gp, gn)), (name, mode)
            print(f"{name} {mode}: float64 loss {loss:.12g}; max |da| |dp| |dn| "
                  + " ".join(f"{np.abs(g).max():.3e}" for g in (ga, gp, gn)))
            store[f"{name}_{mode}_loss"] = np.array(loss)
            for k, g in zip(("da", "dp", "dn"), (ga, gp, gn)):
                store[f"{name}_{mode}_{k}"] = ref.sample(g, ref.EDGE_SAMPLE)
    for name in ref.EDGE_SOFT_GOLDEN:
        seed, B, J, ts, tt, _ = ref.EDGE_SOFT[name]
        loss, ds = _soft_run(*ref.edge_soft(name), ts, tt)
        assert np.isfinite(loss) and np.isfinite(ds).all(), name
        print(f"soft {name}: float64 loss {loss:.12g}; max |ds| {np.abs(ds).max():.3e}")
        store[f"soft_{name}_seed"], store[f"soft_{name}_shape"] = np.array(seed), np.array([B, J])
        store[f"soft_{name}_temps"] = np.array([ts, tt])
        store[f"soft_{name}_loss"] = np.array(loss)
        store[f"soft_{name}_ds"] = ref.sample(ds, ref.EDGE_SAMPLE)
    np.savez_compressed(OUT, **store)
    assert OUT.stat().st_size < 200_000, OUT.stat().st_size
    print("file", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
