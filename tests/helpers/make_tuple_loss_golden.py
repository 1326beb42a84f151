"""Generate tests/golden/tuple_loss.npz by running THE REFERENCE's losses under torch autograd on the CPU, in float32 and
in float64 on the same (fp32) inputs.

Run in the build container only (`python tests/helpers/make_tuple_loss_golden.py`): the reference tree is imported
through oracle.refshim, exactly as tests/helpers/make_region_backward_golden.py does, and does not exist on the GPU box.

Tuple cases (tests/helpers/tuple_loss_ref.CASES; inputs from the stored seeds: rows normalize(base_t + sigma noise),
anchor sigma 0, positive 0.45, negative j 0.25 + 0.12 j), each in the six modes of tuple_loss_ref.MODES:
  Trainer(margin)._get_loss(outputs [B (2 + M)][L], loss_type, B, 2 + M)            triplet, joint_sqdist, ind_sqdist
  SFRSTrainer(margin, temp=[0.07])._get_loss(anchors, positives, negatives, B, .)  triplet_m03, joint_dot, ind_dot
The `_regions` case is the generation >= 1 path: a [B][2 + M][9][L] tensor and a stored score [B][M][9]; the SFRS modes
run the reference's own loop, sum_t SFRSTrainer._get_hard_loss(vec[t, 0, 0], vec[t, 1, 0], vec[t, 2:], score[t], .) / B,
differentiated down to the [B][2 + M][9][L] tensor (the rows the loss does not read must get exactly zero); the Trainer
modes run on the selected rows.
Soft-label cases (tuple_loss_ref.SOFT_CASES): the soft term of SFRSTrainer._forward (ibl/trainers.py:256-257) on score
tables [B][J].
Stored per case and mode: the float64 loss, samples (tuple_loss_ref.sample) of the three float64 gradients, and `ref_err`:
the reference's own fp32-against-float64 error — |loss32 - loss64| / |loss64| and the relative max-norm of each fp32
gradient over the FULL tensor.  The device tests' bars are 8 x these figures.

Asserted here: in every triplet case with M >= 6 at least one hinge is active and one inactive; no hinge argument of
any triplet case lies within 1e-3 of zero in float64, so fp32 and float64 agree on the active set."""
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

OUT = ROOT / "tests" / "golden" / "tuple_loss.npz"
HINGE_GAP = 1e-3


def _run_rows(trainers, mode, a, p, n, dtype):
    """The reference on compact rows -> (loss, ga, gp, gn) as numpy in `dtype`."""
    kind, score, margin, temp, which = ref.MODES[mode]
    B, M, L = n.shape
    a, p, n = (torch.from_numpy(np.ascontiguousarray(t)).to(dtype) for t in (a, p, n))
    if which == "Trainer":
        out = torch.cat((a[:, None], p[:, None], n), dim=1).reshape(B * (2 + M), L).requires_grad_(True)
        loss = trainers.Trainer(None, margin=margin)._get_loss(out, kind, B, 2 + M)
        loss.backward()
        g = out.grad.view(B, 2 + M, L)
        return float(loss.detach()), g[:, 0].numpy(), g[:, 1].numpy(), g[:, 2:].numpy()
    a, p, n = a.requires_grad_(True), p.requires_grad_(True), n.requires_grad_(True)
    loss = trainers.SFRSTrainer(None, None, margin=margin, neg_num=M, temp=[temp])._get_loss(a, p, n, B, kind)
    loss.backward()
    return float(loss.detach()), a.grad.numpy(), p.grad.numpy(), n.grad.numpy()


def _run_regions(trainers, mode, vec, score, dtype):
    """The reference's generation >= 1 loop on the region tensor -> (loss, ga, gp, gn of the selected rows)."""
    kind, _, margin, temp, _ = ref.MODES[mode]
    B, M = score.shape[:2]
    v = torch.from_numpy(vec).to(dtype).requires_grad_(True)
    s = torch.from_numpy(score).to(dtype)
    t = trainers.SFRSTrainer(None, None, margin=margin, neg_num=M, temp=[temp])
    loss = 0
    for b in range(B):
        loss += t._get_hard_loss(v[b, 0, 0].contiguous(), v[b, 1, 0].contiguous(), v[b, 2:], s[b].contiguous(), kind)
    loss /= B
    loss.backward()
    g = v.grad.numpy()
    _, _, _, arg = ref.select_regions(vec, score)
    used = np.zeros(g.shape[:3], dtype=bool)
    used[:, :2, 0] = True
    used[np.arange(B)[:, None], 2 + np.arange(M)[None, :], arg] = True
    assert float(np.abs(g[~used]).max()) == 0.0                     # rows the loss does not read
    assert kind == "triplet" or np.abs(g[used]).max(-1).min() > 0.0  # (an inactive hinge leaves its negative at zero)
    return (float(loss.detach()),) + ref.select_regions(g, score)[:3]


def _soft_run(s, t, ts, tt, dtype):
    s = torch.from_numpy(s).to(dtype).requires_grad_(True)
    t = torch.from_numpy(t).to(dtype)
    F = torch.nn.functional
    log_sim = F.log_softmax(s / ts, dim=1)
    loss = (-F.softmax(t / tt, dim=1).detach() * log_sim).mean(0).sum()
    loss.backward()
    return float(loss.detach()), s.grad.numpy()


def _errors(got, want):
    return np.array([abs(got[0] - want[0]) / abs(want[0]) if want[0] != 0.0 else abs(got[0])] +
                    [ref.rel_max(g, w) for g, w in zip(got[1:], want[1:])])


def main():
    import ibl
    assert ibl.__file__.startswith(refshim.REFERENCE_ROOT), ibl.__file__
    from ibl import trainers

    torch.set_num_threads(8)
    store = {}
    for name, (seed, B, M, L, strided) in ref.CASES.items():
        store[f"{name}_seed"], store[f"{name}_shape"] = np.array(seed), np.array([B, M, L, int(strided)])
        if strided:
            vec, score = ref.draw_regions(seed, B, M, L)
            store[f"{name}_score"] = score
        a, p, n = ref.case_rows(name)
        for margin in (0.1 ** 0.5, 0.3):
            h = ref.hinge_arguments(a, p, n, margin)
            print(f"{name} margin {margin:.4f}: {int((h > 0).sum())} of {h.size} hinges active, min |h| {np.abs(h).min():.3e}")
            assert np.abs(h).min() >= HINGE_GAP, (name, margin, np.abs(h).min())
            assert M < 6 or (0 < int((h > 0).sum()) < h.size), (name, margin)
            store[f"{name}_hinge_{'m03' if margin == 0.3 else 'm'}"] = h
        for mode, (kind, score_kind, margin, temp, which) in ref.MODES.items():
            if strided and which == "SFRSTrainer":
                got, want = _run_regions(trainers, mode, vec, score, torch.float32), \
                    _run_regions(trainers, mode, vec, score, torch.float64)
            else:
                got, want = _run_rows(trainers, mode, a, p, n, torch.float32), \
                    _run_rows(trainers, mode, a, p, n, torch.float64)
            err = _errors(got, want)
            print(f"  {mode}: loss {got[0]:.9f} float64 {want[0]:.12f}; fp32 error loss | da | dp | dn "
                  + " ".join(f"{e:.3e}" for e in err))
            if kind == "triplet":                                  # fp32 and float64 agree on the active set
                assert np.array_equal(np.abs(got[3]).max(-1) > 0, np.abs(want[3]).max(-1) > 0)
            store[f"{name}_{mode}_loss"] = np.array(want[0])
            for k, g in zip(("da", "dp", "dn"), want[1:]):
                store[f"{name}_{mode}_{k}"] = ref.sample(g)
            store[f"{name}_{mode}_ref_err"] = err
    for name, (seed, B, J, ts, tt) in ref.SOFT_CASES.items():
        s, t = ref.draw_soft(seed, B, J)
        got, want = _soft_run(s, t, ts, tt, torch.float32), _soft_run(s, t, ts, tt, torch.float64)
        err = _errors(got, want)
        print(f"soft {name}: loss {got[0]:.9f} float64 {want[0]:.12f}; fp32 error loss | ds " + " ".join(f"{e:.3e}" for e in err))
        store[f"soft_{name}_seed"], store[f"soft_{name}_shape"] = np.array(seed), np.array([B, J])
        store[f"soft_{name}_temps"] = np.array([ts, tt])
        store[f"soft_{name}_loss"] = np.array(want[0])
        store[f"soft_{name}_ds"] = ref.sample(want[1])
        store[f"soft_{name}_ref_err"] = err
    np.savez_compressed(OUT, **store)
    assert OUT.stat().st_size < 1_000_000, OUT.stat().st_size
    print("file", OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
