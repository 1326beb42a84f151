"""The cases of tests/golden/netvlad_k.npz (NetVLAD head for cluster counts other than 64) and how their inputs are
drawn: shared by the generator (make_netvlad_k_golden.py) and the tests, so both sides hold the same arrays."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from . import netvlad_grad_ref as ref

GOLDEN = Path(__file__).resolve().parent.parent / "golden" / "netvlad_k.npz"
QUANTITIES = ("vlad_raw", "vlad_norm", "dW", "dC", "dX")
STRIDE = 29          # stored: every 29th element of a flattened array (co-prime with 32, 512 and every K)


def _case(name, kind, seed, K, N, h, w, normalize=True, jitter=0.0, sharpen=1.0):
    return dict(name=name, kind=kind, seed=seed, K=K, N=N, h=h, w=w, normalize=normalize, jitter=jitter,
                sharpen=sharpen)


CASES = (
    _case("k16_2x3x5_norm", "plain", 71, 16, 2, 3, 5),
    _case("k48_3x6x8_norm", "plain", 72, 48, 3, 6, 8),
    _case("k128_2x5x7_norm", "plain", 73, 128, 2, 5, 7),
    _case("k32_1x8x8_raw", "plain", 74, 32, 1, 8, 8, normalize=False),
    _case("k32_tuple_4x4x4", "tuple", 75, 32, 4, 4, 4, jitter=0.03),
    _case("k32_saturated_2x8x8", "trained", 76, 32, 2, 8, 8, sharpen=4.0),
)
BY_NAME = {c["name"]: c for c in CASES}


def draw_case(case):
    """(x [N][h][w][512], w [K][512], c [K][512], G [N][K*512], info) of a case, float32."""
    K, N, h, w = case["K"], case["N"], case["h"], case["w"]
    if case["kind"] == "plain":
        return (*ref.draw_inputs(case["seed"], N, h, w, K=K), {})
    if case["kind"] == "tuple":       # one tuple of 1 + 1 + 2 images
        x, wt, c, G, info = ref.draw_tuple_inputs(case["seed"], 1, N, h, w, case["jitter"], K=K)
        return x, wt, c, G, {k: info[k] for k in ("alpha", "mean_max_a", "min_A", "cancellation")}
    x, wt, c, G, info = ref.draw_trained_inputs(case["seed"], N, h, w, sharpen=case["sharpen"], populate=True, K=K)
    return x, wt, c, G, {k: info[k] for k in ("alpha", "mean_max_a", "min_A")}


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def stored_error(golden, name, q, got) -> float:
    """max |got - float64| over the stored elements of quantity q, relative to max |float64| over the full array."""
    got = np.asarray(got, dtype=np.float64).ravel()[::STRIDE]
    return float(np.abs(got - golden[f"{name}.{q}"]).max() / float(golden[f"{name}.{q}_max"]))
