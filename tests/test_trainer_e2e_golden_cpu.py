"""tests/golden/trainer_e2e.npz without a GPU and without the reference: the fixture's contract (keys, shapes, the
conditions its generator asserts, the file size) and a forward tie — every single-step loss recomputed in float64 from
the project's own pieces (oracle.descriptor, helpers/region_ref.py, helpers/tuple_loss_ref.py) matches the float64 loss
the reference's trainers gave, to 1e-9 relative.  That pins the file to the oracle the rest of the suite trusts and
checks the per-tuple stacking of two tuples independently of the generator's wrapper."""
import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from helpers import trainer_e2e_ref as ref

REF_ERR_MAX = 1.25e-5


@pytest.fixture(scope="module")
def golden():
    return load_golden("trainer_e2e")


@pytest.fixture(scope="module")
def maps(state_dict):
    """The float64 conv5 maps of the two single-step batches, computed once: ('trainer' | 'easy' | 'diff') -> maps."""
    imgs = ref.batch(ref.TRAINER_SHAPE, 0)
    easy, diff = ref.split(ref.batch(ref.SFRS_SHAPE, 0), ref.SFRS_SHAPE["neg_num"])
    return {k: ref.conv5_maps(v.reshape(-1, *v.shape[2:]), state_dict)
            for k, v in (("trainer", imgs), ("easy", easy), ("diff", diff))}


def test_fixture_contract(golden):
    g = golden
    assert (GOLDEN / "trainer_e2e.npz").stat().st_size < 1_000_000
    assert g["trainer_shape"].tolist() == [ref.TRAINER_SHAPE[k] for k in ("B", "n", "H", "W", "seed")]
    assert g["sfrs_shape"].tolist() == [ref.SFRS_SHAPE[k] for k in ("B", "neg_num", "n_diff", "H", "W", "seed")]
    assert float(g["margin"]) == ref.MARGIN and g["temp"].tolist() == ref.TEMP
    assert float(g["lambda_soft"]) == ref.LAMBDA_SOFT and g["sgd"].tolist() == [ref.MOMENTUM, ref.WEIGHT_DECAY]
    rows, hs = int(g["w_rows"]), int(g["head_stride"])
    shapes = {"dWv": (64 // hs, 512), "dCv": (64 // hs, 512),
              **{f"dW{i}": (rows, 512, 3, 3) for i in (1, 2, 3)}, **{f"db{i}": (512,) for i in (1, 2, 3)}}
    singles = {**{n: (1, ref.HEAD_KEYS if f else ref.KEYS) for n, (_, f) in ref.SINGLE_TRAINER.items()},
               **{n: (2, ref.KEYS) for n in ref.SINGLE_SFRS}}
    for name, (n_loss, keys) in singles.items():
        assert g[f"{name}_losses"].shape == (n_loss,) and g[f"{name}_losses"].dtype == np.float64, name
        assert (g[f"{name}_losses"] > 0).all()
        assert g[f"{name}_ref_err"].shape == (len(keys),) and 0 < g[f"{name}_ref_err"].max() <= REF_ERR_MAX, name
        assert g[f"{name}_loss_ref_err"].shape == (n_loss,) and g[f"{name}_loss_ref_err"].max() <= REF_ERR_MAX, name
        assert np.array_equal(g[f"{name}_losses32"].astype(np.float32), g[f"{name}_losses32"])
        for k in ref.KEYS:
            assert (f"{name}_{k}" in g) == (k in keys), (name, k)
        for k in keys:
            v = g[f"{name}_{k}"]
            assert v.shape == shapes[k] and v.dtype == np.float32 and np.isfinite(v).all() and np.abs(v).max() > 0
    B, neg = ref.SFRS_SHAPE["B"], ref.SFRS_SHAPE["neg_num"]
    for name, (loss_type, gen) in ref.SINGLE_SFRS.items():
        assert g[f"{name}_picks"].shape == (B, neg) and g[f"{name}_pick_gap"].shape == (B, neg)
        assert gen == 0 or g[f"{name}_pick_gap"].min() >= 1e-3
        # with the synthetic weights the reference picks the whole image for every negative (see the generator)
        assert not g[f"{name}_picks"].any()
        h = g[f"{name}_hinge"]
        assert h.shape == (B, neg) and (loss_type != "triplet" or (np.abs(h).min() >= 1e-3 and (h > 0).any()))
    # a frozen backbone does not change the loss, and generation 1 with region 0 picked changes the soft loss only
    assert np.array_equal(g["trainer_sare_joint_losses"], g["trainer_sare_joint_frozen_losses"])
    for lt in ("triplet", "sare_ind", "sare_joint"):
        l0, l1 = g[f"sfrs_{lt}_g0_losses"], g[f"sfrs_{lt}_g1_losses"]
        assert abs(l0[0] - l1[0]) <= 1e-12 * l0[0] and abs(l0[1] - l1[1]) > 0.1   # (one call | a sum over the tuples)
    assert set(ref.TRAJ) == {"traj_sfrs"}
    for name, (_, loss_type, gen) in ref.TRAJ.items():
        assert int(g[f"{name}_iters"]) == ref.ITERS and float(g[f"{name}_lr"]) in ref.LRS
        l64, l32, stale = g[f"{name}_losses"], g[f"{name}_losses32"], g[f"{name}_stale"]
        assert l64.shape == l32.shape == stale.shape == (ref.ITERS, 2) and np.array_equal(l64[0], stale[0])
        assert g[f"{name}_loss_ref_err"].shape == (ref.ITERS, 2) and g[f"{name}_loss_ref_err"].max() <= REF_ERR_MAX
        tot = lambda l: l[:, 0] + ref.LAMBDA_SOFT * l[:, 1]
        bars = np.maximum(1e-5, 8.0 * np.abs(tot(l32) - tot(l64)) / tot(l64))
        ratio = np.abs(tot(l64) - tot(stale)) / (bars * tot(l64))
        print(name, "lr", float(g[f"{name}_lr"]), "sensitivity", ratio[1:])
        assert np.allclose(ratio, g[f"{name}_sensitivity"], rtol=1e-9) and ratio[1:].min() >= 100.0
        assert g[f"{name}_picks"].shape == (ref.ITERS, B, neg) and not g[f"{name}_picks"].any()
        assert g[f"{name}_pick_gap"].min() >= 1e-3
        h = g[f"{name}_hinge"]
        assert h.shape == (ref.ITERS, B, neg) and np.abs(h).min() >= 1e-3 and (h > 0).any(-1).any(-1).all()


@pytest.mark.parametrize("name", list(ref.SINGLE_TRAINER))
def test_trainer_losses_from_the_oracle(golden, maps, state_dict, name):
    loss_type, _ = ref.SINGLE_TRAINER[name]
    got = ref.trainer_loss64(maps["trainer"], state_dict, ref.TRAINER_SHAPE["B"], ref.TRAINER_SHAPE["n"], loss_type)
    want = float(golden[f"{name}_losses"][0])
    print(f"{name}: {got:.15f} from the oracle, the reference's {want:.15f}, {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-9 * want


@pytest.mark.parametrize("name", list(ref.SINGLE_SFRS))
def test_sfrs_losses_from_the_oracle(golden, maps, state_dict, name):
    loss_type, gen = ref.SINGLE_SFRS[name]
    hard, soft, picks, gaps = ref.sfrs_losses64(maps["easy"], maps["diff"], state_dict, ref.SFRS_SHAPE["B"], loss_type, gen)
    want = golden[f"{name}_losses"]
    print(f"{name}: loss_hard {hard:.15f} ({want[0]:.15f}), loss_soft {soft:.15f} ({want[1]:.15f}); "
          f"errors {abs(hard - want[0]) / want[0]:.2e} {abs(soft - want[1]) / want[1]:.2e}")
    assert abs(hard - want[0]) <= 1e-9 * want[0] and abs(soft - want[1]) <= 1e-9 * want[1]
    assert np.array_equal(picks, golden[f"{name}_picks"])
    assert np.allclose(gaps, golden[f"{name}_pick_gap"], rtol=0, atol=1e-9)
