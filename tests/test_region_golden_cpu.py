"""The fp64 comparator of the SFRS region head (tests/helpers/region_ref.py) against vectors the REFERENCE ITSELF
produced with EmbedRegionNet in training mode (tests/golden/region_*.npz, written by
tests/helpers/make_region_golden.py).  CPU only.  The GPU tests use the same comparator at sizes without a fixture."""
import pytest
import torch

from conftest import assert_rel_l2, load_golden, report
from helpers import region_ref
from openibl_amd import synth
from oracle import descriptor as od

TOL = 2e-6        # the bound between oracle and reference (tests/test_oracle_golden.py)


@pytest.mark.parametrize("name", ["region_small", "region_480x640"])
def test_region_comparator_matches_reference(name, state_dict):
    g = load_golden(name)
    n, _, h, w = [int(v) for v in g["shape"]]
    assert int(g["tuple_size"]) == 1
    x = synth.images(n, h, w, seed=int(g["image_seed"]))
    with torch.no_grad():
        feat = od.vgg16_conv5(x, state_dict)          # fp32 like the reference's backbone; the head below is fp64
        vec = region_ref.region_vectors(feat, state_dict["net_vlad.conv.weight"], state_dict["net_vlad.centroids"])
        score = region_ref.region_scores(vec, 1)
    s = int(g["vlad_stride"])
    assert tuple(score.shape) == tuple(g["score"].shape) == (1, n - 1, 9, 9)
    assert tuple(g["vlad_A"].shape) == (1, 1, 9, 32768 // s) and tuple(g["vlad_B"].shape) == (1, n - 1, 9, 32768 // s)
    want = torch.cat([torch.from_numpy(g["vlad_A"])[0], torch.from_numpy(g["vlad_B"])[0]], dim=0)   # [n][9][L / s]
    got = vec[..., ::s]
    for i in range(n):
        for r in range(9):
            assert_rel_l2(f"{name} image {i} region {r}", got[i, r], want[i, r], TOL)
    report(f"{name} score", score, g["score"])
    assert float((score - torch.from_numpy(g["score"]).double()).abs().max()) <= TOL
    # region 0 is the whole image: the four quarters add up to the image's raw VLAD
    whole = od.normalize_vlad(od.netvlad(feat.double(), state_dict["net_vlad.conv.weight"].double(),
                                         state_dict["net_vlad.centroids"].double()))
    assert_rel_l2(f"{name} region 0 against the whole-image VLAD", vec[:, 0], whole, 1e-12)


def test_odd_map_side_is_rejected(state_dict):
    """A 70 x 90 image has a 4 x 5 map: the reference's view() raises, the comparator says why."""
    x = synth.images(2, 70, 90, seed=13)
    with torch.no_grad():
        feat = od.vgg16_conv5(x, state_dict)
    assert tuple(feat.shape[2:]) == (4, 5)
    with pytest.raises(ValueError, match="4 x 5"):
        region_ref.region_vectors(feat, state_dict["net_vlad.conv.weight"], state_dict["net_vlad.centroids"])
