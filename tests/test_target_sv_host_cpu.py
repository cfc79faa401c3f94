"""The numpy mirror of the device single-view sampler (tests/_target_sv_host.py) held to the pinned oracle, the margins of
the GPU scenes, and the comparison the GPU test makes shown to catch planted one-line faults.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _target_sv_host as SV  # noqa: E402
import scene  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402


@pytest.mark.parametrize("name", list(SV.CASES))
def test_mirror_draws_through_the_oracle(name):
    """the mirror's own draws, in the oracle's index conventions, give the mirror's field ids, ijs and masks exactly and its
    floats within the 2e-6 of the G16 comparison: the mirror is the pinned restatement + another random stream"""
    c = SV.CASES[name]
    s, m = SV.run_case(name)
    d = {k: torch.from_numpy(v) for k, v in SV.oracle_draws(m, s["img"][..., 3]).items()}
    act = np.array(c["active"])
    act = act[(act >= 0) & (act < len(s["positions"]))]                  # the oracle has no skipped entries
    cam = O.CameraSpec(scene.SV_W, scene.SV_H, scene.SV_FX, scene.SV_FY, scene.SV_CX, scene.SV_CY)
    t, _ = O.sample_target_sv(cam, torch.from_numpy(s["img"]), torch.from_numpy(s["c2w"]), torch.from_numpy(s["positions"]),
                              torch.from_numpy(act), c["T"], c["R"], s["radius"], draws=d)
    n = m["count"]
    assert n == len(t["field_ids"]) > 0
    assert np.array_equal(t["field_ids"].numpy(), m["field_ids"][:n])
    assert np.array_equal(t["ijs"].numpy(), m["ijs"][:n])
    for k in ("rgb_mask", "depth_mask", "term_mask"):
        assert np.array_equal(t[k].numpy(), m[k][:n]), k
    for k in ("near", "far", "gt", "rgbds", "term_probs"):
        assert np.allclose(t[k].numpy(), m[k][:n], rtol=2e-6, atol=2e-6), k


@pytest.mark.parametrize("name", list(SV.CASES))
def test_scene_margins_and_branches(name):
    """every decision of the GPU scenes is further than MARGIN from its boundary in float64, and float32 decides alike"""
    _, m64 = SV.run_case(name, dt=np.float64)
    _, m32 = SV.run_case(name)
    assert min(m64["margins"]) > SV.MARGIN, m64["margins"]
    for k in SV.EXACT:
        assert np.array_equal(np.asarray(m64[k]), np.asarray(m32[k])), k
    T = SV.CASES[name]["T"]
    assert (m32["num_candidates"] <= T) == (name in ("all_pixels", "boundary"))    # both branches of the field draw are covered
    if name == "all_pixels":
        assert m32["num_used"] == int((SV.g16_scene()["img"][..., 3] != 0).sum()) < 65536


def test_boundary_scene_holds_hits_R_next_to_R_minus_1():
    """one call, one candidate list: the field with hits == R is a candidate and gets a row, the one with hits == R - 1 does not"""
    c = SV.CASES["boundary"]
    _, m = SV.run_case("boundary")
    act = list(c["active"])
    assert m["hits"][act.index(SV.BOUNDARY_IN)] == c["R"] and m["hits"][act.index(SV.BOUNDARY_OUT)] == c["R"] - 1
    ids = list(m["field_ids"][:m["count"]])
    assert SV.BOUNDARY_IN in ids and SV.BOUNDARY_OUT not in ids
    assert m["num_candidates"] == int((m["hits"] >= c["R"]).sum()) == m["count"]


def boundary_R(name="p2000"):
    """R = the hit count of one candidate of the scene, so that a field with hits == R exists there"""
    _, m = SV.run_case(name)
    return int(np.sort(m["hits"][m["hits"] > 0])[1])


def _pair(fault, **kw):
    c = SV.CASES["p2000"]
    s = SV.g16_scene()
    args = dict(num_points=c["num_points"], T=c["T"], R=c["R"], seed=c["seed"], iteration=0)
    args.update(kw)
    run = lambda f: SV.sample(s["img"], s["c2w"], s["positions"], np.array(c["active"]), s["radius"], s["intrinsics"], fault=f, **args)
    return run(fault), run(None)


def _gt_on_far():
    """5 x 5 frame at depth 2.5, principal point on pixel (2, 2), one field at (0, 0, -2) of radius 0.5: far == gt == 2.5 on
    the central ray, all in exactly representable numbers"""
    img = np.zeros((5, 5, 4), np.float32)
    img[..., 3] = 2.5
    args = (img, np.eye(4, dtype=np.float32), np.array([[0.0, 0.0, -2.0]], np.float32), np.array([0]), 0.5, (4.0, 4.0, 2.0, 2.0), 25, 1)
    R = int(SV.sample(*args, 1, 0, 0)["hits"][0])
    return lambda f: SV.sample(*args, R, 0, 0, fault=f)


@pytest.mark.parametrize("fault,named", [("hits_gt", "num_candidates"), ("sorted_when_few", "subset_fields"),
                                         ("ray_key_no_field", "segments"), ("ray_order_by_pixel", "segments"),
                                         ("gt_le_far", "rgb_mask"), ("padding_zero", "padding")])
def test_planted_faults_break_the_comparison(fault, named):
    if fault == "hits_gt":
        bad, good = _pair(fault, R=boundary_R())
    elif fault == "sorted_when_few":
        bad, good = _pair(fault, T=12)                                   # all candidates are taken: active order
    elif fault == "gt_le_far":
        run = _gt_on_far()
        bad, good = run(fault), run(None)
    elif fault == "padding_zero":
        bad, good = _pair(fault, capacity=6)
    else:
        bad, good = _pair(fault)
    SV.compare(good, good)
    with pytest.raises(AssertionError, match="^" + named + ":"):
        SV.compare(bad, good)
