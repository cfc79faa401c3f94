"""The inputs of the loss-term tests, checked on the CPU with the fp64 oracle (no GPU): which branch of the photometric
gaussian_nll's switch (losses.py:34-35) every fixture and every generated case takes, that the NLL-branch cases are well
conditioned and do send a sizeable share of every gradient through the rendered colour variances, that the fp32 oracle alone
stays within a quarter of the bars test_gpu_loss_terms.py holds the kernels to (per-field normalisation), and the host's
loss_values_from_sums on both sides of the switch."""
import pytest
import torch

import _loss_terms as LT
from conftest import load_golden, split_prefix
from gpu_common import HASH_BARS, lattice_level_errors
from neural_graph_mapping_amd import distributed as D
from oracle import ngm_oracle as O
from test_oracle_golden import CASES

NLL_BAR, FOURIER_BAR = 5e-3, 2e-3                # the bars of the GPU tests (NLL-mode step, Fourier network)
NLL_MODES = [("gaussian_nll", "huber"), ("gaussian_nll", "gaussian_nll")]
NLL_BRANCH = [(s, p, d, g, v) for s in LT.NLL_SHAPES for p, d in NLL_MODES for g in ("nrgbd", "occupancy") for v in ("full", "photo_only")]
THRESHOLD = [(s, "gaussian_nll", "huber", "nrgbd", v) for s in LT.NLL_SHAPES for v in ("thr_nll", "thr_l1")]
_id = lambda a: "-".join(str(x) for x in a) if isinstance(a, tuple) else str(a)


def per_field_errors(a, b):
    """worst |a - b| of field f's slice over that field's max |b| -> list of F floats (0 where the reference slice is zero and
    `a` is too, inf where only the reference is)"""
    out = []
    for f in range(b.shape[0]):
        scale, err = float(b[f].abs().max()), float((a[f] - b[f]).abs().max())
        out.append(err / scale if scale > 0 else (0.0 if err == 0 else float("inf")))
    return out


def _fixture_run(name, detach_color_vars=False):
    """the oracle in fp64 on a train-step fixture -> (fixture, its targets, prediction, losses, gradients)"""
    g = load_golden(name)
    fs, rs = O.FieldSpec(**CASES[name]["fs"]), O.RenderSpec(**CASES[name]["rs"])
    c = dict(t=split_prefix(g, "t::"), rs=rs, fs=fs, pos=g["pos"], quat=g["quat"], u_c=g["u_coarse"], u_g=g["u_guided"],
             params={k: v for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"})
    return (g, c["t"]) + LT.oracle_run(c, detach_color_vars=detach_color_vars)


# ------------------------------------------------------------------------------------------------ which branch
@pytest.mark.parametrize("name,branch", [("g20_train_gnll_gnll", "l1"), ("g20_train_l1_lnll", "l1"), ("g20_train_gnll_switch_l1", "l1"),
                                         ("g28_train_gnll_nll_branch", "nll")])
def test_fixture_branch(name, branch):
    """from the fixture's own RECORDED prediction: the mean colour NLL is far from the switch at 2, and the recorded photometric
    loss is the L1 value (all three G20 fixtures) or the NLL value (G28)"""
    g = load_golden(name)
    t = split_prefix(g, "t::")
    rec = dict(rgbds=g["pred_rgbds"], color_vars=g["pred_color_vars"], term_probs=g["pred_term_probs"])
    mean, n = LT.mean_color_nll(rec, t)
    print(f"{name}: mean colour NLL {mean:.6g} over {n} rays")
    assert n > 0 and not 1.0 <= mean <= 4.0, mean
    assert (mean > 2) == (branch == "l1")
    m = t["depth_mask"] & (g["pred_term_probs"] > 0.8)
    l1 = float((g["pred_rgbds"][m][:, :3] - t["rgbds"][m][:, :3]).abs().double().mean())
    pk = [k for k in g if k.startswith("loss::photometric_")]
    assert len(pk) == 1
    if pk[0] == "loss::photometric_gaussian_nll":
        assert float(g[pk[0]]) == pytest.approx(l1 if branch == "l1" else mean, rel=1e-5)
    # the oracle in fp64 takes the same branch
    _, _, pred, loss, _ = _fixture_run(name)
    mean64, _ = LT.mean_color_nll({k: v.detach() for k, v in pred.items() if v is not None}, t)
    assert (mean64 > 2) == (branch == "l1") and not 1.0 <= mean64 <= 4.0


def test_g20_fixtures_send_nothing_through_the_colour_variances_but_g28_does():
    """the oracle's gradients with the colour variances detached: unchanged, bit for bit, on the G20 fixtures (L1 branch) --
    and changed by more than 10 % of every tensor's scale on G28"""
    for name in ("g20_train_gnll_gnll", "g20_train_gnll_switch_l1"):
        full, cut = _fixture_run(name)[4], _fixture_run(name, detach_color_vars=True)[4]
        assert all(torch.equal(full[k], cut[k]) for k in full), name
    g, t, pred, _, full = _fixture_run("g28_train_gnll_nll_branch")
    cut = _fixture_run("g28_train_gnll_nll_branch", detach_color_vars=True)[4]
    share = {k: float((full[k] - cut[k]).abs().max() / full[k].abs().max()) for k in full}
    print("g28 colour-variance share", {k: round(v, 3) for k, v in share.items()})
    assert min(share.values()) >= 0.10, share
    assert int((t["depth_mask"] & (pred["term_probs"] > 0.8)).sum()) >= 16


@pytest.mark.parametrize("key", NLL_BRANCH + THRESHOLD, ids=_id)
def test_generated_case_branch(key):
    c = LT.nll_case(*key)
    variant = key[-1]
    print(f"{key}: scale {c['scale']:.4f} mean colour NLL {c['mean_nll']:.4f} over {c['n_sel']} rays")
    if variant == "thr_nll":
        assert 0.5 <= c["mean_nll"] <= 1.5
    elif variant == "thr_l1":
        assert 2.5 <= c["mean_nll"] <= 3.5
    else:
        assert c["mean_nll"] < 1.0
    # the value of the term is the one of the branch taken
    t, p = c["t"], c["pred"]
    m = t["depth_mask"] & (p["term_probs"] > 0.8)
    l1 = float((p["rgbds"][m][:, :3] - t["rgbds"][m][:, :3]).abs().double().mean())
    want = l1 if variant == "thr_l1" else c["mean_nll"]
    assert float(c["loss"]["photometric_gaussian_nll"]) == pytest.approx(want, rel=1e-4, abs=1e-6)
    # a normaliser wrong by the factor 3 (sum / n, sum / 9 n) would flip one of the two threshold cases
    if variant == "thr_nll":
        assert 3.0 * c["mean_nll"] > 2.0
    if variant == "thr_l1":
        assert c["mean_nll"] / 3.0 < 2.0


# ------------------------------------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("key", NLL_BRANCH + [k for k in THRESHOLD if k[-1] == "thr_nll"], ids=_id)
def test_nll_branch_case_is_well_conditioned(key):
    c = LT.nll_case(*key)
    assert c["n_sel"] >= 16, c["n_sel"]
    assert c["neutralised"] <= 0.15
    _, _, cut = LT.oracle_run(c, detach_color_vars=True)
    share = {k: float((c["grads64"][k] - cut[k]).abs().max() / c["grads64"][k].abs().max()) for k in cut}
    _, _, g32 = LT.oracle_run(c, torch.float32)
    err = {k: max(per_field_errors(g32[k].double(), c["grads64"][k])) for k in g32}
    print(f"{key}: colour-variance share {min(share.values()):.3f}..{max(share.values()):.3f}, fp32 oracle per field {max(err.values()):.2e}")
    assert min(share.values()) >= 0.10, share
    assert max(err.values()) <= NLL_BAR / 4, err


def test_photo_only_case_has_a_field_without_selected_rays():
    """(2, 130, 20, 4), nrgbd: field 0 has no selected ray, so with the photometric term alone its gradient is exactly zero in
    the reference -- the GPU test's exact-zero rule is exercised"""
    c = LT.nll_case((2, 130, 20, 4), variant="photo_only")
    m = c["t"]["depth_mask"] & (c["pred"]["term_probs"] > 0.8)
    assert m.sum(-1).tolist()[0] == 0 and m.sum(-1).tolist()[1] >= 16
    for k, v in c["grads64"].items():
        assert float(v[0].abs().max()) == 0.0 and float(v[1].abs().max()) > 0.0, k


@pytest.mark.parametrize("term", list(LT.TERMS))
@pytest.mark.parametrize("net", ["fourier", "hash"])
def test_single_term_case_is_well_conditioned(net, term):
    """the default losses one term at a time: only that term is in `combined`, and the fp32 oracle alone stays within a quarter
    of the GPU test's bar at the per-field normalisation -- Fourier network.  The hash network has no such margin to give: its
    bars (gpu_common.HASH_BARS) are twice the fp32 floor the whole suite measured, and that floor does not fall with the number
    of rays (a fine level's feature is uncertain by 5e-3 of its scale in ANY fp32 evaluation, and so is its column of the first
    layer's weight gradient).  Its cases are held to the necessary condition -- the fp32 oracle itself passes the bars, per
    field and per level -- and the figures are printed (measured: first weight 0.7-1.8e-3 of 4e-3, coarse levels up to 3.3e-3
    of 6e-3, everything else within a quarter)."""
    c = LT.term_case(net, term)
    key = LT.TERMS[term][2]
    wk = LT.TERMS[term][0]
    assert float(c["loss"]["combined"]) == pytest.approx(LT.WEIGHTS[wk] * float(c["loss"][key]), rel=1e-6) and float(c["loss"][key]) > 0
    assert c["neutralised"] <= 0.15
    _, _, g32 = LT.oracle_run(c, torch.float32)
    frac = 0.25 if net == "fourier" else 1.0
    for k, ref in c["grads64"].items():
        errs = per_field_errors(g32[k].double(), ref)
        if net == "fourier":
            bar = FOURIER_BAR
        elif k == "_encoding.lattice_values":
            bar = HASH_BARS["lattice"]
            for f in range(ref.shape[0]):
                lv = lattice_level_errors(g32[k][f:f + 1].double(), ref[f:f + 1])
                print(f"{net} {term} field {f} lattice levels: coarse {max(lv[:5]):.2e} fine {max(lv[5:]):.2e}")
                assert max(lv[:5]) < frac * HASH_BARS["lattice_coarse_level"] and max(lv[5:]) < frac * HASH_BARS["lattice_fine_level"], (f, lv)
        else:
            bar = HASH_BARS["first_weight"] if k == "_linears.0.weight" else HASH_BARS["other"]
        print(f"{net} {term} {k}: fp32 oracle per field {max(errs):.2e} (bar {bar:.0e})")
        assert max(errs) < frac * bar, (k, errs)
    if term == "depth_huber":
        t, p = c["t"], c["pred"]
        m = t["depth_mask"] & (p["term_probs"] > 0.8)
        e = (p["rgbds"][m][:, 3] - t["rgbds"][m][:, 3]).abs()
        assert int(m.sum()) >= 16
        assert float((e < 0.05).float().mean()) >= 0.25 and float((e > 0.05).float().mean()) >= 0.25
        assert float((e - 0.05).abs().min()) > 1e-4


@pytest.mark.parametrize("shape,output", LT.SEEDED_CASES, ids=_id)
def test_seeded_case_is_well_conditioned(shape, output):
    """one output at a time under autograd: every tensor has a gradient, and the fp32 oracle is within a quarter of the bar"""
    c = LT.seeded_case(shape, output)
    g32 = LT.seeded_oracle(c, torch.float32)
    err = {k: max(per_field_errors(g32[k].double(), ref)) for k, ref in c["grads64"].items()}
    print(f"{shape} {output}: fp32 oracle per field {max(err.values()):.2e}")
    assert max(err.values()) <= FOURIER_BAR / 4, err
    assert all(float(v.abs().max()) > 0 for v in c["grads64"].values())


# ------------------------------------------------------------------------------------------------ the host's loss values
def _sums(photo_sum, n, l1_sum):
    s = torch.zeros(16, dtype=torch.float64)
    s[0], s[1], s[10] = photo_sum, n, l1_sum
    s[2], s[3] = 0.5, n                     # depth
    s[4], s[5], s[6], s[7], s[8], s[9] = 2.0, 10, 3.0, 20, 0.25, 5
    return s


@pytest.mark.parametrize("mean,branch", [(-3.5, "nll"), (1.0, "nll"), (1.999, "nll"), (2.001, "l1"), (3.0, "l1"), (9.6e3, "l1")])
def test_host_loss_values_from_sums_on_both_sides_of_the_switch(mean, branch):
    """distributed.loss_values_from_sums (the multi-GPU path's restatement of the device function): the NLL value up to a
    mean of 2, the L1 value beyond; the mean is the sum over the 3 n colour elements.  A sum of 3 n is a mean of 1.0 (3.0 when
    divided by n: the wrong side), a sum of 9 n a mean of 3.0 (1.0 when divided by 9 n)."""
    n, l1_sum = 7, 4.2
    s = _sums(mean * 3 * n, n, l1_sum)
    out = D.loss_values_from_sums(s, 0.3, 1.0, 1.0, 40.0, 50.0, photometric_loss="gaussian_nll", depth_loss="gaussian_nll")
    want = mean if branch == "nll" else l1_sum / (3 * n)
    assert float(out["photometric_gaussian_nll"]) == pytest.approx(want, rel=1e-12)
    rest = 0.3 * 0.25 / 5 + 0.5 / n + 40.0 * 2.0 / 10 + 50.0 * 3.0 / 20
    assert float(out["combined"]) == pytest.approx(want + rest, rel=1e-12)
    # the other photometric modes never switch
    out = D.loss_values_from_sums(s, 0.3, 1.0, 1.0, 40.0, 50.0, photometric_loss="l2")
    assert float(out["photometric_l2"]) == pytest.approx(mean, rel=1e-12)
    # an empty selection is NaN on either branch
    out = D.loss_values_from_sums(_sums(0.0, 0, 0.0), 0.3, 1.0, 1.0, 40.0, 50.0, photometric_loss="gaussian_nll")
    assert torch.isnan(out["photometric_gaussian_nll"]) and torch.isnan(out["combined"])
