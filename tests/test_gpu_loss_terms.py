"""-m gpu: the train step's loss code, one path at a time, against the oracle in fp64.

  * `photometric_loss: gaussian_nll` ON ITS NLL BRANCH (mean colour NLL <= 2, losses.py:30-36): every earlier gaussian_nll case
    of the suite sits on the L1 side of that switch, where no gradient flows through the rendered colour variances
    (tests/test_loss_terms_cpu.py asserts both).  Inputs: gpu_common.nll_branch_targets;
  * the same with the photometric term alone, and on either side of the switch (mean NLL ~1 and ~3: a normaliser wrong by the
    factor 3 flips one of the two);
  * render_ijs under autograd with a loss that reads ONE output (colour variances, depth variance, rgbd, termination
    probability, free-space / TSDF vector);
  * the default losses with ONE term's weight non-zero, Fourier and hash network, with and without the fused compositing
    backward.

Gradients are compared FIELD BY FIELD (gpu_common.grad_close_per_field: the error of a field's slice over that field's own
max |grad|; a field without gradient in the reference must be exactly zero here) at the project's bars: 2e-3 (Fourier), 5e-3
(the NLL-mode step, test_nll_loss_modes_ragged_vs_oracle's), gpu_common.HASH_BARS (hash).  The problems and their references
are built once (tests/_loss_terms.py) and checked for conditioning on the CPU (tests/test_loss_terms_cpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _loss_terms as LT  # noqa: E402
from gpu_common import DEV, close, grad_close_per_field, hash_grad_close, make_renderer, make_target  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402

NLL_BAR, FOURIER_BAR = 5e-3, 2e-3
NLL_MODES = [("gaussian_nll", "huber"), ("gaussian_nll", "gaussian_nll")]
_id = lambda a: "-".join(str(x) for x in a) if isinstance(a, tuple) else str(a)


def _renderer(c):
    r = make_renderer(c["fkw"], c["ckw"], c["F"], c["params"])
    r.set_field_poses(c["pos"].to(DEV), c["quat"].to(DEV))
    return r


def _step(c):
    r = _renderer(c)
    return r.optimization_iteration(make_target(c["t"], torch.arange(c["F"])), c["u_c"].to(DEV), c["u_g"].to(DEV), update=False)


def _compare_prediction(res, c):
    p, ref = res["prediction"], c["pred"]
    close(p.rgbds, ref["rgbds"])
    close(p.term_probs, ref["term_probs"])
    close(p.color_vars, ref["color_vars"], rtol=1e-3, atol=1e-6)
    close(p.depth_vars, ref["depth_vars"], rtol=1e-3, atol=1e-6)


def _compare_grads(res, c, tol):
    for k, ref in c["grads"].items():
        grad_close_per_field(res["grads"][k], ref, tol, k)


def _l1_value(c):
    m = c["t"]["depth_mask"] & (c["pred"]["term_probs"] > 0.8)
    return float((c["pred"]["rgbds"][m][:, :3] - c["t"]["rgbds"][m][:, :3]).abs().double().mean())


# ------------------------------------------------------------------------------------------------ 1. colour NLL, fused step
@pytest.mark.parametrize("geom", ["nrgbd", "occupancy"])
@pytest.mark.parametrize("photo,depth", NLL_MODES)
@pytest.mark.parametrize("shape", LT.NLL_SHAPES, ids=_id)
def test_colour_nll_branch_fused_step_vs_oracle(shape, photo, depth, geom):
    """k_stash_bwd's NLL seeds (dC = k e / v, gV = k / 2 (1 / v - e^2 / v^2)), the 2 gV (c_k - C) colour term and the
    (q - mC)^2 weight term with non-zero colour-variance seeds, and the NLL value of the photometric term"""
    c = LT.nll_case(shape, photo, depth, geom, "full")
    res = _step(c)
    _compare_prediction(res, c)
    pk = "photometric_" + photo
    assert float(c["loss"][pk]) < 0 and abs(float(c["loss"][pk]) - _l1_value(c)) > 1.0          # the NLL value is not the L1 value
    for k in (pk, "depth_" + depth, "combined"):
        print(k, float(res[k]), float(c["loss"][k]))
        close(res[k], c["loss"][k], rtol=2e-3, atol=1e-5)
    for k in ("termination", "freespace", "tsdf"):
        close(res[k], c["loss"][k], rtol=3e-4, atol=1e-6)
    _compare_grads(res, c, NLL_BAR)


# ------------------------------------------------------------------------------------------------ 2. the photometric term alone
@pytest.mark.parametrize("geom", ["nrgbd", "occupancy"])
@pytest.mark.parametrize("shape", LT.NLL_SHAPES, ids=_id)
def test_colour_nll_branch_photometric_term_alone_vs_oracle(shape, geom):
    """every other weight is zero: nothing masks the colour-variance path.  (2, 130, 20, 4), nrgbd: field 0 has no selected ray,
    its gradient is exactly zero in the reference and must be here"""
    c = LT.nll_case(shape, "gaussian_nll", "huber", geom, "photo_only")
    res = _step(c)
    _compare_prediction(res, c)
    for k in ("photometric_gaussian_nll", "combined"):
        close(res[k], c["loss"][k], rtol=2e-3, atol=1e-5)
    _compare_grads(res, c, NLL_BAR)


# ------------------------------------------------------------------------------------------------ 3. the threshold
@pytest.mark.parametrize("variant", ["thr_nll", "thr_l1"])
@pytest.mark.parametrize("shape", LT.NLL_SHAPES, ids=_id)
def test_colour_nll_switch_either_side_vs_oracle(shape, variant):
    """mean colour NLL 1.0 (-> the NLL value and NLL gradients) and 3.0 (-> the L1 value and L1 gradients): photo_nll_uses_l1
    and loss_values_from_sums on the device, with the mean taken over the 3 n colour elements"""
    c = LT.nll_case(shape, "gaussian_nll", "huber", "nrgbd", variant)
    res = _step(c)
    want = _l1_value(c) if variant == "thr_l1" else c["mean_nll"]
    assert abs(c["mean_nll"] - (3.0 if variant == "thr_l1" else 1.0)) < 0.5 and abs(c["mean_nll"] - _l1_value(c)) > 0.4
    assert float(c["loss"]["photometric_gaussian_nll"]) == pytest.approx(want, rel=1e-4)
    for k in ("photometric_gaussian_nll", "depth_huber", "combined"):
        print(k, float(res[k]), float(c["loss"][k]))
        close(res[k], c["loss"][k], rtol=2e-3, atol=1e-5)
    _compare_grads(res, c, NLL_BAR)


# ------------------------------------------------------------------------------------------------ 4. the seeded path
@pytest.mark.parametrize("shape,output", LT.SEEDED_CASES, ids=_id)
def test_render_ijs_autograd_one_output_at_a_time_vs_oracle(shape, output):
    """render_ijs(use_vmap=True) -> sum(output * cotangent) -> backward: ngm_render_bwd_seeded_vars with a non-zero
    d_color_vars / d_depth_vars and nothing else, ngm_render_bwd_seeded with one of its seeds alone"""
    c = LT.seeded_case(shape, output)
    r = _renderer(c)
    ids = torch.arange(c["F"], device=DEV)
    tgt = make_target(c["t"], ids)
    pred = r.render_ijs(tgt.ijs, tgt.c2ws, None, field_ids=ids, use_vmap=True, near_distances=tgt.near_distances,
                        far_distances=tgt.far_distances, gt_distances=tgt.gt_distances, u_coarse=c["u_c"].to(DEV),
                        u_guided=c["u_g"].to(DEV))
    out = getattr(pred, output)
    assert out.shape == c["cot"].shape
    (out * c["cot"].to(DEV)).sum().backward()
    vp = r._model.vmap_fields_params
    for k, ref in c["grads"].items():
        grad_close_per_field(vp[k].grad, ref, FOURIER_BAR, k)


# ------------------------------------------------------------------------------------------------ 5. one loss term at a time
@pytest.mark.parametrize("fused", [True, False], ids=["fused_comp", "stash_bwd"])
@pytest.mark.parametrize("term", list(LT.TERMS))
@pytest.mark.parametrize("net", ["fourier", "hash"])
def test_default_losses_one_term_at_a_time_vs_oracle(net, term, fused):
    """weights 50 : 40 : 1 : 1 : 0.3 hide a term that carries a few per cent (termination: 0.2-0.4 %) of the combined gradient
    behind the 2e-3 bar; here each term is the whole loss.  Both compositing backwards (inside the MLP backward, and
    k_stash_bwd).  A zero-weight term is reported as 0 by design, so only `combined` and the active term are compared."""
    c = LT.term_case(net, term)
    key = LT.TERMS[term][2]
    L = K.lib()
    old = L.ngm_debug_disable_fused_comp(0 if fused else 1)
    try:
        res = _step(c)
        used = L.ngm_debug_last_comp_fused()
    finally:
        L.ngm_debug_disable_fused_comp(old)
    assert used == (1 if fused else 0), used       # (both networks' stash kernels take the fused problem at any batch size)
    ft = dict(rtol=2e-3, atol=2e-4) if net == "hash" else {}
    close(res["prediction"].rgbds, c["pred"]["rgbds"], **ft)
    close(res["prediction"].term_probs, c["pred"]["term_probs"], **ft)
    lt = dict(rtol=2e-3, atol=1e-5) if net == "hash" else dict(rtol=3e-4, atol=1e-6)
    print(key, float(res[key]), float(c["loss"][key]), "combined", float(res["combined"]), float(c["loss"]["combined"]))
    close(res[key], c["loss"][key], **lt)
    close(res["combined"], c["loss"]["combined"], **lt)
    for k, ref in c["grads"].items():
        if net == "fourier":
            grad_close_per_field(res["grads"][k], ref, FOURIER_BAR, k)
            continue
        g = res["grads"][k].cpu()
        for f in range(ref.shape[0]):
            if float(ref[f].abs().max()) == 0.0:
                assert float(g[f].abs().max()) == 0.0, (k, f)
            else:
                hash_grad_close(g[f:f + 1], ref[f:f + 1], k)
