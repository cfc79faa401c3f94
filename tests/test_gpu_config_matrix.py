"""Every accepted field configuration on every surface: oracle match by the kernel the table names, or a clean refusal.

The table is tests/_config_matrix.py (about 40 explicit entries: depth 1-4, one-16-tile and mixed widths, hash ladders of 1-16
levels, skip connections, the explicit bf16x3 mode outside its shape).  For each (entry, surface, mode) exactly two outcomes
are admissible:

  it runs     the result meets the oracle at the suite's bars -- forward `close` 2e-4 / 2e-5 (2e-3 / 4e-4 through NeRF
              octaves; FWD_BARS for the default hash ladder), gradients 2e-3 of max |grad| through grad_close, HASH_BARS through
              hash_grad_close -- and the library reports the kernel the table names (ngm_debug_last_bwd_variant,
              ngm_debug_last_comp_fused, ngm_debug_last_matmul);
  it refuses  NgmError, code NGM_E_UNSUPPORTED, a message; no gradient has appeared, a refused update=True step leaves
              parameters, Adam moments, 16-bit copies and both step counters bit-identical; and the next call of the process, on
              a supported configuration, succeeds and matches the oracle (no sticky HIP error, no stale stash bookkeeping).

A refusal is a returned status: nothing here launches a kernel on a shape it was not compiled for."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _config_matrix as CM  # noqa: E402
from gpu_common import (DEV, KINK, _test_id, close, compare_losses, cu, grad_close, hash_grad_close, make_renderer, make_target,  # noqa: E402
                        matrix_is_hash, matrix_knn_case, matrix_points_case, matrix_step_case)
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402

# Forward bars.  Fourier / none / triplane: the suite's 2e-4 / 2e-5; NeRF octaves in the point evaluation: 2e-3 with
# atol = 0.2 rtol (test_field_eval_forward_backward_vs_oracle).  The references are the oracle in fp64.
# Hash ladders: the same oracle evaluated in fp32 against itself in fp64, on these very problems (CPU; the error any fp32
# evaluation of the encoding carries), and where that alone is past the suite's bar, 4 x that error as atol:
#   scales >= 0.1 (hash1 / hash4_T8 / hash8 / hash9_T8)   fp32 oracle error <= 4.7e-7 on a point, <= 3.5e-6 rendered: the suite's bar
#   default ladder, finest scale 1e-4 (hash16_L1 / _L2)     fp32 positions carry ~1e-7 and the finest level scales them by 1e4:
#       point evaluation 2.35e-4 -> 9.4e-4;  kNN blend 1.09e-4 -> 4.4e-4;  rendered rgbd 1.13e-3 -> 4.5e-3;
#       rendered termination probability 3.98e-4 -> 1.6e-3
#   (ten times the suite's atol before any kernel has run, so the suite's bar cannot be asked of an fp32 kernel here; the
#   suite's own hash tests use 1e-3 / 1e-4 on points and 2e-3 / 1e-3 rendered against the fp32 oracle.)
FWD_BARS = dict(default=dict(rtol=2e-4, atol=2e-5), nerf=dict(rtol=2e-3, atol=4e-4),
                hash_fine=dict(points=dict(rtol=2e-4, atol=9.4e-4),        # derived: 4 x fp32-vs-fp64 oracle (2.35e-4)
                               knn=dict(rtol=2e-4, atol=4.4e-4),           # derived: 4 x 1.09e-4
                               rgbds=dict(rtol=2e-4, atol=4.5e-3),         # derived: 4 x 1.13e-3
                               term_probs=dict(rtol=2e-4, atol=1.6e-3)))   # derived: 4 x 3.98e-4


def _fwd_bar(e, what):
    f = e["fkw"]
    if f["encoding"] == "permuto" and CM.hash_sigmas(e) is None:
        return FWD_BARS["hash_fine"][what]
    if f["encoding"] == "nerf" and what in ("points", "knn"):
        return FWD_BARS["nerf"]
    return FWD_BARS["default"]


def _grads_close(e, got, ref, surface):
    for k, g in ref.items():
        print(f"  {k}: {float((got[k].cpu() - g).abs().max() / g.abs().max().clamp_min(1e-12)):.3e}")
        derived = e["bars"].get(surface, {}).get(k)          # 4 x the fp32 oracle's own error, see the entry
        if derived is not None:
            grad_close(got[k], g, derived, k)
        elif matrix_is_hash(e):
            hash_grad_close(got[k], g, k, sigmas=CM.hash_sigmas(e))
        else:
            grad_close(got[k], g, 2e-3, k)


def _fwd_close(e, got, ref, what, label=""):
    bar = _fwd_bar(e, what)
    print(f"  {what} {label}: max abs err {float((got.cpu() - ref).abs().max()):.3e} (bar rtol {bar['rtol']:.0e} atol {bar['atol']:.1e})")
    close(got, ref, **bar)


def _refused(exc):
    assert exc.value.code == K.NGM_E_UNSUPPORTED, exc.value
    assert str(exc.value).split(":", 1)[-1].strip(), "a refusal carries a message"


L = K.lib


def _reported(which):
    return {K.MATMUL["f32"]: "f32", K.MATMUL["bf16x3"]: "bf16x3"}.get(L().ngm_debug_last_matmul(which))


def _renderer(e, c, mode, **extra):
    r = make_renderer({**e["fkw"], **extra}, {**c["ckw"], "mlp_matmul": mode}, c["F"], c["params"])
    if c["sd"] is not None:
        with torch.no_grad():
            r._model.all_fields_params["_neus_sd"].copy_(c["sd"].to(DEV))
    r.set_field_poses(c["pos"].to(DEV), c["quat"].to(DEV))
    return r


def _step_matches(e, c, mode, expect, r=None, ids=None):
    """one fused step with update=False against the oracle: prediction, every loss term, every gradient, the kernels that ran
    (r, ids: a renderer that holds the case's fields in the rows `ids` of a larger set, tests/test_gpu_storage_matrix.py)"""
    _, mm, variant, fused = expect
    KINK.extend(dict(k, test=_test_id()) for k in c["kink"])          # the margins report: rays taken out of this comparison
    r = _renderer(e, c, mode) if r is None else r
    ids = torch.arange(c["F"]) if ids is None else ids
    res = r.optimization_iteration(make_target(c["t"], ids), c["u_c"].to(DEV), c["u_g"].to(DEV), update=False)
    torch.cuda.synchronize()
    assert (_reported(0), L().ngm_debug_last_bwd_variant(), L().ngm_debug_last_comp_fused()) == (mm, variant, fused)
    _fwd_close(e, res["prediction"].rgbds, c["pred"]["rgbds"], "rgbds", mode)
    _fwd_close(e, res["prediction"].term_probs, c["pred"]["term_probs"], "term_probs", mode)
    hashed = matrix_is_hash(e)
    compare_losses(res, c["pred"], c["t"], c["rs"], rtol=2e-3 if hashed else 3e-4, atol=1e-5 if hashed else 1e-6)
    _grads_close(e, res["grads"], c["grads"], "step")


def _next_call_succeeds():
    """after a refusal: the suite's flagship network through the point evaluation (forward + stash backward) and one fused
    step, both against the oracle -- an error left behind by the refused call, or bookkeeping of a workspace that was never
    written, would show here"""
    e = CM.BY_NAME["fourier64_L2"]
    p = matrix_points_case(e, 257)
    fc = K.field_cfg(**e["fkw"], matmul_mode="auto")
    pg = {k: v.to(DEV).requires_grad_() for k, v in p["params"].items()}
    out = ops.field_eval(fc, pg, p["q"].to(DEV), p["pos"].to(DEV), p["quat"].to(DEV))
    close(out, p["out"])
    (out * p["d_out"].to(DEV)).sum().backward()
    assert L().ngm_debug_last_bwd_variant() == 3
    for k, g in p["grads"].items():
        assert float((pg[k].grad.cpu() - g).abs().max() / g.abs().max()) < 2e-3, k
    _step_matches(e, matrix_step_case(e, CM.STEP_SHAPES[1]), "auto", e["step"]["auto"])


# ------------------------------------------------------------------------------------------------ 1: point evaluation, forward
@pytest.mark.parametrize("name", CM.NAMES)
def test_points_forward(name):
    e = CM.BY_NAME[name]
    refused = False
    for mode, expect in e["points"].items():
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        for P in (1, 257):                        # 257 ends mid-tile for the 16- and the 32-sample kernels
            c = matrix_points_case(e, P)
            with torch.no_grad():
                if CM.runs(expect):
                    out = ops.field_eval(fc, cu(c["params"]), c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
                    assert _reported(1) == expect[1], (mode, P)
                    _fwd_close(e, out, c["out"], "points", f"{mode} P={P}")
                else:
                    with pytest.raises(K.NgmError) as exc:
                        ops.field_eval(fc, cu(c["params"]), c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
                    _refused(exc)
                    refused = True
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 2: point evaluation, autograd
@pytest.mark.parametrize("name", CM.NAMES)
def test_points_autograd(name):
    e = CM.BY_NAME[name]
    c = matrix_points_case(e, 257)
    refused = False
    for mode, expect in e["autograd"].items():
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        keep = ops.FIELD_EVAL_STASH_MAX_BYTES
        try:
            for i, stash_max in enumerate((keep, 0)):       # with the activation stash, then the recomputing backward
                ops.FIELD_EVAL_STASH_MAX_BYTES = stash_max
                pg = {k: v.to(DEV).requires_grad_(k not in K.NO_GRAD_PARAMS) for k, v in c["params"].items()}
                if CM.runs(expect):
                    out = ops.field_eval(fc, pg, c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
                    _fwd_close(e, out, c["out"], "points", f"{mode} stash_max={stash_max}")
                    (out * c["d_out"].to(DEV)).sum().backward()
                    assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                    _grads_close(e, {k: v.grad for k, v in pg.items()}, c["grads"], "autograd")
                else:
                    with pytest.raises(K.NgmError) as exc:
                        out = ops.field_eval(fc, pg, c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
                        (out * c["d_out"].to(DEV)).sum().backward()
                    _refused(exc)
                    refused = True
                    for k, v in pg.items():
                        assert v.grad is None or not bool(v.grad.any()), k
        finally:
            ops.FIELD_EVAL_STASH_MAX_BYTES = keep
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 3: fused training step
def _state(r):
    s = {"p::" + k: v.clone() for k, v in r._model.all_fields_params.items()}
    for k, st in r._optim_state.items():
        s["m::" + k], s["v::" + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    for k, v in (r._model.lp_fields_params or {}).items():
        s["lp::" + k] = v.clone()
    return s


@pytest.mark.parametrize("shape", CM.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", CM.NAMES)
def test_fused_step(name, shape):
    e = CM.BY_NAME[name]
    c = matrix_step_case(e, shape)
    refused = False
    for mode, expect in e["step"].items():
        if CM.runs(expect):
            _step_matches(e, c, mode, expect)
            continue
        refused = True
        tgt = make_target(c["t"], torch.arange(c["F"]))
        r = _renderer(e, c, mode)
        with pytest.raises(K.NgmError) as exc:
            r.optimization_iteration(tgt, c["u_c"].to(DEV), c["u_g"].to(DEV), update=False)
        _refused(exc)
        # update=True on 16-bit weight storage (not built for the triplane planes): nothing may move
        lp = {} if e["fkw"]["encoding"] == "triplane" else dict(weight_dtype="bfloat16")
        r = _renderer(e, c, mode, **lp)
        before, step0 = _state(r), r._step
        assert lp == {} or any(k.startswith("lp::") for k in before)
        with pytest.raises(K.NgmError) as exc:
            r.optimization_iteration(tgt, c["u_c"].to(DEV), c["u_g"].to(DEV), update=True)
        _refused(exc)
        torch.cuda.synchronize()
        after = _state(r)
        assert before.keys() == after.keys()
        for k, v in before.items():
            assert torch.equal(v, after[k]), k
        assert r._step == step0 and (r._step_dev is None or int(r._step_dev) == step0)
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 4: fused render forward
@pytest.mark.parametrize("shape", CM.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", CM.NAMES)
def test_fused_render_forward(name, shape):
    """ops.render_ijs_fused under no_grad -- the only fused surface a three-layer network has.  neus reads the per-field
    `_neus_sd`, which only the renderer's training forward passes to ngm_render_fwd: that entry goes through it."""
    from neural_graph_mapping_amd import renderer as Rr
    from gpu_common import NRGBD_KW
    e = CM.BY_NAME[name]
    c = matrix_step_case(e, shape)
    t, refused = cu(c["t"]), False
    cam = Rr.Camera(640, 480, NRGBD_KW["fx"], NRGBD_KW["fy"], 319.5, 239.5, pixel_center=0.0)
    rc = Rr.make_render_cfg(cam, Rr.shipped_config(**c["ckw"]), guided=True)
    for mode, expect in e["render"].items():
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)

        def render():
            if e["geometry"] == "neus":
                r = _renderer(e, c, mode)
                ctx = r._iteration_forward(make_target(c["t"], torch.arange(c["F"])), c["u_c"].to(DEV), c["u_g"].to(DEV),
                                           advance=False)
                return ctx["w"]["rgbds"], ctx["w"]["depth_vars"], ctx["w"]["term_probs"]
            with torch.no_grad():
                rgbds, _, dvars, term, _, _ = ops.render_ijs_fused(
                    fc, rc, cu(c["params"]), t["ijs"], t["c2ws"], t["near"], t["far"], t["gt"], c["pos"].to(DEV),
                    c["quat"].to(DEV), c["u_c"].to(DEV), c["u_g"].to(DEV))
            return rgbds, dvars, term
        if CM.runs(expect):
            rgbds, dvars, term = render()
            assert _reported(0) == expect[1], mode
            _fwd_close(e, rgbds, c["pred"]["rgbds"], "rgbds", mode)
            _fwd_close(e, term, c["pred"]["term_probs"], "term_probs", mode)
            if not matrix_is_hash(e):                # (the suite has no bar for a hash network's rendered variances)
                close(dvars, c["pred"]["depth_vars"], rtol=1e-3, atol=1e-5)
        else:
            with pytest.raises(K.NgmError) as exc:
                render()
            _refused(exc)
            refused = True
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 5: kNN evaluation
@pytest.mark.parametrize("name", CM.NAMES)
def test_knn_evaluation(name):
    e = CM.BY_NAME[name]
    c = matrix_knn_case(e)
    refused = False
    for mode, expect in e["knn"].items():
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        args = (fc, cu(c["params"]), c["pts"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV), c["K"], 10.0, 1.0)
        if CM.runs(expect):
            out = ops.field_eval_knn(*args)
            assert _reported(2) == expect[1], mode
            _fwd_close(e, out, c["ref"], "knn", mode)
        else:
            with pytest.raises(K.NgmError) as exc:
                ops.field_eval_knn(*args)
            _refused(exc)
            refused = True
    if refused:
        _next_call_succeeds()
