"""Problems of the loss-term tests (test_loss_terms_cpu.py and, -m gpu, test_gpu_loss_terms.py): inputs that reach the NLL branch
of `photometric_loss: gaussian_nll`, inputs on either side of its switch, and the default losses one term at a time.  Every
reference is the oracle in fp64 (stored as fp32), computed once per session and shared by the tests of both files."""
import torch

from gpu_common import KINK, NRGBD, kink_free_draws, nll_branch_targets, nll_depth_targets, synth_target
from neural_graph_mapping_amd import _capi as K
from oracle import ngm_oracle as O

FOURIER = dict(encoding="fourier", dim_enc=64, num_layers=2)
HASH = dict(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
NETS = dict(fourier=FOURIER, hash=HASH)
NLL_SHAPES = [(3, 37, 5, 2), (2, 130, 20, 4)]
TERM_SHAPE = (3, 41, 9, 5)
# nll_branch_targets' scale: 1.5 sigma (the colour-variance path then carries 17-85 % of every tensor's gradient in nrgbd
# mode).  Occupancy mode at 1.5: 4 % of the last layer's bias in the (3, 37, 5, 2) case, so those cases sit at 1 sigma (32 %+)
NLL_SCALE = dict(nrgbd=1.5, occupancy=1.0)
# the weights of the shipped configuration (tests: termination 0.3), and the same with every term switched off
WEIGHTS = dict(termination_weight=0.3, photometric_weight=1.0, depth_weight=1.0, freespace_weight=40.0, tsdf_weight=50.0)
NO_WEIGHTS = {k: 0.0 for k in WEIGHTS}
# one loss term at a time: name -> (its weight's key, loss mode overrides, key of the term in the loss dict)
TERMS = {
    "termination": ("termination_weight", {}, "termination"),
    "photometric_l1": ("photometric_weight", dict(photometric_loss="l1"), "photometric_l1"),
    "photometric_l2": ("photometric_weight", dict(photometric_loss="l2"), "photometric_l2"),
    "depth_huber": ("depth_weight", dict(depth_loss="huber"), "depth_huber"),
    "freespace": ("freespace_weight", {}, "freespace"),
    "tsdf": ("tsdf_weight", {}, "tsdf"),
}
_CACHE = {}


def _d(x, dtype):
    return x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x


def oracle_run(c, dtype=torch.float64, t=None, rs=None, detach_color_vars=False, backward=True):
    """The oracle on case `c` in `dtype` -> (prediction, loss dict, gradients | None); `detach_color_vars`: the same loss with
    the rendered colour variances held constant (what is left of the gradient when their path is cut)."""
    t, rs = t or c["t"], rs or c["rs"]
    t = {k: _d(v, dtype) for k, v in t.items()}
    po = {k: v.detach().to(dtype, copy=True).requires_grad_(k not in K.NO_GRAD_PARAMS) for k, v in c["params"].items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, _d(c["pos"], dtype), _d(c["quat"], dtype), po, c["fs"], rs, t["near"], t["far"],
                        t["gt"], _d(c["u_c"], dtype), _d(c["u_g"], dtype))
    lp = dict(pred, color_vars=pred["color_vars"].detach()) if detach_color_vars else pred
    loss = O.compute_losses(lp, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    grads = None
    if backward:
        loss["combined"].backward()
        grads = {k: v.grad for k, v in po.items() if v.grad is not None}
    return pred, loss, grads


def mean_color_nll(pred, t):
    """(mean colour NLL over the selection, number of selected rays): what losses.py:30-35 compares with 2"""
    m = t["depth_mask"] & (pred["term_probs"] > 0.8)
    e = (t["rgbds"][m][:, :3] - pred["rgbds"][m][:, :3]).double()
    v = pred["color_vars"][m].double()
    return float((0.5 * e ** 2 / v + 0.5 * torch.log(v)).mean()), int(m.sum())


def base_case(net, shape, geom="nrgbd"):
    """Fields, rays and kink-free draws of one shape, like gpu_common.ragged_case -- shared by every loss configuration on it"""
    key = ("base", net, shape, geom)
    if key in _CACHE:
        return _CACHE[key]
    F, R, n_c, n_g = shape
    fkw = dict(NETS[net])
    torch.manual_seed(F * 1000 + R)
    pos, quat, t = synth_target(F, R, seed=R)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, geometry_mode=geom, geometry_factor=20.0)
    params = O.init_params(fs, F, seed=R, sigma=3.0)
    if shape not in NLL_SHAPES:            # like ragged_case; the NLL shapes keep test_nll_loss_modes_ragged_vs_oracle's set-up
        params[f"_linears.{fkw['num_layers']}.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    n0 = len(KINK)
    # hash: the band of the randomised hash sweep (two fp32 evaluations of a hash encoding differ by ~5e-4)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g, margin=2e-3 if net == "hash" else 5e-5)
    kink = KINK[n0:]
    del KINK[n0:]                          # kept with the case (built once, by whichever test asks first)
    c = dict(net=net, F=F, R=R, n_c=n_c, n_g=n_g, geom=geom, fkw=fkw, fs=fs, pos=pos, quat=quat, t=t, params=params, u_c=u_c,
             u_g=u_g, kink=kink, neutralised=kink[-1]["neutralised_frac"], rs=rs)
    with torch.no_grad():
        c["pred0"], _, _ = oracle_run(c, backward=False)           # fp64, targets as drawn
    _CACHE[key] = c
    return c


def _finish(c, t, weights, modes):
    """case = base + targets + loss configuration, with the fp64 oracle's prediction, losses and gradients (stored as fp32)"""
    c = dict(c)
    ckw = dict(num_samples_coarse=c["n_c"], num_samples_depth_guided=c["n_g"], geometry_mode=c["geom"], geometry_factor=20.0,
               **weights, **modes)
    rs = O.RenderSpec(**ckw)
    c.update(t=t, ckw=ckw, rs=rs)
    pred, loss, grads = oracle_run(c)
    c["mean_nll"], c["n_sel"] = mean_color_nll({k: v.detach() for k, v in pred.items() if v is not None}, t)
    c["pred"] = {k: (v.detach().float() if torch.is_tensor(v) else v) for k, v in pred.items()}
    c["loss"] = {k: v.detach().float() for k, v in loss.items()}
    c["grads"] = {k: v.float() for k, v in grads.items()}
    c["grads64"] = grads
    return c


def nll_scale_for(c, lo, hi, seed):
    """bisection on the fp64 oracle's prediction: the scale at which nll_branch_targets' mean colour NLL is (lo + hi) / 2"""
    def mean_at(s):
        t = nll_branch_targets(c["t"], c["pred0"], s, torch.Generator().manual_seed(seed))
        return mean_color_nll(c["pred0"], {k: _d(v, torch.float64) for k, v in t.items()})[0]
    a, b, goal = 0.0, 64.0, 0.5 * (lo + hi)
    assert mean_at(a) < goal < mean_at(b)
    for _ in range(60):
        m = 0.5 * (a + b)
        a, b = (m, b) if mean_at(m) < goal else (a, m)
    return 0.5 * (a + b)


def nll_case(shape, photo="gaussian_nll", depth="huber", geom="nrgbd", variant="full"):
    """`variant`: "full" (every loss term at its usual weight, targets at NLL_SCALE[geom]), "photo_only" (the photometric term alone),
    "thr_nll" / "thr_l1" (every term; mean colour NLL in [0.5, 1.5] / [2.5, 3.5]: either side of the switch at 2)"""
    key = ("nll", shape, photo, depth, geom, variant)
    if key not in _CACHE:
        b = base_case("fourier", shape, geom)
        seed = 1000 * shape[0] + shape[1]
        scale = {"thr_nll": lambda: nll_scale_for(b, 0.5, 1.5, seed), "thr_l1": lambda: nll_scale_for(b, 2.5, 3.5, seed)}.get(
            variant, lambda: NLL_SCALE[geom])()
        gen = torch.Generator().manual_seed(seed)
        t = nll_branch_targets(b["t"], b["pred0"], scale, gen)
        t = nll_depth_targets(t, b["pred0"], NLL_SCALE[geom], gen)
        weights = dict(NO_WEIGHTS, photometric_weight=1.0) if variant == "photo_only" else dict(WEIGHTS)
        c = _finish(b, t, weights, dict(photometric_loss=photo, depth_loss=depth))
        c["scale"] = scale
        _CACHE[key] = c
    return _CACHE[key]


def huber_targets(t, pred64, delta, gen):
    """Target depths on both sides of the Huber loss's delta: target - D in [0.7, 0.95] delta on 40 % of the rays (the quadratic
    zone, whose seed is the error itself: the hash network's fp32 depth is uncertain by 2e-4, one per cent of an error of 2 cm)
    and in [1.2, 4] delta on the others -- no ray within 2.5e-3 of the kink at delta.  All errors have one sign: with random
    signs the rays' contributions cancel in the biases' gradients (measured, field 0 of the (3, 41, 9, 5) hash case: a sum 25
    times smaller than another field's) and the fp32 ORACLE misses the fp64 one by 1.6e-2 of such a field's scale"""
    D = pred64["rgbds"][..., 3].detach().double()
    u = torch.rand(D.shape, generator=gen, dtype=torch.float64)
    big = torch.rand(D.shape, generator=gen) < 0.6
    sign = 1.0
    mag = torch.where(big, 1.2 + 2.8 * u, 0.7 + 0.25 * u) * delta
    t = dict(t)
    t["rgbds"] = t["rgbds"].clone()
    t["rgbds"][..., 3] = (D + sign * mag).to(t["rgbds"].dtype)
    return t


def term_case(net, term, shape=TERM_SHAPE):
    """the default losses with every weight but `term`'s at zero (TERMS)"""
    key = ("term", net, term, shape)
    if key not in _CACHE:
        b = base_case(net, shape)
        wk, modes, _ = TERMS[term]
        t = dict(b["t"])
        if term == "depth_huber":
            t = huber_targets(t, b["pred0"], 0.05, torch.Generator().manual_seed(shape[1]))
        # rays on the selection's threshold (term_probs > 0.8, rm.py:1787-1788) could fall on either side in fp32
        t["depth_mask"] = t["depth_mask"] & ~((b["pred0"]["term_probs"] - 0.8).abs() < 1e-4)
        _CACHE[key] = _finish(b, t, dict(NO_WEIGHTS, **{wk: WEIGHTS[wk]}), modes)
    return _CACHE[key]


SEEDED_OUTPUTS = ("color_vars", "depth_vars", "rgbds", "term_probs", "freespace_geometry", "tsdf_residuals")
# field 0 of (2, 130, 20, 4) terminates with probability 1 - 5e-8: its d term_probs / d parameters is 1e-8 of field 1's, below
# what 1 - sum(w) resolves in fp32 -- the termination probability alone is seeded on (3, 41, 9, 5) instead
SEEDED_CASES = [(s, o) for s in NLL_SHAPES for o in SEEDED_OUTPUTS if (s, o) != ((2, 130, 20, 4), "term_probs")] + [(TERM_SHAPE, "term_probs")]


def seeded_case(shape, output, geom="nrgbd"):
    """render_ijs under autograd with a loss that reads ONE output: sum(output * cotangent), the cotangent fixed and drawn from
    U(0.5, 1.5) (one sign: no cancellation between rays in the biases' gradients).  Reference: oracle autograd in fp64."""
    key = ("seeded", shape, output, geom)
    if key not in _CACHE:
        c = dict(base_case("fourier", shape, geom))
        c["ckw"] = dict(num_samples_coarse=c["n_c"], num_samples_depth_guided=c["n_g"], geometry_mode=geom, geometry_factor=20.0,
                        **WEIGHTS)
        c["rs"] = O.RenderSpec(**c["ckw"])
        c["output"] = output
        c["cot"] = 0.5 + torch.rand(c["pred0"][output].shape, generator=torch.Generator().manual_seed(shape[1] + len(output)))
        c["grads64"] = seeded_oracle(c, torch.float64)
        c["grads"] = {k: v.float() for k, v in c["grads64"].items()}
        _CACHE[key] = c
    return _CACHE[key]


def seeded_oracle(c, dtype):
    t = {k: _d(v, dtype) for k, v in c["t"].items()}
    po = {k: v.detach().to(dtype, copy=True).requires_grad_(k not in K.NO_GRAD_PARAMS) for k, v in c["params"].items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, _d(c["pos"], dtype), _d(c["quat"], dtype), po, c["fs"], c["rs"], t["near"],
                        t["far"], t["gt"], _d(c["u_c"], dtype), _d(c["u_g"], dtype))
    (pred[c["output"]] * c["cot"].to(dtype)).sum().backward()
    return {k: v.grad for k, v in po.items() if v.grad is not None}
