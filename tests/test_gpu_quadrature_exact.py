"""The quadrature kernels of csrc/ngm_composite.hip against the oracle in fp64, on inputs whose reference weight and gradient
reach every 64-sample wave step of a ray (tests/_quadrature_cases.py; test_quadrature_cases_cpu.py checks that they do) and with
more than one ray per wave -- the two conditions without which the carry between wave steps, the second and later gather
chunks, NST > 1 of the whole-ray backward, the re-reading variance pass and the segmented scans across ray boundaries cannot
be seen at any bar.

Every tensor is compared ray by ray (gpu_common.ray_close).  Its bar is the error of the fp32 torch restatement of the same
operation (`O.quadrature` on the float inputs, with autograd) against the same fp64 reference, times a margin, plus a floor of
four ulp of the tensor's scale, and never looser than the bar the suite already held that tensor to.  Margins, chosen after the
first run on the MI355X (profiles/r19_parity_margins.txt holds, per comparison, the worst ray's measured error, the bar that
binds on it and which of the two bars that is; worst error / bar in brackets):
  forward outputs                                   FWD_MARGIN   = 4  [0.94: D of neus at S = 255, 7 ulp]
  gradients of the exact kernels (k_composite_bwd)  GRAD_MARGIN  = 4  [0.68]
  gradients of k_composite_bwd_whole                WHOLE_MARGIN = 8  [0.24] (occ_pointwise_fast: hardware exp2 and reciprocal)
d_isds is one signed sum per ray, so it is normalised by the tensor's largest value as before (a ray whose sum cancels has no
scale of its own)."""
import pytest
import torch

import _quadrature_cases as Q
from gpu_common import DEV, MARGINS, NRGBD_KW, _test_id, make_renderer, ray_close
from neural_graph_mapping_amd import _capi as K
from neural_graph_mapping_amd import ops

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
FLOOR = 4 * ULP
FWD_MARGIN, GRAD_MARGIN, WHOLE_MARGIN = 4.0, 4.0, 8.0
# the bars the suite already holds these tensors to, in their own form: test_quadrature_golden's rtol 1e-5 + atol 2e-6 element
# by element; test_quadrature_backward_*'s fractions of the TENSOR's largest |gradient|
FWD_CAP = (1e-5, 2e-6, False)
GRAD_CAP = dict(d_colors=1e-5, d_geoms_pointwise=2e-5, d_geoms_neighbour=5e-5, d_isds=1e-4)
FWD = ("C", "D", "Cv", "Dv", "term", "W")
PACKED_OUT = ("C", "D", "Cv", "Dv", "term")


def _case(recipe, mode, N, S, seed=0):
    """inputs, cotangents, the fp64 reference and the fp32 restatement"""
    inp = getattr(Q, recipe + "_inputs")(mode, N, S, seed)
    cot = Q.cotangents(N, seed)
    return inp, cot, Q.reference(mode, inp, cot), Q.reference(mode, inp, cot, dtype=torch.float32)


def _gpu_quadrature(mode, inp, cot):
    rc = K.render_cfg(geometry_mode=mode, geometry_factor=Q.GF)
    c, g = inp["colors"].detach().to(DEV).requires_grad_(), inp["geoms"].detach().to(DEV).requires_grad_()
    i = None if inp["isds"] is None else inp["isds"].detach().to(DEV).requires_grad_()
    outs = ops.quadrature(rc, c, g, inp["dists"].to(DEV), inp["depths"].to(DEV), i)
    res = dict(zip(FWD, outs))
    ((res["C"] * cot["dC"].to(DEV)).sum() + (res["D"] * cot["dD"].to(DEV)).sum() + (res["term"] * cot["dT"].to(DEV)).sum()).backward()
    res["d_colors"], res["d_geoms"] = c.grad, g.grad
    if i is not None:
        res["d_isds"] = i.grad
    return {k: v.detach().cpu() for k, v in res.items()}


def _check(got, ref, r32, names, margin, caps, groups=None, fails=None):
    """every tensor of `names`, per group of rays (label -> (bool mask | None = all rays, derive)): the bar from the fp32
    restatement's error on THOSE rays (derive False: the suite's earlier bar alone) -> list of (tensor, group, error, bar)"""
    fails = [] if fails is None else fails
    for label, (rays, derive) in (groups or {"": (None, True)}).items():
        for n in names:
            err, bar = ray_close(got[n], ref[n], n + label, restated=r32[n], margin=margin if derive else None, floor=FLOOR,
                                 rays=rays, cap=caps[n])
            print(f"  {n}{label}: err {err:.3e} bar {bar:.3e}")
            if not err < bar:
                fails.append((n, label, err, bar))
    return fails


def _compare(mode, N, S, recipe="thin", whole_bwd=False):
    inp, cot, ref, r32 = _case(recipe, mode, N, S)
    got = _gpu_quadrature(mode, inp, cot)
    assert got["W"].shape == ref["W"].shape
    groups = None
    if recipe == "mixed":                                    # each half against the restatement's error on that half
        thin = Q.mixed_thin_rays(mode, N)
        # the opaque-ish rays are the earlier recipe: ill-conditioned here and there (a ray that one sample ends has variances
        # and later gradients of rounding size), so they are held to the earlier bars, in those bars' form
        groups = {" (thin rays)": (thin, True), " (opaque rays)": (~thin, False)}
    fails = _check(got, ref, r32, FWD, FWD_MARGIN, {n: FWD_CAP for n in FWD}, groups)
    ok = torch.ones(N, dtype=torch.bool)
    if mode == "neus":                                       # the clamp's kink: the gradient is discontinuous there (forward: not)
        kink = Q.neus_kink_rays(inp)
        assert float(kink.float().mean()) <= 0.05, float(kink.float().mean())
        ok = ~kink
    ggroups = {k: (ok if v is None else v & ok, dv) for k, (v, dv) in (groups or {"": (None, True)}).items()}
    margin = WHOLE_MARGIN if whole_bwd else GRAD_MARGIN
    gcap = GRAD_CAP["d_geoms_pointwise" if mode in Q.POINTWISE else "d_geoms_neighbour"]
    _check(got, ref, r32, ("d_colors", "d_geoms"), margin, dict(d_colors=(GRAD_CAP["d_colors"], 0.0, True), d_geoms=(gcap, 0.0, True)),
           ggroups, fails)
    if mode == "neus":
        assert got["d_isds"].shape == inp["isds"].shape
        scale = float(ref["d_isds"][ok].abs().max())                # (S = 1: no sample carries weight, every gradient is zero)
        rel = lambda x: float((x[ok].double() - ref["d_isds"][ok]).abs().max()) / scale if scale > 0 else float(x.abs().max() > 0) * 1e30
        e32 = rel(r32["d_isds"])
        bar = min(GRAD_CAP["d_isds"], margin * e32 + FLOOR)
        err = rel(got["d_isds"])
        MARGINS.append(dict(test=_test_id(), name=f"d_isds[fp32 torch {e32:.2e}]", err=err, tol=bar))
        print(f"  d_isds: err {err:.3e} bar {bar:.3e}")
        if not err < bar:
            fails.append(("d_isds", "", err, bar))
    assert not fails, (mode, N, S, fails)


# ------------------------------------------------------------------------------------------------ ops.quadrature (SRC 0)
@pytest.mark.parametrize("mode", Q.POINTWISE)
@pytest.mark.parametrize("S", Q.WHOLE_S)
def test_whole_ray_forward_and_backward(mode, S):
    """k_composite_fwd_whole<0> and k_composite_bwd_whole<S / 64>, every NST; 256 is exactly one gather chunk, 320 one more step"""
    _compare(mode, 5, S, whole_bwd=True)


@pytest.mark.parametrize("mode", Q.POINTWISE)
@pytest.mark.parametrize("S", Q.WHOLE_BIG_S)
def test_whole_ray_forward_beyond_the_whole_ray_backward(mode, S):
    """S > 512: the whole-ray forward (1024: four gather chunks) with the generic backward"""
    _compare(mode, 5, S)


@pytest.mark.parametrize("mode", Q.POINTWISE)
@pytest.mark.parametrize("N,S", Q.MULTI_WHOLE)
def test_whole_ray_kernels_with_several_rays_per_wave(mode, N, S):
    """2 and 3 rays per wave (the last wave holds one): the LDS planes and the carries are reused from ray to ray"""
    _compare(mode, N, S, whole_bwd=True)


@pytest.mark.parametrize("mode,S", [(m, s) for m in Q.MODES for s in Q.GENERIC_S[m]])
def test_generic_kernels(mode, S):
    """k_composite_fwd<KEEP> / <!KEEP> (255 / 256 / 257 straddle the threshold: above it the variance pass reads memory again)
    and k_composite_bwd, one ray per wave, rays of up to 16 wave steps"""
    _compare(mode, 5, S)


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("S", Q.FULL_S)
def test_generic_kernels_with_full_batches(mode, S):
    """33 rays per wave: a batch of BR = 32 rays, then a batch of one; even rays opaque-ish, odd rays thin, so sharp and flat
    transmittance both cross ray boundaries inside a wave step"""
    _compare(mode, Q.FULL_N, S, recipe="mixed")


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("N,S", Q.MULTI_GENERIC)
def test_generic_kernels_with_two_rays_per_wave(mode, N, S):
    """S = 200: BR = 1 in the forward (256 / 200) and 5 in the backward (1024 / 200); S = 300: the re-reading forward, BR = 3"""
    _compare(mode, N, S)


# ------------------------------------------------------------------------------------------------ packed (N,S,4) source
@pytest.mark.parametrize("mode,S", [(m, s) for m in Q.POINTWISE for s in Q.PACKED_S] + [("density", 100), ("density", 300)])
def test_packed_source(mode, S):
    """ops.composite_packed: k_composite_fwd_whole<9> (64, 320, 1024) and the generic packed path (100, 300), a colour factor
    other than one, and samples behind the camera on three rays, which the reference overwrites with its constant"""
    N, cf = 7, 0.5                                                    # (0.5: the product with a colour is exact in fp32)
    inp = Q.thin_inputs(mode, N, S, 2)
    gen = torch.Generator().manual_seed(S)
    pz = -inp["depths"].clone()
    for ray, (a, b) in ((1, (5, 20)), (2, (60, 70)), (3, (S - 9, S))):         # (2: across a wave step's boundary where S > 64)
        pz[ray, a:min(b, S)] *= -1.0
    pcam = torch.cat([torch.randn(N, S, 2, generator=gen), pz[..., None]], -1)
    o4 = torch.cat([inp["colors"], inp["geoms"][..., None]], -1)
    const = -100.0 if mode in ("occupancy", "density") else 1.0
    rinp = dict(colors=cf * inp["colors"], geoms=torch.where(pz > 0, torch.full_like(pz, const), inp["geoms"]), dists=inp["dists"],
                depths=-pz, isds=None)
    with torch.no_grad():
        ref, r32 = Q.reference(mode, rinp), Q.reference(mode, rinp, dtype=torch.float32)
    rc = K.render_cfg(geometry_mode=mode, geometry_factor=Q.GF, color_factor=cf, overwrite_behind_camera=True)
    rgbd, cv, dv, term = ops.composite_packed(rc, o4.to(DEV), inp["dists"].to(DEV), pcam.to(DEV))
    got = dict(C=rgbd[:, :3], D=rgbd[:, 3], Cv=cv, Dv=dv, term=term)
    fails = _check(got, ref, r32, PACKED_OUT, FWD_MARGIN, {n: FWD_CAP for n in PACKED_OUT})
    assert not fails, (mode, S, fails)


# ------------------------------------------------------------------------------------------------ pair records (SRC 1..8)
@pytest.mark.parametrize("mode", Q.POINTWISE)
@pytest.mark.parametrize("K_,S,N,block", Q.PAIR_CASES)
def test_pair_record_source_of_the_fused_image_call(mode, K_, S, N, block):
    """ngm_render_eval_knn (k_composite_fwd_whole<K>: the blend inside the gather, chunks of 5 steps for K <= 4 and of 2 above)
    against the fp64 quadrature of the STAGED operators' blended outputs, distances and camera-frame points on the same draws
    -- not against the staged composite_packed, which is the same kernel.  The blend inside the gather runs in k_knn_blend's
    fmaf order, so the comparison isolates the quadrature.  The scene (Q.pair_scene) is thin; that the reference has weight
    in a step of the second or a later chunk, in two different steps, and that a ray has a step wholly outside every field
    (the all_ref shortcut) next to a mixed one is asserted on at least a quarter of the rays (S = 64 is a single step: mixed)."""
    seed, cf = 77, 0.5
    sc = Q.pair_scene(mode, S, N)
    r = make_renderer(Q.PAIR_FIELD, dict(num_samples_coarse=8, num_samples_depth_guided=16), sc["pos"].shape[0], sc["params"])
    params = {k: v for k, v in r._model.kernel_params().items() if k != "_neus_sd"}
    rc = K.render_cfg(geometry_mode=mode, geometry_factor=Q.GF, color_factor=cf, num_samples_coarse=S, num_samples_guided=0, **NRGBD_KW)
    d = {k: sc[k].to(DEV) for k in ("pos", "quat", "ijs", "c2ws", "near", "far")}
    ov = sc["outside_value"]
    rgbd, cv, dv, term = ops.render_eval_knn(r._fc, rc, params, d["ijs"], d["c2ws"], d["pos"], d["quat"], K_, 10.0, ov,
                                             near=d["near"], far=d["far"], seed=seed, ray_block=block)
    o4s, dists, pcs = [], [], []
    for s0 in range(0, N, block):
        sl = slice(s0, s0 + block)
        pc, pw, dist = ops.sample_rays_world(rc, d["ijs"][sl][None], d["c2ws"][sl][None], d["near"][sl][None], d["far"][sl][None],
                                             seed=seed + s0)
        o4s.append(ops.field_eval_knn(r._fc, params, pw.view(-1, 3), d["pos"], d["quat"], K_, 10.0, ov).view(-1, S, 4).cpu())
        dists.append(dist.view(-1, S).cpu())
        pcs.append(pc.view(-1, S, 3).cpu())
    o4, dist, pc = torch.cat(o4s), torch.cat(dists), torch.cat(pcs)
    rinp = dict(colors=cf * o4[..., :3], geoms=o4[..., 3], dists=dist, depths=-pc[..., 2], isds=None)
    with torch.no_grad():
        ref, r32 = Q.reference(mode, rinp), Q.reference(mode, rinp, dtype=torch.float32)
    cond = Q.pair_conditions(o4, ref["W"], ov, 5 if K_ <= 4 else 2)
    print("  conditions:", cond)
    if S > 64:
        assert cond["later_chunk"] >= 0.25 and cond["two_steps"] >= 0.25 and cond["outside_and_mixed"] >= 0.25, cond
    else:
        assert cond["mixed"] >= 0.25, cond
    got = dict(C=rgbd[:, :3].cpu(), D=rgbd[:, 3].cpu(), Cv=cv.cpu(), Dv=dv.cpu(), term=term.cpu())
    fails = _check(got, ref, r32, PACKED_OUT, FWD_MARGIN, {n: FWD_CAP for n in PACKED_OUT})
    assert not fails, (mode, K_, S, N, fails)
