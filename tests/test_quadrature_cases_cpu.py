"""Conditions on the INPUTS of test_gpu_quadrature_exact.py, checked in the fp64 reference without a GPU: a comparison of the
quadrature kernels sees a wave step only if the reference puts weight and gradient there.  These are no measurements of a
kernel; a recipe that misses one is changed, not the bound."""
import pytest
import torch

import _quadrature_cases as Q


def _conditions(mode, S, N, seed):
    inp = Q.thin_inputs(mode, N, S, seed)
    ref = Q.reference(mode, inp, Q.cotangents(N, seed))
    rows = slice(1, None)                                     # ray 0 holds the exact-zero probes: opaque in nrgbd
    sh = Q.step_shares(ref["W"])[rows]
    nst = sh.shape[-1]
    assert float(sh.min()) >= 1.0 / (8 * nst), (mode, S, "weight share of a wave step", float(sh.min()), 1.0 / (8 * nst))
    if mode != "neus":
        t = ref["term"][rows]
        assert 0.4 <= float(t.min()) and float(t.max()) <= 0.98, (mode, S, "term", float(t.min()), float(t.max()))
    # the gradient reaches the last wave step that holds a sample with a weight: density and neus drop sample S - 1, whose
    # gradient is zero (density) or its predecessor's occupancy's alone (neus), so at S = 65 the step that holds only that
    # sample has nothing of its own to show
    dg = ref["d_geoms"].abs()[rows]
    Sg = Q.s_eff(mode, S)
    last = dg[:, ((Sg - 1) // 64) * 64:Sg].max(-1).values
    ratio = last / dg.max(-1).values
    if N < 1000:
        assert float(ratio.min()) >= 0.1, (mode, S, "d_geoms in the last wave step / the ray's largest", float(ratio.min()))
    else:
        # thousands of rays with random cotangents: a_k = dC . c_k + dD d_k + dT is nearly constant along a ray whose dC is
        # small, and may cross zero at the ray's end, so the minimum over all rays is a tail figure (measured 0.06 .. 0.09 on one
        # or two rays of 6150).  A wrong last step is wrong on every ray; it is in sight if the condition holds on nearly all
        # of them (the pair-record cases ask a quarter)
        assert float((ratio >= 0.1).float().mean()) >= 0.99, (mode, S, float((ratio >= 0.1).float().mean()), float(ratio.min()))
    if mode == "neus":
        frac = float(Q.neus_kink_rays(inp).float().mean())
        assert frac <= 0.05, (mode, S, "rays within 1e-4 of the clamp's kink", frac)


@pytest.mark.parametrize("mode,S", Q.ALL_MODE_S, ids=lambda v: str(v))
def test_thin_inputs_put_weight_and_gradient_in_every_wave_step(mode, S):
    _conditions(mode, S, 5, 0)                                # the rays the GPU tests use
    _conditions(mode, S, 48, 1)                               # and the recipe at large


@pytest.mark.parametrize("mode,N,S", [(m, n, s) for n, s in Q.MULTI_WHOLE for m in Q.POINTWISE])
def test_thin_inputs_of_the_many_ray_cases(mode, N, S):
    inp = Q.thin_inputs(mode, N, S, 0)
    with torch.no_grad():
        ref = Q.reference(mode, inp)
    sh = Q.step_shares(ref["W"])[1:]
    assert float(sh.min()) >= 1.0 / (8 * sh.shape[-1])
    assert 0.4 <= float(ref["term"][1:].min()) and float(ref["term"][1:].max()) <= 0.98


@pytest.mark.parametrize("mode,bound", [("nrgbd", 1e-20), ("occupancy", 1e-20)])
def test_the_earlier_recipe_is_opaque_after_one_wave_step(mode, bound):
    """the finding the new cases answer: `geoms = 0.1 * randn` at geometry_factor 20 (test_quadrature_backward_vs_oracle, S =
    512) leaves less than 1e-20 of a ray's weight beyond sample 64, and gradients of the same size: at bars of 1e-5 a kernel
    that returned zeros for every later sample would pass"""
    S = 512
    torch.manual_seed(S)
    colors = torch.rand(3, S, 3)
    geoms = 0.1 * torch.randn(3, S)
    dists = torch.sort(torch.rand(3, S) * 3 + 0.5, -1)[0]
    inp = dict(colors=colors, geoms=geoms, dists=dists, depths=dists * 0.9, isds=None)
    ref = Q.reference(mode, inp, Q.cotangents(3, 0))
    beyond = ref["W"][:, 64:].sum(-1) / ref["W"].sum(-1)
    assert float(beyond.max()) < bound, float(beyond.max())
    dg = ref["d_geoms"].abs()
    assert float(dg[:, 64:].max() / dg.max()) < bound


def test_step_shares():
    W = torch.zeros(2, 130, dtype=torch.float64)
    W[0, 0], W[0, 64], W[0, 129] = 1.0, 2.0, 1.0
    W[1, 70] = 3.0
    assert torch.equal(Q.step_shares(W), torch.tensor([[0.25, 0.5, 0.25], [0.0, 1.0, 0.0]], dtype=torch.float64))


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("N,S", Q.MULTI_GENERIC)
def test_thin_inputs_of_the_many_ray_generic_cases(mode, N, S):
    _conditions(mode, S, N, 0)


@pytest.mark.parametrize("S", Q.FULL_S)
def test_mixed_neus_inputs_leave_at_most_a_twentieth_of_the_rays_on_the_kink(S):
    frac = float(Q.neus_kink_rays(Q.mixed_inputs("neus", Q.FULL_N, S, 0)).float().mean())
    assert frac <= 0.05, (S, frac)


# ---- gpu_common.ray_close, the comparison every tensor of test_gpu_quadrature_exact.py goes through (it needs no GPU)
def _ray_close(*a, **k):
    import gpu_common
    n = len(gpu_common.MARGINS)
    try:
        return gpu_common.ray_close(*a, **k)
    finally:
        del gpu_common.MARGINS[n:]                            # nothing measured on a GPU: keep it out of the session's file


def test_ray_close_does_not_let_one_ray_hide_another():
    b = torch.tensor([[100.0, 1.0], [1e-3, 2e-3]])
    a = b.clone()
    a[1, 0] += 1e-3
    assert float((a - b).abs().max() / b.abs().max()) < 2e-5          # one normalisation per tensor: passes a bar of 2e-5
    err, tol = _ray_close(a, b, "x", restated=b, margin=4.0, cap=(2e-5, 0.0, False))
    assert abs(err - 0.5) < 1e-6 and tol <= 2e-5 and not err < tol
    err, tol = _ray_close(b, b, "x", restated=b, margin=4.0)
    assert err == 0.0 and err < tol


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_ray_close_fails_on_a_ray_that_is_not_finite(bad):
    """a kernel that wrote NaN past its first wave step, or on the second ray of a wave, must not read as error 0"""
    torch.manual_seed(0)
    b = torch.rand(3, 128, dtype=torch.float64) + 0.5
    r32 = b.float()
    a = r32.clone()
    a[1, 40:64] = bad
    for kw in (dict(restated=r32, margin=4.0), dict(restated=r32, margin=4.0, cap=(1e-5, 2e-6, False)), dict(cap=(1e-5, 0.0, True)),
               dict(restated=r32, margin=4.0, rays=torch.tensor([False, True, True]))):
        err, tol = _ray_close(a, b, "x", **kw)
        assert not err < tol, (kw, err, tol)
    err, tol = _ray_close(a, b, "x", restated=r32, margin=4.0, rays=torch.tensor([True, False, True]))
    assert err < tol                                          # the rays left out are left out


def test_ray_close_bars():
    torch.manual_seed(1)
    b = torch.rand(4, 64, dtype=torch.float64) + 0.5
    r32 = b.float()
    # the fp32 rounding of the reference itself passes its own derived bar, and reports the measured error
    err, tol = _ray_close(r32, b, "x", restated=r32, margin=4.0)
    assert 0 < err < 2.0 ** -23 and err < tol < 8 * 2.0 ** -23 + 4 * 2.0 ** -23
    # the earlier bar binds where it is the smaller one, in its own form: rtol * the TENSOR's scale for gradients
    b2 = b.clone()
    b2[3] *= 1e-3                                             # a ray of small values
    a = b2.clone()
    a[3, 5] += 3e-5 * float(b2.abs().max())
    err, tol = _ray_close(a, b2, "x", cap=(2e-5, 0.0, True))
    assert not err < tol
    err, tol = _ray_close(a, b2, "x", cap=(5e-5, 0.0, True))
    assert err < tol
    # a ray whose reference is all zero must be all zero
    z = b.clone()
    z[2] = 0.0
    a = z.clone()
    err, tol = _ray_close(a, z, "x", restated=z.float(), margin=4.0, floor=0.0)
    assert err == 0.0
    a[2, 7] = 1e-12
    err, tol = _ray_close(a, z, "x", restated=z.float(), margin=4.0, floor=0.0)
    assert not err < tol
    # a reference that is zero everywhere (S = 1 in density and neus: no sample carries weight) is met only by zeros
    z0 = torch.zeros(3, 4, dtype=torch.float64)
    err, tol = _ray_close(z0.float(), z0, "x", restated=z0.float(), margin=4.0, cap=(1e-5, 0.0, True))
    assert err == 0.0 and err < tol
    a = z0.float()
    a[1, 1] = 1e-30
    err, tol = _ray_close(a, z0, "x", restated=z0.float(), margin=4.0, cap=(1e-5, 0.0, True))
    assert not err < tol
