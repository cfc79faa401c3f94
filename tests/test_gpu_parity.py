"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against
  (a) the golden fixtures generated from the real reference,
  (b) the CPU oracle on seeded random inputs (small sizes),
  (c) size-independent properties at the full benchmark size (4096 rays x 128 samples).
Tolerances (fp32): forward 2e-4 rel / 2e-5 abs; gradients 2e-3 of the tensor's max |grad|
(same bars the oracle meets against the reference in test_oracle_golden.py); sample distances are
bit-exact."""
import ctypes as C
import os

import pytest
import torch

from conftest import load_golden, split_prefix

pytestmark = pytest.mark.gpu

from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402
from gpu_common import (CASES, DEV, NRGBD, NRGBD_KW, away_from_relu_boundaries, close, cu, grad_close,  # noqa: E402
                        hash_grad_close, host_philox_uniform, kink_free_draws, make_renderer, make_target, ragged_case, synth_target,
                        compare_losses)

def test_device_is_gfx950_and_library_loaded():
    n = C.c_int(0)
    name = C.create_string_buffer(128)
    assert K.lib().ngm_device_info(C.byref(n), name, 128) == 0
    assert n.value >= 64
    assert b"gfx9" in name.value


# ---------------------------------------------------------------------------------- sampler (G1-G3)
def test_sampler_golden_bit_exact():
    g = load_golden("g3_sample_merged")
    rc = K.render_cfg(num_samples_coarse=g["u_coarse"].shape[-1], num_samples_guided=g["u_guided"].shape[-1],
                      truncation_distance=float(g["rho"]), **NRGBD_KW)
    d = cu({k: g[k] for k in ("ijs", "near", "far", "gt", "u_coarse", "u_guided")})
    pts, t, _ = ops.sample_rays(rc, d["ijs"], d["near"], d["far"], d["gt"], d["u_coarse"], d["u_guided"])
    assert torch.equal(t.cpu(), g["distances"])          # rank merge == torch.sort, fp32 op order identical
    close(pts, g["points"], rtol=1e-6, atol=1e-6)
    g2 = load_golden("g2_sample_uniform")
    rc2 = K.render_cfg(num_samples_coarse=g2["u"].shape[-1], num_samples_guided=0, **NRGBD_KW)
    d2 = cu({k: g2[k] for k in ("ijs", "near", "far", "u")})
    pts2, t2, _ = ops.sample_rays(rc2, d2["ijs"], d2["near"], d2["far"], None, d2["u"])
    assert torch.equal(t2.cpu(), g2["distances"])
    g1 = load_golden("g1_directions")
    ij = g1["ijs"][None].to(DEV)
    rc1 = K.render_cfg(num_samples_coarse=1, num_samples_guided=0, **NRGBD_KW)
    z = torch.zeros(1, ij.shape[1], device=DEV)
    _, _, dirs = ops.sample_rays(rc1, ij, z, z + 1, None, torch.zeros(1, ij.shape[1], 1, device=DEV))
    close(dirs[0], g1["dirs"], rtol=1e-6, atol=1e-7)


def test_weighted_bin_sampler_golden_bit_exact():
    """Camera.sample_ijs_uniform's weighted-bin branch (camera.py:277-289): fixture G23 from the real reference, distances
    bit for bit (torch.cumsum's CPU arithmetic: sequential, fp64 accumulator, fp32 prefixes; first bin whose sum + 1e-3 reaches the draw, start + size * offset draw)"""
    g = load_golden("g23_weighted_bins")
    S = g["u_bin"].shape[-1]
    rc = K.render_cfg(num_samples_coarse=S, num_samples_guided=0, **NRGBD_KW)
    d = cu({k: g[k] for k in ("ijs", "boundaries", "weights", "u_bin", "u_off")})
    pts, t, dirs = ops.sample_rays_weighted(rc, d["ijs"], d["boundaries"], d["weights"], d["u_bin"], d["u_off"])
    assert torch.equal(t.cpu(), g["distances"])
    close(pts, g["points"], rtol=1e-6, atol=1e-6)
    close(dirs, O.ijs_to_directions(g["ijs"], NRGBD), rtol=1e-6, atol=1e-7)
    # flat (R,2) pixel lists are accepted like the reference's `...` leading dims
    pts1, t1, _ = ops.sample_rays_weighted(rc, d["ijs"][0], d["boundaries"][0], d["weights"][0], d["u_bin"][0], d["u_off"][0])
    assert torch.equal(t1[0], t[0])
    with pytest.raises(ValueError):
        ops.sample_rays_weighted(rc, d["ijs"], d["boundaries"][..., :-1], d["weights"], d["u_bin"], d["u_off"])
    with pytest.raises(ValueError, match="go together"):       # one draw array without the other (checked before the library is called)
        ops.sample_rays_weighted(rc, d["ijs"], d["boundaries"], d["weights"], d["u_bin"], None)
    with pytest.raises(ValueError, match="must have shape"):   # draws sized for another sample count would be read out of bounds
        ops.sample_rays_weighted(rc, d["ijs"], d["boundaries"], d["weights"], d["u_bin"][..., :-1], d["u_off"][..., :-1])


@pytest.mark.parametrize("S,B", [(1, 1), (64, 7), (200, 128), (16, 3000)])
def test_weighted_bin_sampler_vs_oracle_random(S, B):
    """random bins incl. zero-weight ones, weights that stop short of 1 (the draw beyond the last cumulative weight takes the
    last bin -- the reference's gather is out of range there -- so such draws are excluded from the comparison), and the
    in-kernel Philox draws: every distance inside a bin the weights allow, histogram of bins ~ the weights"""
    torch.manual_seed(S * 1000 + B)
    F, R = 3, 41
    ijs = torch.stack([torch.randint(0, 480, (F, R)), torch.randint(0, 640, (F, R))], -1)
    edges = torch.sort(torch.rand(F, R, B + 1) * 5 + 0.1, dim=-1).values
    w = torch.rand(F, R, B) ** 3
    w[torch.rand(F, R, B) < 0.3] = 0.0
    w[..., 0] += 0.01
    w = w / w.sum(-1, keepdim=True)
    w[0, 0] *= 0.5                                         # sums to 0.5: half the draws are beyond the last cumulative weight
    u_bin, u_off = torch.rand(F, R, S), torch.rand(F, R, S)
    cum = torch.cumsum(w, -1) + 1e-3
    ok = u_bin <= cum[..., -1:]
    pts_o, t_o, _ = O.sample_rays_weighted(ijs, NRGBD, edges, w, torch.where(ok, u_bin, torch.zeros(())), u_off)
    rc = K.render_cfg(num_samples_coarse=S, num_samples_guided=0, **NRGBD_KW)
    pts, t, _ = ops.sample_rays_weighted(rc, ijs.to(DEV), edges.to(DEV), w.to(DEV), u_bin.to(DEV), u_off.to(DEV))
    assert torch.equal(t.cpu()[ok], t_o[ok])
    close(pts.cpu()[ok], pts_o[ok], rtol=1e-6, atol=1e-6)
    assert int((~ok).sum()) > 0 or S == 1
    last = edges[..., -2:-1].expand_as(t_o)
    assert bool((t.cpu()[~ok] >= last[~ok]).all())         # beyond the last cumulative weight: the last bin
    # Philox: deterministic, seed-dependent, distributed like the weights
    p1 = ops.sample_rays_weighted(rc, ijs.to(DEV), edges.to(DEV), w.to(DEV), seed=5)[1]
    p2 = ops.sample_rays_weighted(rc, ijs.to(DEV), edges.to(DEV), w.to(DEV), seed=5)[1]
    p3 = ops.sample_rays_weighted(rc, ijs.to(DEV), edges.to(DEV), w.to(DEV), seed=6)[1]
    assert torch.equal(p1, p2) and (S * B == 1 or not torch.equal(p1, p3))
    assert bool(((p1.cpu() >= edges[..., :1]) & (p1.cpu() <= edges[..., -1:])).all())
    # ... and pinned: sample e of ray r draws words 0 (bin) and 1 (offset) of Philox4x32-10 block (r S + e, stream 0) -- the host
    # generator (itself pinned to the Random123 vectors) reproduces the in-kernel draws bit for bit
    import numpy as np
    idx = np.arange(F * R * S, dtype=np.uint64)
    hb = torch.from_numpy(host_philox_uniform(5, 0, idx, 0, word=0)).view(F, R, S)
    ho = torch.from_numpy(host_philox_uniform(5, 0, idx, 0, word=1)).view(F, R, S)
    ph = ops.sample_rays_weighted(rc, ijs.to(DEV), edges.to(DEV), w.to(DEV), hb.to(DEV), ho.to(DEV))[1]
    assert torch.equal(ph, p1)
    if S >= 200:
        bins = (torch.searchsorted(edges[1:].contiguous(), p1.cpu()[1:].contiguous(), right=True) - 1).clamp(0, B - 1)
        hist = torch.zeros(F - 1, R, B).scatter_add_(-1, bins, torch.ones_like(p1.cpu()[1:])) / S
        assert float((hist - w[1:]).abs().max()) < 0.2


@pytest.mark.parametrize("n_c,n_g", [(24, 0), (7, 5), (64, 64), (1, 1)])
def test_sampler_vs_oracle_random(n_c, n_g):
    torch.manual_seed(n_c * 100 + n_g)
    F, R = 3, 37
    ijs = torch.stack([torch.randint(0, 480, (F, R)), torch.randint(0, 640, (F, R))], -1)
    near = torch.rand(F, R) * 2
    far = near + 0.5 + torch.rand(F, R) * 3
    far[0, 0] = near[0, 0]                                # degenerate segment (near == far)
    gt = near + (far - near) * torch.rand(F, R)
    gt[0, 1] = 0.0; gt[1, 2] = far[1, 2] + 1.0; gt[2, 3] = near[2, 3] * 0.5
    u_c, u_g = torch.rand(F, R, n_c), (torch.rand(F, R, n_g) if n_g else None)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g)
    pts_o, t_o, _ = O.sample_rays(ijs, NRGBD, near, far, gt if n_g else None, rs, u_c, u_g)
    rc = K.render_cfg(num_samples_coarse=n_c, num_samples_guided=n_g, **NRGBD_KW)
    pts, t, _ = ops.sample_rays(rc, ijs.to(DEV), near.to(DEV), far.to(DEV), gt.to(DEV) if n_g else None, u_c.to(DEV),
                                u_g.to(DEV) if n_g else None)
    assert torch.equal(t.cpu(), t_o)
    assert (t[..., 1:] >= t[..., :-1]).all()


def test_sampler_philox_statistics_and_reproducibility():
    F, R, n = 4, 256, 64
    rc = K.render_cfg(num_samples_coarse=n, num_samples_guided=0, **NRGBD_KW)
    ijs = torch.zeros(F, R, 2, dtype=torch.long, device=DEV)
    near, far = torch.zeros(F, R, device=DEV), torch.full((F, R), float(n), device=DEV)
    _, t1, _ = ops.sample_rays(rc, ijs, near, far, seed=7)
    _, t2, _ = ops.sample_rays(rc, ijs, near, far, seed=7)
    _, t3, _ = ops.sample_rays(rc, ijs, near, far, seed=8)
    assert torch.equal(t1, t2) and not torch.equal(t1, t3)
    u = t1 - torch.arange(n, device=DEV)                  # delta = 1 -> jitter in [0,1)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 + 1e-5
    assert abs(float(u.mean()) - 0.5) < 0.01 and abs(float(u.var()) - 1 / 12) < 0.005


# ------------------------------------------------------------------------- field evaluation (G4)
@pytest.mark.parametrize("enc", ["fourier", "nerf"])
def test_field_forward_golden(enc):
    g = load_golden(f"g4_field_forward_{enc}")
    fc = K.field_cfg(encoding=enc, dim_enc=64, num_layers=2, num_octaves=8)
    params = cu({k: v for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"})
    out = ops.field_eval(fc, params, g["query"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV))
    close(out, g["out"], rtol=2e-4, atol=3e-5)


@pytest.mark.parametrize("name", ["g12_skip_add_D64", "g12_skip_add_D61"])
def test_skip_add_golden(name):
    """skip_mode "add" (models.py:162-169) against the reference: forward and every parameter gradient.
    D61: dim_enc 61 < dim_hidden 64, only the first 61 units receive the encoding."""
    g = load_golden(name)
    D = int(name.split("D")[-1])
    fc = K.field_cfg(encoding="fourier", dim_enc=D, dim_hidden=int(g["dim_hidden"]), num_layers=2, skip_mode="add")
    params = {k: v.to(DEV).requires_grad_() for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"}
    out = ops.field_eval(fc, params, g["query"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV))
    close(out, g["out"], rtol=2e-4, atol=3e-5)
    (out * g["seed"].to(DEV)).sum().backward()
    from neural_graph_mapping_amd import _capi
    assert _capi.lib().ngm_debug_last_bwd_variant() == 0          # skip connections run on the 32-sample-tile kernel
    for k, gr in split_prefix(g, "g::").items():
        grad_close(params[k].grad, gr, 2e-3, k)


@pytest.mark.parametrize("name", ["g12_skip_concat_D32", "g12_skip_concat_D64"])
def test_skip_concat_golden(name):
    """skip_mode "concat" (models.py:159-161) against the reference: every layer after the first and the output layer
    read cat(hidden, encoding) -- "_linears.{i}.weight" is (out, H + D) for i >= 1.  Forward and every gradient."""
    g = load_golden(name)
    D = int(name.split("D")[-1])
    fc = K.field_cfg(encoding="fourier", dim_enc=D, dim_hidden=int(g["dim_hidden"]), num_layers=2, skip_mode="concat")
    assert K.param_shapes(fc)["_linears.1.weight"] == tuple(g["p::_linears.1.weight"].shape[1:])
    params = {k: v.to(DEV).requires_grad_() for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"}
    out = ops.field_eval(fc, params, g["query"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV))
    close(out, g["out"], rtol=2e-4, atol=3e-5)
    (out * g["seed"].to(DEV)).sum().backward()
    assert K.lib().ngm_debug_last_bwd_variant() == 0              # skip connections run on the 32-sample-tile kernel
    for k, gr in split_prefix(g, "g::").items():
        grad_close(params[k].grad, gr, 2e-3, k)
    # the kNN-blended evaluation path uses the same weights (one field, every point inside it: blend weight 1)
    pts = g["pos"][:1] + 0.4 * (torch.rand(200, 3) - 0.5)
    one = {k: v[:1].detach() for k, v in params.items()}
    a = ops.field_eval_knn(fc, one, pts.to(DEV), g["pos"][:1].to(DEV), g["quat"][:1].to(DEV), 1, 10.0, 1.0)
    b = ops.field_eval(fc, one, pts[None].to(DEV), g["pos"][:1].to(DEV), g["quat"][:1].to(DEV))[0]
    close(a, b, rtol=1e-5, atol=1e-6)


def test_non_unit_quaternions_scale_the_local_frame_like_the_reference():
    """`quaternion_apply(quaternion_invert(q), .)` (models.py:338-339, 377-379) is two raw Hamilton products: for |q| != 1
    the local coordinates come out scaled by |q|^2 -- the reference never normalises, and neither do the kernels (standalone
    evaluation, kNN evaluation, the fused training step's ray set-up).  Against the oracle's restatement of the raw products."""
    torch.manual_seed(12)
    F, P = 3, 600
    norms = torch.tensor([0.85, 1.0, 1.2])
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    fs = O.FieldSpec(**fkw)
    params = O.init_params(fs, F, seed=5, sigma=3.0)
    pos = torch.randn(F, 3)
    unit = torch.nn.functional.normalize(torch.randn(F, 4), dim=-1)
    quat = unit * norms[:, None]
    q = pos[:, None, :] + 0.35 * torch.randn(F, P, 3)
    fc = K.field_cfg(field_radius=1.0, **fkw)
    ref = O.field_set_forward_vmap(q, pos, quat, params, fs, radius=1.0)
    out = ops.field_eval(fc, cu(params), q.to(DEV), pos.to(DEV), quat.to(DEV))
    close(out, ref, rtol=2e-4, atol=3e-5)
    normalised = O.field_set_forward_vmap(q, pos, unit, params, fs, radius=1.0)
    assert float((normalised[0] - ref[0]).abs().max()) > 1e-2 and float((normalised[1] - ref[1]).abs().max()) < 1e-4
    pts = q.reshape(-1, 3)
    ref_k = O.field_set_forward_knn(pts, pos, quat, params, fs, radius=1.0)
    out_k = ops.field_eval_knn(fc, cu(params), pts.to(DEV), pos.to(DEV), quat.to(DEV), 2, 10.0, 1.0)
    close(out_k, ref_k, rtol=2e-4, atol=3e-5)
    # the fused training step: rays set up in the (scaled) local frame
    R, n_c, n_g = 40, 8, 8
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    pos2, quat2, t = synth_target(F, R, seed=6)
    quat2 = quat2 * norms[:, None]
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    params[f"_linears.2.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos2, quat2, params, fs, rs, u_c, u_g)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos2, quat2, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    r = make_renderer(fkw, ckw, F, params)
    r.set_field_poses(pos2.to(DEV), quat2.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    close(res["combined"], loss["combined"].detach(), rtol=3e-4, atol=1e-6)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)


@pytest.mark.parametrize("D,layers", [(64, 2), (32, 1), (61, 2)])
def test_skip_concat_fused_train_step_vs_oracle(D, layers):
    """skip_mode "concat" through the fused render / train step (forward kernel + 32-sample-tile backward)."""
    F, R, n_c, n_g = 2, 33, 6, 10
    torch.manual_seed(8)
    fkw = dict(encoding="fourier", dim_enc=D, num_layers=layers, skip_mode="concat")
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    pos, quat, t = synth_target(F, R, seed=4)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    params = O.init_params(fs, F, seed=11, sigma=3.0)
    params[f"_linears.{layers}.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    r = make_renderer(fkw, ckw, F, params)
    assert r._model.all_fields_params[f"_linears.{layers}.weight"].shape[-1] == 2 * D       # H + D inputs (H = D here)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    close(res["combined"], loss["combined"].detach(), rtol=3e-4, atol=1e-6)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)
    out = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=True)   # fused Adam
    assert torch.isfinite(out["combined"])


def test_skip_add_fused_train_step_vs_oracle():
    """skip_mode "add" through the fused render / train step."""
    F, R, n_c, n_g = 2, 33, 6, 10
    torch.manual_seed(8)
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2, skip_mode="add")
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    pos, quat, t = synth_target(F, R, seed=4)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    params = O.init_params(fs, F, seed=11, sigma=3.0)
    params["_linears.2.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    r = make_renderer(fkw, ckw, F, params)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    close(res["combined"], loss["combined"].detach(), rtol=3e-4, atol=1e-6)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)


FIELD_CASES = [dict(encoding="fourier", dim_enc=64, num_layers=2), dict(encoding="fourier", dim_enc=32, num_layers=2),
               dict(encoding="fourier", dim_enc=32, num_layers=1), dict(encoding="nerf", num_octaves=8, num_layers=1),
               dict(encoding="fourier", dim_enc=64, num_layers=1, raw_coords=False),
               dict(encoding="nerf", num_octaves=4, num_layers=2)]


@pytest.mark.parametrize("kw", FIELD_CASES)
@pytest.mark.parametrize("P", [1, 257])
def test_field_eval_forward_backward_vs_oracle(kw, P):
    torch.manual_seed(3)
    F = 3
    fs = O.FieldSpec(**kw)
    fc = K.field_cfg(**kw)
    params = O.init_params(fs, F, seed=5, sigma=3.0)
    pos, quat = torch.randn(F, 3), torch.nn.functional.normalize(torch.randn(F, 4), dim=-1)
    q = away_from_relu_boundaries(pos[:, None] + 0.5 * torch.randn(F, P, 3), pos, quat, params, fs)
    d_out = torch.randn(F, P, 4)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    out_o = O.field_set_forward_vmap(q, pos, quat, po, fs)
    (out_o * d_out).sum().backward()
    pg = {k: v.to(DEV).requires_grad_() for k, v in params.items()}
    out = ops.field_eval(fc, pg, q.to(DEV), pos.to(DEV), quat.to(DEV))
    tol = 2e-4 if kw["encoding"] == "fourier" else 2e-3        # octave encoding amplifies fp32 argument error
    close(out, out_o.detach(), rtol=tol, atol=tol * 0.2)
    (out * d_out.to(DEV)).sum().backward()
    for k in po:
        grad_close(pg[k].grad, po[k].grad, 2e-3, k)              # NeRF octaves too (measured <= 3.4e-4; was 1e-2)


@pytest.mark.parametrize("kw,P,posed", [(dict(encoding="fourier", dim_enc=64, num_layers=2), 4133, True),
                                        (dict(encoding="fourier", dim_enc=64, num_layers=2), 31, False),
                                        (dict(encoding="fourier", dim_enc=64, num_layers=1, raw_coords=False), 1000, True),
                                        (dict(encoding="nerf", num_octaves=9, num_layers=2), 777, True),
                                        (dict(encoding="fourier", dim_enc=50, num_layers=2, dim_hidden=60), 515, True)])
def test_field_eval_training_pair_with_activation_stash(kw, P, posed):
    """ABI 11: under autograd the point evaluation writes the activation stash (ngm_field_eval_fwd_train) and its backward is the
    fused step's MLP backward in point mode (ngm_field_eval_bwd_stash -> k_field_bwd_b3).  Same outputs as the plain forward bit
    for bit; gradients against the oracle at the usual 2e-3 bar and against the recomputing backward; bitwise repeatable; fields
    that start in the middle of a 32-sample stash tile (P not a multiple of 32); mlp_matmul f32 keeps the recomputing pair."""
    torch.manual_seed(11)
    F = 3
    fs = O.FieldSpec(**kw)
    fc = K.field_cfg(**kw, matmul_mode="auto")
    assert K.lib().ngm_field_eval_stash_bytes(K.C.byref(fc), F, P) >= F * P * 256 * kw["num_layers"]
    assert K.lib().ngm_field_eval_stash_bytes(K.C.byref(K.field_cfg(**kw)), F, P) == 0            # mlp_matmul f32: no stash-reading backward
    params = O.init_params(fs, F, seed=5, sigma=3.0)
    pos, quat = torch.randn(F, 3), torch.nn.functional.normalize(torch.randn(F, 4), dim=-1)
    if not posed:
        pos, quat = torch.zeros(F, 3), torch.tensor([[1.0, 0.0, 0.0, 0.0]]).repeat(F, 1)
    q = away_from_relu_boundaries(pos[:, None] + 0.5 * torch.randn(F, P, 3), pos, quat, params, fs)
    d_out = torch.randn(F, P, 4)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    out_o = O.field_set_forward_vmap(q, pos, quat, po, fs)
    (out_o * d_out).sum().backward()
    pose = (pos.to(DEV), quat.to(DEV)) if posed else (None, None)
    with torch.no_grad():
        plain = ops.field_eval(fc, cu(params), q.to(DEV), *pose)
    runs = []
    for _ in range(2):
        pg = {k: v.to(DEV).requires_grad_() for k, v in params.items()}
        out = ops.field_eval(fc, pg, q.to(DEV), *pose)
        assert torch.equal(out, plain)
        (out * d_out.to(DEV)).sum().backward()
        assert K.lib().ngm_debug_last_bwd_variant() == 3
        runs.append({k: v.grad.clone() for k, v in pg.items()})
    for k in po:
        grad_close(runs[0][k], po[k].grad, 2e-3, k)
        assert torch.equal(runs[0][k], runs[1][k]), k
    # the recomputing backward (no stash kept) on the same inputs
    keep = ops.FIELD_EVAL_STASH_MAX_BYTES
    ops.FIELD_EVAL_STASH_MAX_BYTES = 0
    try:
        pg = {k: v.to(DEV).requires_grad_() for k, v in params.items()}
        out = ops.field_eval(fc, pg, q.to(DEV), *pose)
        (out * d_out.to(DEV)).sum().backward()
        assert K.lib().ngm_debug_last_bwd_variant() != 3
    finally:
        ops.FIELD_EVAL_STASH_MAX_BYTES = keep
    for k in po:
        grad_close(pg[k].grad, runs[0][k], 2e-3, k)


def test_neural_field_set_module_matches_oracle():
    torch.manual_seed(0)
    fs = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=64, mu=0.0, sigma=4.0, raw_coords=True), num_layers=2, dim_out=4),
        num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=1.0, scale_mode="unit_cube").to(DEV)
    fs.add_fields(4)
    ids = torch.tensor([3, 1], device=DEV)
    fs.set_vmap_fields(ids)
    pos, quat = torch.randn(2, 3), torch.nn.functional.normalize(torch.randn(2, 4), dim=-1)
    q = pos[:, None] + 0.4 * torch.randn(2, 50, 3)
    out = fs(q.to(DEV), pos.to(DEV), quat.to(DEV), ids, True)
    ospec = O.FieldSpec(encoding="fourier", dim_enc=64, num_layers=2)
    pcpu = {k: v.cpu() for k, v in fs.vmap_fields_params.items() if k != "_neus_sd"}
    close(out, O.field_set_forward_vmap(q, pos, quat, pcpu, ospec))


def _g21_module(g, **kw):
    r = float(g["radius"])
    fs = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=64, mu=0.0, sigma=4.0, raw_coords=True), num_layers=2, dim_out=4,
        neus_initial_sd=1.0), num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=r, scale_mode="unit_cube",
        **kw).to(DEV)
    fs.add_fields(g["pos"].shape[0])
    for k, v in split_prefix(g, "p::").items():
        fs.all_fields_params[k].copy_(v.to(DEV))
    fs.refresh_lp()
    return fs


def test_module_forward_field_radius_argument_golden():
    """Boundary row (b): `NeuralFieldSet.forward(field_radius=...)` through the drop-in CLASS (not the op): fixture G21 from
    the real reference, called as run_mapping.py:2320-2332 calls it.  The argument widens the inside test of the kNN branch
    only (models.py:368); the scaling keeps the constructor's radius (models.py:278-285); the vmap branch ignores it."""
    g = load_golden("g21_field_radius_override")
    fs = _g21_module(g)
    mr = float(g["mask_radius"])
    pts, pos, quat = g["points"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV)
    out = fs(pts, pos, quat, None, use_vmap=False, field_radius=mr)
    close(out, g["out_knn"], rtol=2e-4, atol=3e-5)
    out_d = fs(pts, pos, quat, None, use_vmap=False)
    close(out_d, g["out_knn_default"], rtol=2e-4, atol=3e-5)
    shell = (g["out_knn"] != g["out_knn_default"]).any(-1)
    assert int(shell.sum()) > 60 and bool((out.cpu()[shell] != 1.0).any(-1).all())      # shell points ARE evaluated
    assert torch.equal(out_d.cpu()[shell], torch.ones(int(shell.sum()), 4))             # ... and are not without it
    # leading dims are restored, field_ids maps slots to parameter rows (models.py:347-349, 395)
    perm = torch.tensor([2, 0, 3, 1])
    fs2 = _g21_module(g)
    for k in fs2.all_fields_params:
        fs2.all_fields_params[k][perm] = fs.all_fields_params[k].clone()
    out_p = fs2(pts.view(4, -1, 3), pos, quat, perm.to(DEV), use_vmap=False, field_radius=mr)
    assert out_p.shape == (4, pts.shape[0] // 4, 4)
    assert torch.equal(out_p.reshape(-1, 4), out)
    ids = g["vmap_ids"].long().to(DEV)
    fs.set_vmap_fields(ids)
    q = g["query"].to(DEV)
    out_v = fs(q, pos[ids], quat[ids], ids, use_vmap=True, field_radius=mr)
    close(out_v, g["out_vmap"], rtol=2e-4, atol=2e-5)
    assert torch.equal(out_v, fs(q, pos[ids], quat[ids], ids, use_vmap=True))           # bitwise: the argument is unread


def _g22_module(g, enc):
    et = "PositionalEncodingFourier" if enc == "fourier" else "PositionalEncodingNeRF"
    ek = dict(dim_in=2, dim_out=40, mu=0.0, sigma=4.0, raw_coords=True) if enc == "fourier" else dict(dim_in=2, num_octaves=6, start_octave=0)
    fs = M.NeuralFieldSet(dim_points=2, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings." + et, encoding_kwargs=ek, num_layers=2, dim_out=4,
        dim_mlp_out=64, skip_mode="no"), num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=float(g["radius"]),
        scale_mode="unit_cube").to(DEV)
    fs.add_fields(g["pos"].shape[0])
    for k, v in split_prefix(g, "p::").items():
        assert fs.all_fields_params[k].shape == v.shape, k          # the 2-D parameter shapes ARE the reference's
        fs.all_fields_params[k].copy_(v.to(DEV))
    return fs


@pytest.mark.parametrize("enc", ["fourier", "nerf"])
def test_module_forward_planar_field_set_golden(enc):
    """`NeuralFieldSet(dim_points=2)` (models.py:236-238): fixture G22 from the real reference (complex orientations, two
    of non-unit modulus, one on the square root's branch cut) through the drop-in class, both branches of `forward` and
    the already-local call; the kernels see the z = 0 embedding (`models.Embed2D`)."""
    g = load_golden(f"g22_fields_2d_{enc}")
    fs = _g22_module(g, enc)
    pts, pos, comp = g["points"].to(DEV), g["pos"].to(DEV), g["comp"].to(DEV)
    out = fs(pts, pos, comp, None, use_vmap=False)
    close(out, g["out_knn"], rtol=2e-4, atol=3e-5)
    outside = (g["out_knn"] == 1.0).all(-1)
    assert int(outside.sum()) > 30 and torch.equal(out.cpu()[outside], torch.ones(int(outside.sum()), 4))
    assert fs(pts.view(3, -1, 2), pos, comp, None, use_vmap=False).shape == (3, pts.shape[0] // 3, 4)
    ids = g["vmap_ids"].long().to(DEV)
    fs.set_vmap_fields(ids)
    q = g["query"].to(DEV)
    close(fs(q, pos[ids], comp[ids], ids, use_vmap=True), g["out_vmap"], rtol=2e-4, atol=2e-5)
    close(fs(q, None, None, ids, use_vmap=True), g["out_local"], rtol=2e-4, atol=2e-5)
    # one field through the prototype class (models.py:143-182 with a 2-D encoding)
    proto = fs._prototype_field.to(DEV)
    sd = {k: v[0] for k, v in fs.vmap_fields_params.items()}
    proto.load_state_dict(sd)
    x_local = q[0] / (2 * float(g["radius"])) + 0.5
    close(proto(x_local), fs(q[:1], None, None, ids[:1], use_vmap=True)[0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("enc", ["fourier", "nerf"])
def test_module_planar_field_set_gradients_vs_oracle(enc):
    """autograd through the planar set: gradients of every 2-D parameter against the oracle's native 2-D restatement
    (float64 autograd); the zero blocks of the embedding take no part"""
    g = load_golden(f"g22_fields_2d_{enc}")
    fs = _g22_module(g, enc)
    ids = g["vmap_ids"].long()
    fs.set_vmap_fields(ids.to(DEV))
    leaves = {k: v.clone().requires_grad_(True) for k, v in fs.vmap_fields_params.items()}
    fs.vmap_fields_params = leaves
    q, pos, comp = g["query"].to(DEV), g["pos"][ids].to(DEV), g["comp"][ids].to(DEV)
    wgt = torch.randn(3, 50, 4, generator=torch.Generator().manual_seed(5))
    (fs(q, pos, comp, ids.to(DEV), use_vmap=True) * wgt.to(DEV)).sum().backward()
    fs2 = (O.FieldSpec(encoding="fourier", dim_enc=40, num_layers=2, dim_hidden=64) if enc == "fourier"
           else O.FieldSpec(encoding="nerf", num_octaves=6, num_layers=2, dim_hidden=64))
    po = {k: v[ids].double().requires_grad_(True) for k, v in split_prefix(g, "p::").items()}
    (O.field_set_forward_vmap(g["query"].double(), g["pos"][ids].double(), g["comp"][ids].double(), po, fs2,
                              radius=float(g["radius"])) * wgt.double()).sum().backward()
    for k, v in po.items():
        assert leaves[k].grad is not None and leaves[k].grad.shape == v.shape, k
        ref = v.grad.float()
        err = float((leaves[k].grad.cpu() - ref).abs().max())
        assert err <= 2e-3 * float(ref.abs().max()) + 1e-6, (k, err, float(ref.abs().max()))


@pytest.mark.parametrize("scale_mode,r", [("unit_cube", 0.7), ("unit_ball", 1.3), ("no", 0.9)])
def test_module_forward_field_radius_argument_vs_oracle(scale_mode, r):
    """the same contract against the oracle with separate scale / mask radii, every scale mode, 30 fields, K = 2"""
    torch.manual_seed(7)
    NF, P = 30, 20000
    fs = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=32, mu=0.0, sigma=3.0, raw_coords=True), num_layers=1, dim_out=4),
        num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=r, scale_mode=scale_mode).to(DEV)
    fs.add_fields(NF)
    ospec = O.FieldSpec(encoding="fourier", dim_enc=32, num_layers=1)
    params = O.init_params(ospec, NF, seed=3, sigma=3.0)
    for k, v in params.items():
        fs.all_fields_params[k].copy_(v.to(DEV))
    pos = torch.rand(NF, 3) * 4
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1)
    pts = torch.rand(P, 3) * 5 - 0.5
    for mr in (r + 0.1, 0.5 * r, None):
        ref = O.field_set_forward_knn(pts, pos, quat, params, ospec, radius=r, scale_mode=scale_mode, mask_radius=mr)
        out = fs(pts.to(DEV), pos.to(DEV), quat.to(DEV), None, use_vmap=False, field_radius=mr)
        close(out, ref, rtol=3e-4, atol=3e-5)
    ids = torch.tensor([5, 17, 2])
    fs.set_vmap_fields(ids.to(DEV))
    q = pos[ids][:, None] + 0.4 * r * torch.randn(3, 333, 3)
    ref = O.field_set_forward_vmap(q, pos[ids], quat[ids], {k: v[ids] for k, v in params.items()}, ospec, radius=r,
                                   scale_mode=scale_mode)
    out = fs(q.to(DEV), pos[ids].to(DEV), quat[ids].to(DEV), ids.to(DEV), use_vmap=True, field_radius=r + 0.1)
    close(out, ref, rtol=3e-4, atol=3e-5)


# ------------------------------------------------------------------------------ quadrature (G5)
@pytest.mark.parametrize("mode", ["nrgbd", "occupancy", "density", "neus"])
@pytest.mark.parametrize("S", [2, 24, 128])
def test_quadrature_golden(mode, S):
    g = load_golden(f"g5_quadrature_{mode}_S{S}")
    rc = K.render_cfg(geometry_mode=mode, geometry_factor=float(g["geometry_factor"]))
    isds = g["isds"].to(DEV) if "isds" in g else None
    C_, D, Cv, Dv, term, w = ops.quadrature(rc, g["colors"].to(DEV), g["geoms"].to(DEV), g["dists"].to(DEV),
                                            g["depths"].to(DEV), isds)
    for a, b in ((C_, "C"), (D, "D"), (Cv, "Cv"), (Dv, "Dv"), (term, "term"), (w, "w")):
        close(a, g[b], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("mode", ["nrgbd", "occupancy"])
@pytest.mark.parametrize("lead,S", [((3, 5), 24), ((7,), 128), ((2, 3), 1), ((1,), 200), ((40,), 7),
                                    ((5,), 64), ((300,), 192), ((3,), 512), ((2,), 576)])      # 64 | S <= 512: the whole-ray kernels
def test_quadrature_backward_vs_oracle(mode, lead, S):
    torch.manual_seed(S)
    colors = torch.rand(*lead, S, 3)
    geoms = 0.1 * torch.randn(*lead, S)
    geoms.view(-1)[0] = 0.0                          # occ == 1 exactly: division-free recursion must be exact
    if S > 3:
        geoms.view(-1, S)[0, 3] = 0.0
    dists = torch.sort(torch.rand(*lead, S) * 3 + 0.5, -1)[0]
    depths = dists * 0.9
    dC, dD, dT = torch.randn(*lead, 3), torch.randn(*lead), torch.randn(*lead)
    co, go = colors.clone().requires_grad_(), geoms.clone().requires_grad_()
    outs_o = O.quadrature(mode, co, go, dists, depths, 20.0)
    Co, Do, _, _, To, _ = outs_o
    ((Co * dC).sum() + (Do * dD).sum() + (To * dT).sum()).backward()
    rc = K.render_cfg(geometry_mode=mode, geometry_factor=20.0)
    cg, gg = colors.to(DEV).requires_grad_(), geoms.to(DEV).requires_grad_()
    outs_g = ops.quadrature(rc, cg, gg, dists.to(DEV), depths.to(DEV))
    Cg, Dg, _, _, Tg, _ = outs_g
    for a, b in zip(outs_g, outs_o):                 # colour, depth, both variances, termination probability, weights
        close(a.detach(), b.detach(), 1e-5, 2e-6)
    ((Cg * dC.to(DEV)).sum() + (Dg * dD.to(DEV)).sum() + (Tg * dT.to(DEV)).sum()).backward()
    grad_close(cg.grad, co.grad, 1e-5, "d_colors")
    grad_close(gg.grad, go.grad, 2e-5, "d_geoms")


@pytest.mark.parametrize("mode", ["density", "neus"])
@pytest.mark.parametrize("lead,S", [((3, 5), 24), ((7,), 128), ((2, 3), 2), ((1,), 200), ((40,), 7)])
def test_quadrature_backward_neighbour_modes_vs_oracle(mode, lead, S):
    """density / neus (rm.py:746-758): occ_k depends on the next sample; neus also on the per-ray inverse
    standard deviation.  Gradients w.r.t. colours, geometry and neus_isds against torch autograd on the oracle."""
    torch.manual_seed(S + len(mode))
    colors = torch.rand(*lead, S, 3)
    geoms = (torch.randn(*lead, S) if mode == "density" else 0.05 * torch.randn(*lead, S).cumsum(-1).flip(-1))
    dists = torch.sort(torch.rand(*lead, S) * 3 + 0.5, -1)[0]
    depths = dists * 0.9
    isds = (0.5 + torch.rand(*lead, 1)) if mode == "neus" else None
    dC, dD, dT = torch.randn(*lead, 3), torch.randn(*lead), torch.randn(*lead)
    co, go = colors.clone().requires_grad_(), geoms.clone().requires_grad_()
    io = isds.clone().requires_grad_() if isds is not None else None
    outs_o = O.quadrature(mode, co, go, dists, depths, 20.0, io)
    Co, Do, _, _, To, _ = outs_o
    ((Co * dC).sum() + (Do * dD).sum() + (To * dT).sum()).backward()
    rc = K.render_cfg(geometry_mode=mode, geometry_factor=20.0)
    cg, gg = colors.to(DEV).requires_grad_(), geoms.to(DEV).requires_grad_()
    ig = isds.to(DEV).requires_grad_() if isds is not None else None
    outs_g = ops.quadrature(rc, cg, gg, dists.to(DEV), depths.to(DEV), ig)
    Cg, Dg, _, _, Tg, _ = outs_g
    for a, b in zip(outs_g, outs_o):                 # colour, depth, both variances, termination probability, weights
        close(a.detach(), b.detach(), 1e-5, 2e-6)
    ((Cg * dC.to(DEV)).sum() + (Dg * dD.to(DEV)).sum() + (Tg * dT.to(DEV)).sum()).backward()
    grad_close(cg.grad, co.grad, 1e-5, "d_colors")
    grad_close(gg.grad, go.grad, 5e-5, "d_geoms")
    if ig is not None:
        assert ig.grad.shape == isds.shape
        grad_close(ig.grad, io.grad, 1e-4, "d_isds")


def test_fused_train_step_density_mode_vs_oracle():
    """geometry_mode = density in the fused forward / backward (occ_k needs t_{k+1}; last sample dropped)."""
    F, R, n_c, n_g = 3, 40, 10, 6
    torch.manual_seed(5)
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode="density",
               geometry_factor=1.0)
    pos, quat, t = synth_target(F, R, seed=3)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3,
                      geometry_mode="density", geometry_factor=1.0)
    params = O.init_params(fs, F, seed=9, sigma=3.0)
    params["_linears.2.weight"] *= 4.0
    params["_linears.2.bias"][:, 3] += 1.0           # positive densities on a good share of the samples
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    r = make_renderer(fkw, ckw, F, params)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    close(res["prediction"].term_probs, pred["term_probs"].detach())
    close(res["prediction"].depth_vars, pred["depth_vars"].detach(), rtol=1e-3, atol=1e-5)
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    close(res["combined"], loss["combined"].detach(), rtol=3e-4, atol=1e-6)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)


def test_neus_staged_train_step_vs_oracle():
    """geometry_mode = neus (rm.py:641-644, 753-758): rendered through the staged path (sampler -> field evaluation ->
    quadrature kernels under autograd); prediction, loss and every gradient incl. the per-field `_neus_sd`; then one
    sparse-Adam update must move `_neus_sd` of the trained fields only."""
    F, R, n_c, n_g = 3, 40, 10, 6
    torch.manual_seed(7)
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode="neus",
               geometry_factor=5.0)
    pos, quat, t = synth_target(F, R, seed=4)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3,
                      geometry_mode="neus", geometry_factor=5.0)
    params = O.init_params(fs, F, seed=11, sigma=3.0)
    params["_linears.2.weight"] *= 3.0
    sd = torch.tensor([0.4, 0.8, 1.5])
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g, neus_isds=1.0 / sd.abs())
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    sdo = sd.clone().requires_grad_()
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g,
                        neus_isds=1.0 / sdo.abs().view(-1, 1, 1))
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    loss["combined"].backward()
    r = make_renderer(fkw, ckw, F + 1, None)                        # one extra field that is never trained
    with torch.no_grad():
        for k, v in params.items():
            r._model.all_fields_params[k][:F].copy_(v.to(DEV))
        r._model.all_fields_params["_neus_sd"][:F].copy_(sd.to(DEV))
    r.set_field_poses(torch.cat([pos, torch.zeros(1, 3)]).to(DEV), torch.cat([quat, torch.tensor([[1.0, 0, 0, 0]])]).to(DEV))
    tgt = make_target(t, torch.arange(F))
    res = r.optimization_iteration_staged(tgt, u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    close(res["prediction"].term_probs, pred["term_probs"].detach())
    close(res["combined"], loss["combined"].detach(), rtol=3e-4, atol=1e-6)
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)
    close(res["grads"]["_neus_sd"].view(-1), sdo.grad, rtol=5e-3, atol=1e-6)
    before = r._model.all_fields_params["_neus_sd"].clone()
    r.optimization_iteration_staged(tgt, u_c.to(DEV), u_g.to(DEV), update=True)
    after = r._model.all_fields_params["_neus_sd"]
    assert bool((after[:F] != before[:F]).all()) and bool(after[F] == before[F])
    # optimization_iteration dispatches to the staged path for this mode
    res2 = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=False)
    assert torch.isfinite(res2["combined"]) and "_neus_sd" in res2["grads"]


@pytest.mark.parametrize("F,R,n_c,n_g,layers", [(3, 40, 10, 6, 2), (2, 33, 1, 1, 1), (1, 5, 64, 64, 2), (4, 130, 20, 4, 2)])
def test_neus_fused_train_step_vs_oracle(F, R, n_c, n_g, layers):
    """geometry_mode = neus inside the FUSED kernels (rm.py:641-644, 753-758): occ_k depends on the geometry of samples k
    and k + 1 and on the per-field learnable `_neus_sd`.  Forward: compositing as a second pass over the wave's LDS
    planes; backward: neighbour terms rebuilt from the stash, d loss / d _neus_sd reduced per field.  Prediction, loss,
    every gradient incl. `_neus_sd` against the oracle; the fused update moves `_neus_sd` of the trained fields only; the
    iteration is capturable (device-side counters)."""
    torch.manual_seed(7 + F)
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=layers)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode="neus",
               geometry_factor=5.0)
    pos, quat, t = synth_target(F, R, seed=4)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3,
                      geometry_mode="neus", geometry_factor=5.0)
    params = O.init_params(fs, F, seed=11, sigma=3.0)
    params[f"_linears.{layers}.weight"] *= 3.0
    sd = torch.tensor([0.4, 0.8, -1.5, 1.1])[:F]                      # a negative one: isd = 1 / |sd| (rm.py:641-644)
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g, neus_isds=1.0 / sd.abs())
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    sdo = sd.clone().requires_grad_()
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g,
                        neus_isds=1.0 / sdo.abs().view(-1, 1, 1))
    r = make_renderer(fkw, ckw, F + 1, None)                        # one extra field that is never trained
    with torch.no_grad():
        for k, v in params.items():
            r._model.all_fields_params[k][:F].copy_(v.to(DEV))
        r._model.all_fields_params["_neus_sd"][:F].copy_(sd.to(DEV))
    r.set_field_poses(torch.cat([pos, torch.zeros(1, 3)]).to(DEV), torch.cat([quat, torch.tensor([[1.0, 0, 0, 0]])]).to(DEV))
    assert r._neus_fused()
    tgt = make_target(t, torch.arange(F))
    res = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    close(res["prediction"].term_probs, pred["term_probs"].detach())
    close(res["prediction"].depth_vars, pred["depth_vars"].detach(), rtol=1e-3, atol=1e-5)
    loss, _ = compare_losses(res, pred, t, rs)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)
    grad_close(res["grads"]["_neus_sd"].view(-1), sdo.grad, 2e-3, "_neus_sd")
    again = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=False)          # deterministic
    assert torch.equal(again["grads"]["_neus_sd"], res["grads"]["_neus_sd"]) and torch.equal(
        again["grads"]["_linears.0.weight"], res["grads"]["_linears.0.weight"])
    before = r._model.all_fields_params["_neus_sd"].clone()
    replay = r.capture_iteration(tgt, u_coarse=u_c.to(DEV), u_guided=u_g.to(DEV))       # 2 warm-up updates + capture
    replay()
    torch.cuda.synchronize()
    after = r._model.all_fields_params["_neus_sd"]
    assert bool((after[:F] != before[:F]).all()) and bool(after[F] == before[F]) and r._step == 3


@pytest.mark.parametrize("seed", list(range(int(os.environ.get("NGM_FUZZ_SEEDS_NEUS", "5")))))      # NGM_FUZZ_SEEDS_NEUS=200: a longer sweep
def test_neus_fused_train_random_shapes_vs_oracle(seed):
    """geometry_mode = neus on random batch shapes, sample counts (incl. S = 2), layer counts, per-field standard deviations of
    either sign: prediction, loss and every gradient incl. `_neus_sd` against the oracle; the clamp's kinks are kept out of the
    comparison by kink_free_draws."""
    g = torch.Generator().manual_seed(9000 + seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))
    F, R, n_c, n_g, layers = ri(1, 5), ri(1, 80), ri(1, 20), ri(1, 20), ri(1, 2)
    torch.manual_seed(seed)
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=layers)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode="neus", geometry_factor=5.0)
    pos, quat, t = synth_target(F, R, seed=seed)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode="neus",
                      geometry_factor=5.0)
    params = O.init_params(fs, F, seed=seed, sigma=3.0)
    params[f"_linears.{layers}.weight"] *= 3.0
    sd = (0.3 + 1.5 * torch.rand(F, generator=g)) * torch.where(torch.rand(F, generator=g) < 0.3, -1.0, 1.0)
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g, neus_isds=1.0 / sd.abs(), max_neutralised=0.5)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    sdo = sd.clone().requires_grad_()
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g,
                        neus_isds=1.0 / sdo.abs().view(-1, 1, 1))
    r = make_renderer(fkw, ckw, F, None)
    with torch.no_grad():
        for k, v in params.items():
            r._model.all_fields_params[k].copy_(v.to(DEV))
        r._model.all_fields_params["_neus_sd"].copy_(sd.to(DEV))
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    close(res["prediction"].term_probs, pred["term_probs"].detach())
    loss, _ = compare_losses(res, pred, t, rs)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)
    grad_close(res["grads"]["_neus_sd"].view(-1), sdo.grad, 2e-3, "_neus_sd")


# ------------------------------------------------------------------------- triplane encoding (G15)
@pytest.mark.parametrize("name", ["g15_triplane_sum_C32", "g15_triplane_product_C32", "g15_triplane_concat_C20",
                                  "g15_triplane_sum_C64"])
def test_triplane_golden(name):
    """TriplaneEncoding (positional_encodings.py:69-161; pure torch in the reference, so this one IS pinned): vmapped
    field forward and every gradient incl. the feature planes, points inside and outside [-1,1]^3 (border padding)."""
    g = load_golden(name)
    mode, comps = name.split("_")[2], int(name.split("_C")[-1])
    fc = K.field_cfg(encoding="triplane", resolution=int(g["resolution"]), num_components=comps, tri_mode=mode, num_layers=1,
                     scale_mode="unit_ball")
    params = {k: v.to(DEV).requires_grad_() for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"}
    out = ops.field_eval(fc, params, g["query"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV))
    close(out, g["out"], rtol=2e-4, atol=3e-5)
    (out * g["seed"].to(DEV)).sum().backward()
    for k, gr in split_prefix(g, "g::").items():
        grad_close(params[k].grad, gr, 2e-3, k)
    untouched = split_prefix(g, "g::")["_encoding.plane_coef"] == 0          # texels no sample reaches: exactly zero
    assert bool((params["_encoding.plane_coef"].grad.cpu()[untouched] == 0).all())
    # kNN-blended evaluation path, one field, every point inside it
    pts = g["pos"][:1] + 0.4 * (torch.rand(200, 3) - 0.5)
    one = {k: v[:1].detach() for k, v in params.items()}
    a = ops.field_eval_knn(fc, one, pts.to(DEV), g["pos"][:1].to(DEV), g["quat"][:1].to(DEV), 1, 10.0, 1.0)
    b = ops.field_eval(fc, one, pts[None].to(DEV), g["pos"][:1].to(DEV), g["quat"][:1].to(DEV))[0]
    close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["g19_skip_add_nerf", "g19_skip_concat_nerf", "g19_skip_add_triplane", "g19_skip_concat_triplane"])
def test_skip_with_other_encodings_golden(name):
    """models.py:159-169 is encoding-agnostic: skip add / concat with NeRF octaves and with the triplane encoding against
    the real reference (G19): forward, every parameter gradient (planes included), the kNN evaluation path."""
    g = load_golden(name)
    mode, enc = name.split("_")[2], name.split("_")[3]
    if enc == "nerf":
        fc = K.field_cfg(encoding="nerf", num_octaves=8, num_layers=2, skip_mode=mode)
        ftol, gtol = dict(rtol=2e-3, atol=3e-4), 2e-3             # arguments up to 2^7 pi: forward looser; gradients at the common bar
    else:
        fc = K.field_cfg(encoding="triplane", resolution=12, num_components=32, tri_mode="sum", num_layers=2, skip_mode=mode,
                         scale_mode="unit_ball")
        ftol, gtol = dict(rtol=2e-4, atol=3e-5), 2e-3
    assert K.param_shapes(fc)["_linears.1.weight"] == tuple(g["p::_linears.1.weight"].shape[1:])
    params = {k: v.to(DEV).requires_grad_() for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"}
    out = ops.field_eval(fc, params, g["query"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV))
    close(out, g["out"], **ftol)
    (out * g["seed"].to(DEV)).sum().backward()
    assert K.lib().ngm_debug_last_bwd_variant() == 0              # skip connections run on the 32-sample-tile kernel
    for k, gr in split_prefix(g, "g::").items():
        grad_close(params[k].grad, gr, gtol, k)
    pts = g["pos"][:1] + 0.4 * (torch.rand(200, 3) - 0.5)
    one = {k: v[:1].detach() for k, v in params.items()}
    a = ops.field_eval_knn(fc, one, pts.to(DEV), g["pos"][:1].to(DEV), g["quat"][:1].to(DEV), 1, 10.0, 1.0)
    b = ops.field_eval(fc, one, pts[None].to(DEV), g["pos"][:1].to(DEV), g["quat"][:1].to(DEV))[0]
    close(a, b, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("mode", ["add", "concat"])
@pytest.mark.parametrize("enc", ["permuto", "nerf", "triplane"])
def test_skip_other_encodings_fused_train_step_vs_oracle(enc, mode):
    """the fused render / train step with skip connections on every encoding the Fourier-only build refused
    (hash: 1x32 MLP, W_out becomes (4, 32 + 32) with concat; parity of the hash encoding itself is unpinned)"""
    F, R, n_c, n_g = 2, 33, 6, 10
    torch.manual_seed(8)
    fkw = dict(permuto=dict(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4),
               nerf=dict(encoding="nerf", num_octaves=8, num_layers=2),
               triplane=dict(encoding="triplane", resolution=16, num_components=32, tri_mode="sum", num_layers=2))[enc]
    fkw = dict(fkw, skip_mode=mode)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    pos, quat, t = synth_target(F, R, seed=4)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    params = O.init_params(fs, F, seed=11)
    params[f"_linears.{fkw['num_layers']}.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g)
    po = {k: v.clone().requires_grad_(k != "_encoding.random_shift_per_level") for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    r = make_renderer(fkw, ckw, F, params)
    if mode == "concat":
        assert r._model.all_fields_params[f"_linears.{fkw['num_layers']}.weight"].shape[-1] == fs.dim_hidden + fs.dim_enc
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    loose = enc != "triplane"            # hash: lattice coordinates up to 1e4; NeRF: arguments up to 2^7 pi
    # "add" puts the encoding itself (fp32 error ~1e-3 absolute at these frequencies / lattice scales, in the oracle as in the
    # kernels) straight into the hidden units of every layer: a single ray in 264 sat 5e-4 off at atol 2e-4
    close(res["prediction"].rgbds, pred["rgbds"].detach(),
          **(dict(rtol=2e-3, atol=1e-3 if mode == "add" else 2e-4) if loose else {}))
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    close(res["combined"], loss["combined"].detach(), rtol=2e-3 if loose else 3e-4, atol=1e-5)
    loss["combined"].backward()
    for k in po:
        if po[k].grad is not None:
            if enc == "permuto":
                hash_grad_close(res["grads"][k], po[k].grad, k)
            else:            # NeRF octaves: measured worst 3.4e-4 over the suite (profiles/r05_parity_margins.txt); was 1e-2
                grad_close(res["grads"][k], po[k].grad, 2e-3, k)
    out = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=True)   # fused Adam
    assert torch.isfinite(out["combined"])


@pytest.mark.parametrize("tri_mode,comps", [("sum", 64), ("product", 32), ("concat", 20)])
def test_triplane_fused_train_step_vs_oracle(tri_mode, comps):
    F, R, n_c, n_g = 2, 33, 6, 10
    torch.manual_seed(8)
    fkw = dict(encoding="triplane", resolution=16, num_components=comps, tri_mode=tri_mode, num_layers=1)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    pos, quat, t = synth_target(F, R, seed=4)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3)
    params = O.init_params(fs, F, seed=11)
    params["_linears.1.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g)
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    r = make_renderer(fkw, ckw, F, params)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    tgt = make_target(t, torch.arange(F))
    res = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=False)
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    close(res["combined"], loss["combined"].detach(), rtol=3e-4, atol=1e-6)
    loss["combined"].backward()
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 2e-3, k)
    again = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=False)
    assert torch.equal(again["grads"]["_encoding.plane_coef"], res["grads"]["_encoding.plane_coef"])   # fixed-point scatter
    before = r._model.all_fields_params["_encoding.plane_coef"].clone()
    out = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=True)                          # Adam on the planes too
    assert torch.isfinite(out["combined"]) and not torch.equal(before, r._model.all_fields_params["_encoding.plane_coef"])


# ------------------------------------------------------------------------- train step (G6, G7)
@pytest.mark.parametrize("name", list(CASES))
def test_fused_train_step_golden(name):
    g = load_golden(name)
    fkw, ckw = CASES[name]
    F = g["pos"].shape[0]
    r = make_renderer(fkw, ckw, F, split_prefix(g, "p::"))
    r.set_field_poses(g["pos"].to(DEV), g["quat"].to(DEV))
    tgt = make_target(split_prefix(g, "t::"), torch.arange(F))
    res = r.optimization_iteration(tgt, g["u_coarse"].to(DEV), g["u_guided"].to(DEV), update=False)
    nerf = fkw["encoding"] == "nerf"
    ft = dict(rtol=2e-3, atol=3e-4) if nerf else dict(rtol=2e-4, atol=2e-5)
    p = res["prediction"]
    close(p.rgbds, g["pred_rgbds"], **ft)
    close(p.color_vars, g["pred_color_vars"], **ft)
    close(p.depth_vars, g["pred_depth_vars"], **ft)
    close(p.term_probs, g["pred_term_probs"], **ft)
    ref_loss = split_prefix(g, "loss::")
    for k, v in ref_loss.items():
        close(res[k], v, rtol=1e-3 if nerf else 2e-4, atol=1e-5)
    for k, v in split_prefix(g, "g::").items():
        grad_close(res["grads"][k], v, 2e-3, k)                  # NeRF octaves too: measured 3.4e-4 (was 1e-2)


@pytest.mark.parametrize("name", ["g6_train_cfg0", "g6_train_3field", "g18_train_l2", "g20_train_gnll_gnll", "g20_train_l1_lnll",
                                  "g20_train_gnll_switch_l1", "g28_train_gnll_nll_branch"])
def test_render_ijs_autograd_path_golden(name):
    """reference-style call sequence: render_ijs -> compute_losses -> backward (rm.py:1164-1186).  G20: the *_nll loss modes,
    whose autograd reaches the parameters through Prediction.depth_vars as well (ngm_render_bwd_seeded_vars); G28: through
    Prediction.color_vars too (the G20 fixtures are on the L1 side of the photometric switch)."""
    g = load_golden(name)
    fkw, ckw = CASES[name]
    F = g["pos"].shape[0]
    r = make_renderer(fkw, ckw, F, split_prefix(g, "p::"))
    r.set_field_poses(g["pos"].to(DEV), g["quat"].to(DEV))
    ids = torch.arange(F, device=DEV)
    tgt = make_target(split_prefix(g, "t::"), ids)
    pred = r.render_ijs(tgt.ijs, tgt.c2ws, None, field_ids=ids, use_vmap=True, near_distances=tgt.near_distances,
                        far_distances=tgt.far_distances, gt_distances=tgt.gt_distances,
                        u_coarse=g["u_coarse"].to(DEV), u_guided=g["u_guided"].to(DEV))
    close(pred.rgbds, g["pred_rgbds"])
    assert pred.freespace_geometry.shape == g["pred_freespace"].shape
    assert pred.tsdf_residuals.shape == g["pred_tsdf"].shape
    close(pred.freespace_geometry, g["pred_freespace"])
    close(pred.tsdf_residuals, g["pred_tsdf"])
    loss = r.compute_losses(tgt, pred)
    close(loss["combined"], split_prefix(g, "loss::")["combined"], rtol=2e-4, atol=1e-6)
    loss["combined"].backward()
    vp = r._model.vmap_fields_params
    for k, v in split_prefix(g, "g::").items():
        grad_close(vp[k].grad, v, 2e-3, k)


def test_sparse_adam_ten_iterations_golden():
    """G7: trained parameters after 10 iterations with changing active sets and the shared step."""
    g = load_golden("g7_adam")
    fkw = dict(encoding="fourier", dim_enc=32, num_layers=2)
    ckw = dict(num_samples_coarse=4, num_samples_depth_guided=8)
    NF = g["pos"].shape[0]
    r = make_renderer(fkw, ckw, NF, {k: v for k, v in split_prefix(g, "p0::").items()})
    r.set_field_poses(g["pos"].to(DEV), g["quat"].to(DEV))
    for it in range(int(g["num_iters"])):
        t = split_prefix(g, f"it{it}::")
        ids = t.pop("field_ids")
        uc, ug, ref = t.pop("u_coarse"), t.pop("u_guided"), t.pop("loss")
        res = r.optimization_iteration(make_target(t, ids), uc.to(DEV), ug.to(DEV), update=True)
        close(res["combined"], ref, rtol=2e-3, atol=1e-5)
    for k, v in split_prefix(g, "p1::").items():
        if k == "_neus_sd":
            continue
        close(r._model.all_fields_params[k], v, rtol=2e-3, atol=5e-5)
        close(r._optim_state[k]["exp_avg"], g["m1::" + k], rtol=5e-3, atol=1e-6)
        grad_close(r._optim_state[k]["exp_avg_sq"], g["v1::" + k], 5e-3, "exp_avg_sq " + k)   # sums of g^2: 2x the gradient bar


# ---------------------------------------------------------------- full-size properties (M1 shape)
def test_full_size_properties_m1():
    F, R = 8, 512
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=64, num_samples_depth_guided=64)
    pos, quat, t = synth_target(F, R)
    r = make_renderer(fkw, ckw, F)
    with torch.no_grad():
        for k, v in r._model.all_fields_params.items():
            if v.dim() > 1:
                v.add_(0.05 * torch.randn_like(v))
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    tgt = make_target(t, torch.arange(F))
    a = r.optimization_iteration(tgt, seed=11, update=False)
    pa = {k: v.clone() for k, v in a["grads"].items()}
    pred_a = a["prediction"].rgbds.clone()
    term = a["prediction"].term_probs
    assert torch.isfinite(pred_a).all() and all(torch.isfinite(v).all() for v in pa.values())
    assert float(term.min()) >= -1e-6 and float(term.max()) <= 1 + 1e-5          # sum w + bg = 1
    assert (a["prediction"].color_vars >= -1e-7).all() and (a["prediction"].depth_vars >= -1e-7).all()
    # determinism: same seed -> bitwise identical predictions and gradients (fixed reduction order)
    b = r.optimization_iteration(tgt, seed=11, update=False)
    assert torch.equal(b["prediction"].rgbds, pred_a)
    for k in pa:
        assert torch.equal(b["grads"][k], pa[k]), k
    # at this size the default plan is ray-aligned: the split backward did the compositing backward itself (no k_stash_bwd
    # launch); the same step behind k_stash_bwd: same loss scalars bit for bit, gradients to 1e-5 of their scale
    from neural_graph_mapping_amd import _capi
    Lc = _capi.lib()
    assert Lc.ngm_debug_last_bwd_variant() == 3 and Lc.ngm_debug_last_comp_fused() == 1
    Lc.ngm_debug_disable_fused_comp(1)
    try:
        u = r.optimization_iteration(tgt, seed=11, update=False)
        assert Lc.ngm_debug_last_bwd_variant() == 3 and Lc.ngm_debug_last_comp_fused() == 0
        assert torch.equal(u["combined"], b["combined"]) and torch.equal(u["prediction"].rgbds, pred_a)
        for k in pa:
            grad_close(u["grads"][k], pa[k], 1e-5, "separate compositing backward " + k)
    finally:
        Lc.ngm_debug_disable_fused_comp(0)
    # field permutation equivariance (fields are independent; only the global loss counts couple them)
    perm = torch.tensor([3, 0, 7, 1, 6, 2, 5, 4])
    tp = {k: v[perm] for k, v in t.items()}
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    c = r.optimization_iteration(make_target(tp, perm), seed=11, update=False)
    # Philox streams are keyed by batch position, so compare statistically-free quantities: loss counts
    assert abs(float(c["combined"]) - float(a["combined"])) / float(a["combined"]) < 0.05
    # linearity of the backward in the loss weights
    r2 = make_renderer(fkw, {**ckw, "photometric_weight": 2.0, "depth_weight": 2.0, "freespace_weight": 80.0,
                             "tsdf_weight": 100.0}, F, {k: v for k, v in r._model.all_fields_params.items()})
    r2.set_field_poses(pos.to(DEV), quat.to(DEV))
    d = r2.optimization_iteration(tgt, seed=11, update=False)
    for k in pa:
        grad_close(d["grads"][k], 2 * pa[k], 1e-5, k)


def test_idle_rank_iteration():
    """a rank with no active field in an iteration still enters the loss all-reduce with zeros and keeps the shared
    step counter moving; without a process group that is just the bookkeeping."""
    F, R = 2, 8
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=4, num_samples_depth_guided=4)
    pos, quat, t = synth_target(F, R, seed=3)
    r = make_renderer(fkw, ckw, F)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    empty = make_target({k: v[:0] for k, v in t.items()}, torch.arange(0))
    p0 = {k: v.clone() for k, v in r._model.all_fields_params.items()}
    out = r.optimization_iteration(empty, update=True)
    # no ray anywhere: every mean is over an empty selection -- NaN, like the reference's `.mean()` of an empty tensor
    assert bool(torch.isnan(out["combined"])) and r._step == 1 and int(r._step_dev.item()) == 1
    for k, v in r._model.all_fields_params.items():
        assert torch.equal(v, p0[k])
    r.optimization_iteration(make_target(t, torch.arange(F)), seed=1, update=True)      # a normal iteration follows
    assert r._step == 2 and int(r._step_dev.item()) == 2


def test_iteration_counter_drives_jitter_and_adam_step():
    """One device counter counts the iterations (ngm_rays.philox_offset_autoinc): the forward adds it to the Philox
    offset, the loss reduction advances it, Adam reads it as its step.  update=False must leave it alone; a captured
    iteration must advance it at every replay (fresh jitter, growing step)."""
    F, R = 2, 16
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=8, num_samples_depth_guided=8)
    pos, quat, t = synth_target(F, R, seed=3)
    r = make_renderer(fkw, ckw, F)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    tgt = make_target(t, torch.arange(F))
    a = r.optimization_iteration(tgt, seed=5, update=False)["prediction"].rgbds.clone()
    b = r.optimization_iteration(tgt, seed=5, update=False)["prediction"].rgbds.clone()
    assert torch.equal(a, b) and int(r._step_dev.item()) == 0                   # nothing advanced
    p0 = {k: v.clone() for k, v in r._model.all_fields_params.items()}
    r.optimization_iteration(tgt, seed=5, update=True)
    assert int(r._step_dev.item()) == 1 == r._step
    c = r.optimization_iteration(tgt, seed=5, update=False)["prediction"].rgbds.clone()
    assert not torch.equal(a, c)                                                 # new jitter offset (and new parameters)
    # first Adam step with zero moments moves every parameter with a non-zero gradient by ~lr (bias correction of step 1)
    moved = max(float((r._model.all_fields_params[k] - p0[k]).abs().max()) for k in p0)
    assert 0.2 * r._learning_rate < moved < 1.5 * r._learning_rate, moved
    replay = r.capture_iteration(tgt, seed=5)
    s0 = int(r._step_dev.item())
    for _ in range(3):
        replay()
    torch.cuda.synchronize()
    assert int(r._step_dev.item()) == s0 + 3 == r._step


@pytest.mark.parametrize("F,R,n_c,n_g", [(1, 5, 3, 0), (2, 33, 1, 1), (5, 7, 8, 16), (1, 1, 128, 0), (3, 130, 20, 4)])
def test_ragged_shapes_vs_oracle(F, R, n_c, n_g):
    ragged_case(F, R, n_c, n_g, dict(encoding="fourier", dim_enc=32, num_layers=1))


@pytest.mark.parametrize("mm,variant", [("f32", 2), ("auto", 3)])
@pytest.mark.parametrize("F,R,n_c,n_g,layers", [(2, 33, 1, 1, 2), (5, 7, 8, 16, 2), (3, 130, 20, 4, 2), (3, 37, 5, 2, 1),
                                                (1, 1, 128, 0, 2), (2, 9, 31, 0, 1)])
def test_ragged_shapes_stash_backward(F, R, n_c, n_g, layers, mm, variant):
    """64-wide layers: the training forward stashes the hidden activations and the backward consumes them --
    k_field_bwd16s (fp32 MFMA, 16-sample tiles) or k_field_bwd_b3 (three-way bf16 split, 32-sample tiles): partial
    tiles, fields that start in the middle of a 32-sample stash tile.  Same tolerances for both."""
    ragged_case(F, R, n_c, n_g, dict(encoding="fourier", dim_enc=64, num_layers=layers), mlp_matmul=mm)
    from neural_graph_mapping_amd import _capi
    assert _capi.lib().ngm_debug_last_bwd_variant() == variant
    # the split kernel also does the compositing backward (no k_stash_bwd launch) -- rays of 2, 7, 24, 31 and 128 samples
    # against its 32-sample tiles, wave ranges that end in the middle of a ray, partial last tiles, fields starting in the
    # middle of a stash tile; the fp32 kernels leave it to k_stash_bwd
    assert _capi.lib().ngm_debug_last_comp_fused() == (1 if variant == 3 else 0)
    if variant == 3:                                 # and the same kernel behind k_stash_bwd
        L = _capi.lib()
        L.ngm_debug_disable_fused_comp(1)
        try:
            ragged_case(F, R, n_c, n_g, dict(encoding="fourier", dim_enc=64, num_layers=layers), mlp_matmul=mm)
            assert L.ngm_debug_last_bwd_variant() == 3 and L.ngm_debug_last_comp_fused() == 0
        finally:
            L.ngm_debug_disable_fused_comp(0)


@pytest.mark.parametrize("geom", ["nrgbd", "occupancy", "density"])
@pytest.mark.parametrize("photo", ["l1", "l2"])
def test_fused_compositing_backward_equals_stash_bwd(geom, photo):
    """The compositing backward inside k_field_bwd_b3 against k_stash_bwd + the same kernel on one batch (8 + 16 samples,
    rays straddling the 32-sample tiles): same loss scalars bit for bit (same sums), gradients to 1e-5 of their scale (the
    per-ray suffix recursion is composed in a different order); the density mode is not fused."""
    from neural_graph_mapping_amd import _capi
    L = _capi.lib()
    F, R = 3, 40
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=8, num_samples_depth_guided=16, geometry_mode=geom, photometric_loss=photo,
               termination_weight=0.3, mlp_matmul="auto")
    pos, quat, t = synth_target(F, R, seed=11)
    r = make_renderer(fkw, ckw, F)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    tgt = make_target(t, torch.arange(F))
    out = {}
    try:
        for fused in (1, 0):
            L.ngm_debug_disable_fused_comp(0 if fused else 1)
            res = r.optimization_iteration(tgt, seed=5, update=False)
            torch.cuda.synchronize()
            assert L.ngm_debug_last_bwd_variant() == 3
            assert L.ngm_debug_last_comp_fused() == (1 if fused and geom != "density" else 0)
            out[fused] = ({k: v.clone() for k, v in res.items() if k not in ("grads", "prediction")},
                          {k: v.clone() for k, v in res["grads"].items()})
    finally:
        L.ngm_debug_disable_fused_comp(0)
    for k, v in out[1][0].items():          # bitwise; NaN (an empty selection's term, as in the reference) counts as equal to NaN
        o = out[0][0][k]
        assert torch.equal(torch.isnan(v), torch.isnan(o)) and torch.equal(v.nan_to_num(), o.nan_to_num()), k
    for k, v in out[1][1].items():
        scale = float(out[0][1][k].abs().max()) + 1e-30
        assert float((v - out[0][1][k]).abs().max()) / scale < 1e-5, k
        assert float(v.abs().max()) > 0, k


@pytest.mark.parametrize("enc", ["nerf", "fourier61"])
def test_stash_backward_bf16_split_other_encodings(enc):
    """NeRF octaves (no encoding gradient: one weight plane set) and zero-padded widths (61 of 64 features)."""
    fkw = (dict(encoding="nerf", num_octaves=10, num_layers=2) if enc == "nerf" else
           dict(encoding="fourier", dim_enc=61, num_layers=2))
    ragged_case(3, 41, 9, 5, fkw, mlp_matmul="auto")
    from neural_graph_mapping_amd import _capi
    L = _capi.lib()
    assert L.ngm_debug_last_bwd_variant() == 3


# ------------------------------------------------------------------ eval path: kNN blend + image (G8, G9)
@pytest.mark.parametrize("mm", ["auto", "f32", "bf16x3"])
def test_knn_blend_golden(mm):
    """G8 through each arithmetic of the evaluation kernels' hidden layers; which one really ran is read back from the
    library (ngm_debug_last_matmul), so a silent fallback to the other would fail here"""
    g = load_golden("g8_knn")
    fc = K.field_cfg(encoding="fourier", dim_enc=64, num_layers=2, matmul_mode=mm)
    params = cu({k: v for k, v in split_prefix(g, "p::").items() if k != "_neus_sd"})
    out = ops.field_eval_knn(fc, params, g["points"].to(DEV), g["pos"].to(DEV), g["quat"].to(DEV), 2, 10.0, 1.0)
    assert K.lib().ngm_debug_last_matmul(2) == K.MATMUL["f32" if mm == "f32" else "bf16x3"]
    close(out, g["out"], rtol=2e-4, atol=3e-5)
    assert torch.equal(out[:5].cpu(), torch.ones(5, 4))
    pts = g["points"][:64].to(DEV)
    one = {k: v[:1] for k, v in params.items()}
    ops.field_eval(fc, one, pts[None], g["pos"][:1].to(DEV), g["quat"][:1].to(DEV))
    assert K.lib().ngm_debug_last_matmul(1) == K.MATMUL["f32" if mm == "f32" else "bf16x3"]       # the point evaluation too


@pytest.mark.parametrize("NF,K_,P", [(1, 2, 300), (7, 3, 5000), (40, 2, 70000), (40, 5, 9000), (12, 8, 9000), (6, 8, 3000), (90, 7, 20000),
                                     (40, 9, 9000), (60, 12, 6000), (30, 16, 5000), (11, 16, 2000)])     # K = 9..16: the 16-slot instance (round 6)
def test_knn_blend_vs_oracle(NF, K_, P):
    torch.manual_seed(NF)
    fs = O.FieldSpec(encoding="fourier", dim_enc=32, num_layers=1)
    fc = K.field_cfg(encoding="fourier", dim_enc=32, num_layers=1)
    params = O.init_params(fs, NF, seed=NF, sigma=3.0)
    pos = torch.rand(NF, 3) * 3
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1)
    pts = torch.rand(P, 3) * 4 - 0.5
    ref = O.field_set_forward_knn(pts, pos, quat, params, fs, num_knn=K_, distance_factor=10.0, outside_value=1.0)
    out = ops.field_eval_knn(fc, cu(params), pts.to(DEV), pos.to(DEV), quat.to(DEV), K_, 10.0, 1.0)
    close(out, ref, rtol=3e-4, atol=3e-5)


@pytest.mark.parametrize("NF,K_", [(150, 2), (150, 4), (3, 4), (70, 1)])
def test_knn_blend_ray_ordered_points_vs_oracle(NF, K_):
    """points in ray order (what render_image feeds): the assignment kernel culls the field list per wave from the
    wave's bounding ball -- the result must still be the exact K nearest (ragged tail, segments that leave every
    field, fewer centres than K)."""
    torch.manual_seed(100 + NF)
    fs = O.FieldSpec(encoding="fourier", dim_enc=32, num_layers=1)
    fc = K.field_cfg(encoding="fourier", dim_enc=32, num_layers=1)
    params = O.init_params(fs, NF, seed=NF, sigma=3.0)
    g = torch.arange(0.0, 3.01, 0.6)
    grid = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    pos = grid[torch.randperm(grid.shape[0])[:NF] % grid.shape[0]] if NF <= grid.shape[0] else grid
    pos = pos.clone() + 1e-3 * torch.randn(pos.shape[0], 3)   # no exact distance ties (their order is unpinned in the reference)
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1)
    o = torch.rand(37, 1, 3) * 3
    d = torch.nn.functional.normalize(torch.randn(37, 1, 3), dim=-1)
    t = torch.linspace(-1.0, 5.0, 333)[None, :, None]
    pts = (o + t * d).reshape(-1, 3)[:-11]                    # 37 rays x 333 samples, ragged tail
    ref = O.field_set_forward_knn(pts, pos, quat, params, fs, num_knn=K_, distance_factor=10.0, outside_value=1.0)
    out = ops.field_eval_knn(fc, cu(params), pts.to(DEV), pos.to(DEV), quat.to(DEV), K_, 10.0, 1.0)
    close(out, ref, rtol=3e-4, atol=3e-5)


def test_render_image_and_psnr_golden():
    g = load_golden("g9_render_image")
    w, h, fx, fy, cx, cy = [float(x) for x in g["cam"]]
    fkw = dict(encoding="fourier", dim_enc=64, num_layers=2)
    ckw = dict(num_samples_coarse=8, num_samples_depth_guided=16, eval_far_distance=float(g["eval_far"]),
               eval_num_samples=int(g["eval_num_samples"]))
    NF = g["pos"].shape[0]
    r = make_renderer(fkw, ckw, NF, split_prefix(g, "p::"))
    r.set_field_poses(g["pos"].to(DEV), g["quat"].to(DEV))
    cam = Rr.Camera(int(w), int(h), fx, fy, cx, cy, pixel_center=0.0)
    r.eval()                                                          # make_golden.g9_render_image: ngm.eval() first
    rgbd, dvar = r.render_image(g["c2w"].to(DEV), cam, u=g["u"].to(DEV))
    close(rgbd, g["rgbd"], rtol=5e-4, atol=5e-5)
    close(dvar, g["dvar"], rtol=5e-4, atol=5e-5)
    p = r.psnr(rgbd[..., :3].cpu(), g["target_rgb"], crop=2)
    assert abs(p - O.psnr(g["rgbd"][..., :3], g["target_rgb"], crop=2)) < 0.01       # well inside the 0.1 dB bar


# --------------------------------------------------------- permutohedral hash encoding (parity unpinned)
PERMUTO = dict(encoding="permuto", nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)


@pytest.mark.parametrize("L_", [1, 2])
@pytest.mark.parametrize("P", [64, 1000])
def test_permuto_field_eval_vs_oracle(L_, P):
    """HIP hash encoding + MLP against the oracle's restatement of the published lattice algorithm
    (NOT against the reference's CUDA package, which cannot run here: parity unpinned)."""
    torch.manual_seed(P)
    F = 2
    fs = O.FieldSpec(num_layers=L_, **PERMUTO)
    fc = K.field_cfg(num_layers=L_, **PERMUTO)
    params = O.init_params(fs, F, seed=3)
    x = torch.rand(F, P, 3)                                          # already in the unit-cube field frame
    p64 = {k: v.double() for k, v in params.items()}
    for _ in range(20):                                              # keep the points off the ReLU kinks (fp64 check)
        pres = []
        O.field_mlp(O.encode(x.double(), p64, fs), p64, fs, pre_out=pres)
        bad = torch.stack([(pre.abs() < 5e-5).any(-1) for pre in pres]).any(0)
        if not bad.any():
            break
        x[bad] = torch.rand(int(bad.sum()), 3)
    assert not bad.any()
    d_out = torch.randn(F, P, 4)
    po = {k: v.clone().requires_grad_(k != "_encoding.random_shift_per_level") for k, v in params.items()}
    out_o = O.field_forward_local(x, po, fs)
    (out_o * d_out).sum().backward()
    fc_local = K.field_cfg(num_layers=L_, scale_mode="no", **PERMUTO)
    pg = {k: v.to(DEV).requires_grad_(k != "_encoding.random_shift_per_level") for k, v in params.items()}
    out = ops.field_eval(fc_local, pg, x.to(DEV))
    close(out, out_o.detach(), rtol=1e-3, atol=1e-4)
    (out * d_out.to(DEV)).sum().backward()
    for k in po:
        if po[k].grad is not None:
            hash_grad_close(pg[k].grad, po[k].grad, k)               # hash: measured bars per tensor / level group (gpu_common.HASH_BARS)
    # table gradient: every touched entry matches, untouched entries are exactly zero
    gl, rl = pg["_encoding.lattice_values"].grad.cpu(), po["_encoding.lattice_values"].grad
    assert torch.equal(gl == 0, rl == 0) or float(((gl == 0) != (rl == 0)).float().mean()) < 1e-3


@pytest.mark.parametrize("mm", ["auto", "f32", "auto-separate", "auto-float"])
@pytest.mark.parametrize("F,R,n_c,n_g", [(3, 40, 8, 16), (1, 9, 4, 4), (2, 33, 3, 2), (5, 7, 8, 16), (3, 130, 20, 4)])
def test_permuto_fused_train_step_vs_oracle(F, R, n_c, n_g, mm):
    """the reference's DEFAULT field (config/neural_graph_map.yaml:6-20): hash encoding, 1x32 MLP; ragged shapes put
    field starts in the middle of the 32-sample tiles of the encoding stash and leave partial tiles.  Both backward
    kernels: k_hash_mlp_bwd (bf16 split, `auto`: it also does the compositing backward and writes the positions of
    k_hash_grad; `auto-separate`: behind k_stash_bwd) and k_field_bwd16 (fp32 MFMA, `mlp_matmul: f32`).  `auto-float`: the
    opt-in `hash_grad_atomics: float` (fp32 LDS atomics like the reference's CUDA package): same bars, no bitwise claim."""
    separate = mm == "auto-separate"
    atomics = "float" if mm == "auto-float" else "exact"
    if mm == "auto-float":
        mm = "auto"
    if separate:
        mm = "auto"
        K.lib().ngm_debug_disable_fused_comp(1)
    try:
        _permuto_train_case(F, R, n_c, n_g, mm, atomics=atomics)
        assert K.lib().ngm_debug_last_comp_fused() == (1 if (mm == "auto" and not separate) else 0)
    finally:
        K.lib().ngm_debug_disable_fused_comp(0)


def _permuto_train_case(F, R, n_c, n_g, mm, max_neutralised=0.15, atomics="exact"):
    torch.manual_seed(5)
    fs = O.FieldSpec(num_layers=1, **PERMUTO)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g)
    pos, quat, t = synth_target(F, R, seed=17)
    params = O.init_params(fs, F, seed=9)
    params["_linears.1.weight"] *= 2.0
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g, max_neutralised=max_neutralised)
    po = {k: v.clone().requires_grad_(k != "_encoding.random_shift_per_level") for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    loss["combined"].backward()
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PermutohedralEncoding",
        encoding_kwargs=dict(pos_dim=3, log2_hashmap_size=12, nr_levels=16, nr_feat_per_level=2, coarsest_scale=1,
                             finest_scale=0.0001, init_scale=0.00001), num_layers=1, dim_out=4, neus_initial_sd=1.0),
        num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=1.0, scale_mode="unit_cube").to(DEV)
    cfg = Rr.shipped_config(num_samples_coarse=n_c, num_samples_depth_guided=n_g, mlp_matmul=mm, hash_grad_atomics=atomics)
    cam = Rr.Camera(640, 480, NRGBD_KW["fx"], NRGBD_KW["fy"], 319.5, 239.5)
    r = Rr.NeuralGraphRenderer(model, cam, cfg, device=DEV)
    r.add_fields(F)
    assert set(model.all_fields_params) >= {"_encoding.lattice_values", "_encoding.random_shift_per_level"}
    for k, v in params.items():
        model.all_fields_params[k].copy_(v.to(DEV))
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    assert K.lib().ngm_debug_last_bwd_variant() == (5 if mm == "auto" else 1)     # no silent fallback either way
    close(res["prediction"].rgbds, pred["rgbds"].detach(), rtol=2e-3, atol=2e-4)
    compare_losses(res, pred, t, rs, rtol=2e-3, atol=1e-5)
    for k in po:
        if po[k].grad is not None:
            hash_grad_close(res["grads"][k], po[k].grad, k)           # hash: measured bars per tensor / level group (gpu_common.HASH_BARS)
    first = {k: v.clone() for k, v in res["grads"].items()}            # (the renderer reuses its gradient buffers)
    again = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    for k in first:
        if atomics == "float" and k == "_encoding.lattice_values":     # float atomics: the order of the adds is not fixed
            grad_close(again["grads"][k], first[k], 1e-5, "float atomics, run to run")
            continue
        assert torch.equal(again["grads"][k], first[k]), k             # fixed orders + fixed-point scatter: bitwise reproducible
    before = model.all_fields_params["_encoding.random_shift_per_level"].clone()
    r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=True)
    assert torch.equal(before, model.all_fields_params["_encoding.random_shift_per_level"])   # no grad -> untouched
    # the update itself (fused into the reduction kernels: MLP tensors in k_grad_reduce, hash tables in k_hash_reduce):
    # first Adam step from zero moments on the oracle's gradients
    for k in ("_encoding.lattice_values", "_linears.0.weight", "_linears.1.bias"):
        exp, _, _ = O.adam_step(params[k], po[k].grad, torch.zeros_like(params[k]), torch.zeros_like(params[k]), 1,
                                lr=1e-3, eps=1e-15, weight_decay=1e-5)
        got = model.all_fields_params[k].cpu()
        big = po[k].grad.abs() > 1e-3 * po[k].grad.abs().max()     # |update| = lr there, whatever the rounding of g
        close(got[big], exp[big], rtol=1e-5, atol=2e-6)
        assert float((got - params[k]).abs().max()) <= 1.001e-3     # nothing moves by more than lr on step 1


# ------------------------------------------------------------------ training-target sampler (G11)
def test_target_sampler_golden():
    """_sample_target_mv (rm.py:1259-1459) with the reference's recorded draws: pixel indices, field ids and masks
    must be identical, distances / poses / RGB-D within fp32 round-off."""
    g = load_golden("g11_target_sampler")
    fkw = dict(encoding="fourier", dim_enc=32, num_layers=1)
    r = make_renderer(fkw, dict(num_samples_coarse=4, num_samples_depth_guided=4), int(g["num_fields"]))
    r.set_field_poses(g["positions"].to(DEV), torch.zeros(int(g["num_fields"]), 4, device=DEV))
    cam = Rr.Camera(int(g["width"]), int(g["height"]), float(g["fx"]), float(g["fy"]), float(g["cx"]), float(g["cy"]),
                    pixel_center=0.0)
    draws = dict(subset_observed=g["d_subset_observed"], subset_random=g["d_subset_random"], offsets=g["d_offsets"],
                 frame_cids=g["d_frame_cids"], u_xy=g["d_u_xy"])
    t = r.sample_target_mv(g["current_field_ids"], g["c_c2w"].to(DEV), g["nc_rgbd"].to(DEV).contiguous(),
                           g["frame_cid_to_ncid"].to(DEV), int(g["num_train_fields"]), int(g["num_rays_per_field"]),
                           camera=cam, draws=draws)
    assert torch.equal(t.field_ids.cpu(), g["o_field_ids"])
    assert torch.equal(t.ijs.cpu(), g["o_ijs"].long())
    for a, b in ((t.c2ws, "o_c2ws"), (t.near_distances, "o_near"), (t.far_distances, "o_far"), (t.gt_distances, "o_gt"),
                 (t.rgbds, "o_rgbds"), (t.term_probs, "o_term_probs")):
        close(a, g[b], rtol=2e-6, atol=2e-6)
    for a, b in ((t.rgb_mask, "o_rgb_mask"), (t.depth_mask, "o_depth_mask"), (t.term_mask, "o_term_mask")):
        assert torch.equal(a.cpu(), g[b]), b
    # own draws on the device: structural checks only (the stream differs from the CPU generator's)
    torch.manual_seed(3)
    t2 = r.sample_target_mv(g["current_field_ids"], g["c_c2w"].to(DEV), g["nc_rgbd"].to(DEV).contiguous(),
                            g["frame_cid_to_ncid"].to(DEV), int(g["num_train_fields"]), int(g["num_rays_per_field"]),
                            camera=cam)
    assert t2.ijs.shape[1:] == (16, 2) and t2.ijs.shape[0] == len(t2.field_ids) <= 8
    assert bool((t2.near_distances <= t2.far_distances).all()) and bool((t2.near_distances >= 0).all())
    assert bool((t2.ijs[..., 0] < 48).all()) and bool((t2.ijs[..., 1] < 64).all()) and bool((t2.ijs >= 0).all())


def test_target_sampler_single_view_golden():
    """_sample_target_sv (rm.py:1461-1583, update_mode single_view) with the reference's recorded draws on the procedural frame
    of fixture G16: the field set, pixel indices and masks must be identical (so the segment-sphere test agrees on all
    14 x 50 000 pairs that matter), distances / RGB-D within fp32 round-off."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import scene
    g = load_golden("g16_target_sampler_sv")
    NF = g["positions"].shape[0]
    fkw = dict(encoding="fourier", dim_enc=32, num_layers=1)
    r = make_renderer(fkw, dict(num_samples_coarse=4, num_samples_depth_guided=4, field_radius=float(g["field_radius"])), NF)
    r.set_field_poses(g["positions"].to(DEV), torch.zeros(NF, 4, device=DEV))
    cam = Rr.Camera(scene.SV_W, scene.SV_H, scene.SV_FX, scene.SV_FY, scene.SV_CX, scene.SV_CY, pixel_center=0.0)
    img = scene.sv_frame(int(g["frame_seed"]))
    draws = dict(subset_points=g["d_subset_points"].long(), segments=g["d_segments"],
                 subset_fields=g["d_subset_fields"] if "d_subset_fields" in g else None)
    R = int(g["num_rays_per_field"])
    t = r.sample_target_sv(img, g["c2w"], g["active_field_ids"], int(g["num_train_fields"]), R, camera=cam, draws=draws)
    assert torch.equal(t.field_ids.cpu(), g["o_field_ids"])
    assert torch.equal(t.ijs.cpu(), g["o_ijs"].long())
    for a, b in ((t.c2ws, "o_c2ws"), (t.near_distances, "o_near"), (t.far_distances, "o_far"), (t.gt_distances, "o_gt"),
                 (t.rgbds, "o_rgbds"), (t.term_probs, "o_term_probs")):
        close(a, g[b], rtol=2e-6, atol=2e-6)
    for a, b in ((t.rgb_mask, "o_rgb_mask"), (t.depth_mask, "o_depth_mask"), (t.term_mask, "o_term_mask")):
        assert torch.equal(a.cpu(), g[b]), b
    # the segment-sphere test against the oracle's formula on every candidate pair
    pos_c = (g["positions"][g["active_field_ids"]] - g["c2w"][:3, 3]) @ g["c2w"][:3, :3]
    d = img[..., 3]
    ij = torch.nonzero(d)[g["d_subset_points"].long()]
    dv = d[ij[:, 0], ij[:, 1]]
    pts = torch.stack(((ij[:, 1].float() - scene.SV_CX) * dv / scene.SV_FX, -(ij[:, 0].float() - scene.SV_CY) * dv / scene.SV_FY, -dv), -1)
    hit = ops.target_sv_intersect(pos_c.to(DEV), pts.to(DEV), float(g["field_radius"])).cpu()
    sq = (pts * pts).sum(-1, keepdim=True)
    tt = ((pos_c[:, None, :] * pts).sum(-1, keepdim=True) / sq).clamp(0.0, 1.0)
    ref = ((pos_c[:, None, :] - pts * tt) ** 2).sum(-1) <= float(g["field_radius"]) ** 2
    assert int((hit != ref).sum()) <= 2, int((hit != ref).sum())          # pairs on the sphere to the last bit
    # own draws on the device: structural checks
    torch.manual_seed(5)
    t2 = r.sample_target_sv(img, g["c2w"], g["active_field_ids"], int(g["num_train_fields"]), R, camera=cam)
    assert t2.ijs.shape[1:] == (R, 2) and 1 <= t2.ijs.shape[0] == len(t2.field_ids) <= int(g["num_train_fields"])
    assert bool((t2.near_distances < t2.far_distances).all()) and bool(t2.term_mask.all())
    assert bool((t2.gt_distances > 0).all())                               # only pixels with depth are sampled


# (the 200-iteration "both trajectories improve" comparison that stood here is superseded by the G13 runs of
# tests/test_gpu_training_run.py: trained parameters against the real reference's trajectory, ensemble PSNR within 0.1 dB)


# ------------------------------------------------------------------ end to end: sampler -> train -> kNN render
def test_end_to_end_synthetic_fit():
    """examples/fit_synthetic.py: keyframe store -> training-target sampler -> fused training step -> render_image.
    The loss must fall and the re-rendered keyframe must approach the synthetic scan."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_synthetic", os.path.join(root, "examples", "fit_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, psnr, derr = mod.main(iters=200, device=str(DEV), quiet=True)
    assert losses[-1] < 0.25 * losses[0], losses
    assert psnr > 14.0 and derr < 0.3, (psnr, derr)


# ------------------------------------------------------------------ randomised differential sweep
@pytest.mark.parametrize("seed", list(range(int(os.environ.get("NGM_FUZZ_SEEDS", "10")))))      # NGM_FUZZ_SEEDS=200: a longer sweep
def test_fused_train_random_shapes_vs_oracle(seed):
    """Random batch shapes, sample counts, widths, layer counts and geometry modes against the oracle: exercises
    partial tiles, fields starting mid stash tile, S not a multiple of anything, every backward kernel variant."""
    g = torch.Generator().manual_seed(1000 + seed)

    def ri(lo, hi):
        return int(torch.randint(lo, hi + 1, (1,), generator=g))
    F, R, n_c, n_g = ri(1, 6), ri(1, 90), ri(1, 14), ri(0, 14)
    wide = seed % 2 == 0
    fkw = dict(encoding="fourier", dim_enc=64 if wide else 32, num_layers=ri(1, 2))
    if seed % 5 == 3:
        fkw["skip_mode"] = "add"
    mode = ["nrgbd", "occupancy", "density"][seed % 3]
    if n_c + n_g < 2 and mode == "density":
        n_c += 1                                                   # density drops the last sample
    ragged_case(F, R, n_c, n_g, fkw, geometry_mode=mode, geometry_factor=20.0 if mode != "density" else 1.0)


# ------------------------------------------------------------------ checkpoint interchange (rm.py:2147-2173)
def test_checkpoint_in_reference_layout_renders_the_reference_image(tmp_path):
    """G14: a .pt written by the real reference (the dict of save_model, rm.py:2149-2156) for the map of G9.  A renderer
    with an EMPTY field set loads it and must render the reference's image; saving and re-loading changes nothing."""
    import os
    from conftest import GOLDEN
    g = load_golden("g9_render_image")
    w, h, fx, fy, cx, cy = [float(x) for x in g["cam"]]
    ckw = dict(num_samples_coarse=8, num_samples_depth_guided=16, eval_far_distance=float(g["eval_far"]),
               eval_num_samples=int(g["eval_num_samples"]))
    cam = Rr.Camera(int(w), int(h), fx, fy, cx, cy, pixel_center=0.0)
    r = make_renderer(dict(encoding="fourier", dim_enc=64, num_layers=2), ckw, 1)     # holds one unrelated field
    r.load_model(os.path.join(GOLDEN, "g14_checkpoint_reference_layout.pt"))
    assert r._global_map_dict["num"] == 3 and r._model.all_fields_params["_linears.0.weight"].is_cuda
    r.eval()
    rgbd, dvar = r.render_image(g["c2w"].to(DEV), cam, u=g["u"].to(DEV))
    close(rgbd, g["rgbd"], rtol=5e-4, atol=5e-5)
    close(dvar, g["dvar"], rtol=5e-4, atol=5e-5)
    r.save_model(str(tmp_path / "again.pt"))
    r2 = make_renderer(dict(encoding="fourier", dim_enc=64, num_layers=2), ckw, 0)
    r2.load_model(str(tmp_path / "again.pt"))
    r2.eval()
    rgbd2, _ = r2.render_image(g["c2w"].to(DEV), cam, u=g["u"].to(DEV))
    assert torch.equal(rgbd, rgbd2)
    # a loaded map trains: moments start from zero (the reference does not checkpoint them either)
    _, _, t = synth_target(3, 16, seed=2)
    t["c2ws"] = t["c2ws"].clone()
    t["c2ws"][..., :3, 3] += (g["pos"] - synth_target(3, 1, seed=2)[0])[:, None]
    out = r2.optimization_iteration(make_target(t, torch.arange(3)), seed=1, update=True)
    assert torch.isfinite(out["combined"]) and r2._step == 1
