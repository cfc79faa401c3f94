"""-m gpu tests that close the gaps the round-3 review named ("harden green"):

  * oracle comparisons AT THE METRIC SIZE (M1 = 8 fields x 512 rays x (64 + 64) samples, explicit jitter): prediction, loss and
    every gradient, Fourier network and the reference's default hash network, at the usual bars;
  * BASELINE config 4 (8192 rays x 256 samples, fp16 weights) at full size WITH fp16 storage: properties + bitwise equality to
    fp32 storage on representable weights;
  * the timed path's random numbers pinned: a host Philox4x32-10 with the kernels' (seed, offset, counter) mapping reproduces the
    in-kernel draws bit for bit (sample distances and predictions) for three offsets;
  * which arithmetic the hash network's forward and backward resolved to."""
import numpy as np
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_common import (DEV, NRGBD, close, grad_close, host_philox_draws, make_renderer, make_target,  # noqa: E402
                        ragged_case, synth_target)
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402
from test_gpu_configs import FOURIER, HASH, _perturb, _properties  # noqa: E402
from test_gpu_parity import _permuto_train_case  # noqa: E402


# ------------------------------------------------------------------------------------------------ (a) metric size vs oracle
def test_m1_size_fourier_train_step_vs_oracle():
    """the bench line's batch shape through the bench line's kernels (fused forward, bf16-split backward with the fused
    compositing backward), against the CPU oracle on the same explicit jitter: 524 288 samples"""
    ragged_case(8, 512, 64, 64, dict(FOURIER), max_neutralised=0.02)     # >= 98 % of the batch is compared (measured: 99.9 %)
    L = K.lib()
    assert L.ngm_debug_last_bwd_variant() == 3 and L.ngm_debug_last_comp_fused() == 1
    assert L.ngm_debug_last_matmul(0) == K.MATMUL["bf16x3"]


@pytest.mark.parametrize("atomics", ["exact", "float"])
def test_m1_size_hash_train_step_vs_oracle(atomics):
    """the reference's default network on the same batch (tolerances of the hash tests: forward 2e-3 / 2e-4, gradients per tensor /
    level group: gpu_common.HASH_BARS); `float`: the opt-in fp32 LDS atomics of the table gradient, at the same bars"""
    _permuto_train_case(8, 512, 64, 64, "auto", max_neutralised=0.02, atomics=atomics)
    assert K.lib().ngm_debug_last_comp_fused() == 1


# ------------------------------------------------------------------------------------------------ (d) resolved arithmetic
def test_hash_network_resolved_arithmetic():
    """hash forward: fp32 MFMA (the split forward for 32-wide layers was measured and not kept); hash backward under `auto`:
    k_hash_mlp_bwd on the bf16 split (variant 5); under `mlp_matmul: f32`: k_field_bwd16 (variant 1).  No silent fallback."""
    F, R = 2, 40
    pos, quat, t = synth_target(F, R, seed=3)
    for mm, fwd, bwd in (("auto", "f32", 5), ("f32", "f32", 1)):
        r = make_renderer(HASH, dict(num_samples_coarse=8, num_samples_depth_guided=16, mlp_matmul=mm), F)
        _perturb(r)
        r.set_field_poses(pos.to(DEV), quat.to(DEV))
        r.optimization_iteration(make_target(t, torch.arange(F)), seed=1, update=False)
        assert K.lib().ngm_debug_last_matmul(0) == K.MATMUL[fwd], (mm, K.lib().ngm_debug_last_matmul(0))
        assert K.lib().ngm_debug_last_bwd_variant() == bwd, (mm, K.lib().ngm_debug_last_bwd_variant())


# ------------------------------------------------------------------------------------------------ (b) cfg4, fp16 storage
def test_cfg4_8192_rays_x_256_samples_fp16_weight_storage():
    F, R = 16, 512
    ckw = dict(num_samples_coarse=128, num_samples_depth_guided=128)
    ra = make_renderer(FOURIER, ckw, F)                                                  # fp32 storage
    _perturb(ra)
    with torch.no_grad():                                                                # every weight fp16-representable
        for k, v in ra._model.all_fields_params.items():
            if k not in K.NO_GRAD_PARAMS and k != "_neus_sd":
                v.copy_(v.to(torch.float16).float())
    rb = make_renderer({**FOURIER, "weight_dtype": "float16"}, ckw, F, {k: v for k, v in ra._model.all_fields_params.items()})
    assert rb._model.lp_fields_params["_linears.0.weight"].dtype == torch.float16
    pos, quat, t = synth_target(F, R, seed=2)
    tgt = make_target(t, torch.arange(F))
    outs = []
    for r in (ra, rb):
        r.set_field_poses(pos.to(DEV), quat.to(DEV))
        o = _properties(r, tgt)                                                          # finite, term in [0,1], deterministic
        assert K.lib().ngm_debug_last_bwd_variant() == 3
        outs.append((o["prediction"].rgbds.clone(), {k: v.clone() for k, v in o["grads"].items()}, float(o["combined"])))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][2] == outs[1][2]             # bitwise: storage only, fp32 arithmetic
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
    replay = rb.capture_iteration(tgt, seed=3)                                           # and it trains with the fp16 copies refreshed
    losses = [float(replay()["combined"]) for _ in range(20)]
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    for k, v in rb._model.all_fields_params.items():
        if k not in K.NO_GRAD_PARAMS and k != "_neus_sd":
            assert torch.equal(rb._model.lp_fields_params[k], v.to(torch.float16)), k


# ------------------------------------------------------------------------------------------------ (c) Philox pinned
def _dists(r, F, R, S):
    w = r._workspace(F, R)
    g, d = torch.empty(F, R, S, device=DEV), torch.empty(F, R, S, device=DEV)
    K.check(K.lib().ngm_render_read_samples(K.C.byref(r._fc), K.C.byref(r._rc_train), F, R, S, w["ws"].data_ptr(), g.data_ptr(),
                                            d.data_ptr(), ops._stream()), "ngm_render_read_samples")
    return d


@pytest.mark.parametrize("n_c,n_g", [(64, 64), (8, 16)])
def test_in_kernel_philox_equals_host_philox(n_c, n_g):
    """What bench.py times draws its jitter in the kernel.  The same iteration fed with the HOST restatement's draws for the
    same (seed, offset) must give bitwise the same sample distances, predictions and gradients -- for three offsets (the
    offset is the device iteration counter the captured graph advances)."""
    F, R, seed = 3, 130, 0x1234567 + n_c
    r = make_renderer(FOURIER, dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g), F)
    _perturb(r)
    pos, quat, t = synth_target(F, R, seed=8)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    tgt = make_target(t, torch.arange(F))
    for offset in (0, 1, 77):
        r._step = offset
        if r._step_dev is not None:
            r._step_dev.fill_(offset)
        a = r.optimization_iteration(tgt, seed=seed, update=False)                       # in-kernel Philox
        da, pa = _dists(r, F, R, n_c + n_g).clone(), a["prediction"].rgbds.clone()
        ga = {k: v.clone() for k, v in a["grads"].items()}
        assert int(r._step_dev.item()) == offset
        u_c, u_g = host_philox_draws(seed, offset, F, R, n_c, n_g)
        b = r.optimization_iteration(tgt, u_c.to(DEV), u_g.to(DEV), update=False)        # explicit draws
        db = _dists(r, F, R, n_c + n_g)
        assert torch.equal(da, db), offset
        assert torch.equal(pa, b["prediction"].rgbds), offset
        for k in ga:
            assert torch.equal(ga[k], b["grads"][k]), (offset, k)
    # the standalone sampler operator draws from the same stream (offset 0)
    rc = K.render_cfg(num_samples_coarse=n_c, num_samples_guided=n_g, fx=554.2562584220408, fy=554.2562584220408, cx=319.5, cy=239.5)
    u_c, u_g = host_philox_draws(seed, 0, F, R, n_c, n_g)
    near, far, gt = t["near"].to(DEV), t["far"].to(DEV), t["gt"].to(DEV)
    _, t1, _ = ops.sample_rays(rc, t["ijs"].to(DEV), near, far, gt, seed=seed)
    _, t2, _ = ops.sample_rays(rc, t["ijs"].to(DEV), near, far, gt, u_c.to(DEV), u_g.to(DEV))
    assert torch.equal(t1, t2)


# ------------------------------------------------------------------------------------------------ kNN evaluation, large maps
@pytest.mark.parametrize("NF,K_,P,layout", [(10000, 2, 6000, "cover_grid"), (10000, 4, 4000, "random"), (5000, 2, 6000, "two_rooms"),
                                            (40000, 2, 3000, "cover_grid"), (20000, 6, 3000, "cover_grid"),      # K > 4 with a histogram of more than 64 KB of LDS
                                            (3000, 11, 3000, "random"), (20000, 14, 2000, "cover_grid")])         # K = 9..16: run-time K in the 16-slot instance
def test_knn_assignment_large_maps_vs_oracle(NF, K_, P, layout):
    """The nearest-field assignment bins the centres into a uniform grid on the device and grows the block of cells around a
    point until the K-th neighbour is provably exact -- no limit on the number of fields (round 3: 4096).  10 000 fields on
    the reference's cover grid (rm.py:299: spacing 2 r / sqrt 3), random centres (sparse regions: several rings), two distant
    clusters (coarsened grid), and 40 000 fields (per-workgroup histograms no longer fit the LDS: global-atomic path)."""
    torch.manual_seed(NF + K_)
    fs = O.FieldSpec(encoding="fourier", dim_enc=32, num_layers=1)
    fc = K.field_cfg(encoding="fourier", dim_enc=32, num_layers=1)
    params = O.init_params(fs, NF, seed=NF % 1000, sigma=3.0)
    r = 1.0
    if layout == "cover_grid":
        n = int(round(NF ** (1 / 3))) + 1
        g = torch.arange(n) * (2 * r / 3 ** 0.5)
        pos = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[torch.randperm(n ** 3)[:NF]]
        pos = pos + 1e-3 * torch.randn(NF, 3)                       # no exact distance ties (unpinned in the reference)
        ext = float(g[-1])
        pts = torch.rand(P, 3) * (ext + 4) - 2                      # inside the map, at its border and outside
    elif layout == "random":
        pos = torch.rand(NF, 3) * 60                                 # ~0.05 centres per r^3: most points see few neighbours nearby
        pts = pos[torch.randint(0, NF, (P,))] + 0.7 * torch.randn(P, 3)
    else:
        pos = torch.cat([torch.rand(NF // 2, 3) * 8, torch.rand(NF - NF // 2, 3) * 8 + 500.0])
        pts = torch.cat([torch.rand(P // 2, 3) * 10 - 1, torch.rand(P - P // 2, 3) * 10 + 499.0])
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1)
    ref = O.field_set_forward_knn(pts, pos, quat, params, fs, num_knn=K_, distance_factor=10.0, outside_value=1.0)
    out = ops.field_eval_knn(fc, {k: v.to(DEV) for k, v in params.items()}, pts.to(DEV), pos.to(DEV), quat.to(DEV), K_, 10.0, 1.0)
    n_in = int((ref != 1.0).any(-1).sum())
    assert n_in > P // 10, n_in                                      # the case does exercise fields
    close(out, ref, rtol=3e-4, atol=3e-5)


# ------------------------------------------------------------------------------------------------ standalone encode stage
@pytest.mark.parametrize("enc", ["permuto", "fourier", "nerf"])
def test_standalone_encode_stage_vs_oracle(enc):
    """ngm_encode_fwd: the positional encoding alone, (F,P,3) -> (F,P,dim_enc), against the oracle's
    `encode` on posed fields with unit-cube scaling (hash: the oracle restates the published lattice algorithm -- unpinned)."""
    torch.manual_seed(3)
    F, P = 3, 1111
    if enc == "permuto":
        fs = O.FieldSpec(**HASH)
        fc = K.field_cfg(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
    elif enc == "fourier":
        fs = O.FieldSpec(**FOURIER)
        fc = K.field_cfg(encoding="fourier", dim_enc=64, num_layers=2)
    else:
        fs = O.FieldSpec(encoding="nerf", num_octaves=8, num_layers=1)
        fc = K.field_cfg(encoding="nerf", num_octaves=8, num_layers=1)
    params = O.init_params(fs, F, seed=2)
    if enc == "permuto":
        params["_encoding.lattice_values"] += 0.1 * torch.randn_like(params["_encoding.lattice_values"])
    pos = 0.5 * torch.randn(F, 3)
    quat = torch.nn.functional.normalize(torch.randn(F, 4), dim=-1)
    pts = pos[:, None] + 0.6 * torch.randn(F, P, 3)
    ref = O.encode(O.world_to_field(pts, pos, quat, 1.0, "unit_cube"), params, fs)
    out = ops.encode(fc, {k: v.to(DEV) for k, v in params.items()}, pts.to(DEV), pos.to(DEV), quat.to(DEV))
    assert out.shape == ref.shape
    # hash: the finest levels scale positions by 1e4, so the fp32 rounding of the world -> field transform (1e-7) moves a
    # barycentric weight by 1e-3 and a feature (lattice values ~0.1) by a few 1e-3 where it matters; 99 % of the features
    # agree to 2e-4 (the encoding is continuous across simplex faces, so nothing jumps).  These bars measure that input
    # conditioning; the kernel's own arithmetic is held to 16 eps of the table values in test_gpu_permuto_exact.py
    tol = dict(permuto=(2e-3, 6e-3), fourier=(2e-4, 2e-5), nerf=(1e-2, 2e-3))[enc]
    close(out, ref, rtol=tol[0], atol=tol[1])
    if enc == "permuto":
        ok = (out.cpu() - ref).abs() <= 2e-4 + 2e-3 * ref.abs()
        assert float(ok.float().mean()) > 0.99
        assert float((out.cpu()[..., :16] - ref[..., :16]).abs().max()) < 2e-4      # the eight coarser levels: tight


# ------------------------------------------------------------------------------------------------ variance-weighted losses
@pytest.mark.parametrize("geom", ["nrgbd", "occupancy"])
@pytest.mark.parametrize("photo,depth", [("gaussian_nll", "gaussian_nll"), ("l2", "laplacian_nll"), ("gaussian_nll", "huber")])
@pytest.mark.parametrize("F,R,n_c,n_g", [(3, 37, 5, 2), (2, 130, 20, 4)])
def test_nll_loss_modes_ragged_vs_oracle(F, R, n_c, n_g, photo, depth, geom):
    """losses.py:30-36, 64-75 on ragged shapes (rays of 7 and 24 samples against 32-sample tiles): prediction, loss and every
    gradient against the oracle, whose restatement of these modes is pinned by the G20 fixtures of the real reference.  The
    gradient reaches the samples through the rendered variances as well (k_stash_bwd; the fused compositing backward is not
    used for these modes).  Conditioning: the NLL divides by the rendered variance, which is a cancellation (sum w (c - C)^2)
    and vanishes where one sample takes all the weight -- there e^2 / V^2 amplifies the fp32 rounding of V without bound in
    ANY implementation; rays whose variances fall below 1e-4 are therefore taken out of the loss (depth mask off): 19-39 of
    the masked rays stay in.  The photometric gaussian_nll instances all sit on the L1 side of its switch (random target
    colours: mean colour NLL 434 to 750, losses.py:34-35), so here only the DEPTH variance carries gradient; the NLL side is
    tests/test_gpu_loss_terms.py."""
    from gpu_common import kink_free_draws
    torch.manual_seed(F * 1000 + R)
    fkw = dict(FOURIER)
    ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode=geom,
               geometry_factor=20.0, photometric_loss=photo, depth_loss=depth)
    pos, quat, t = synth_target(F, R, seed=R)
    fs = O.FieldSpec(**fkw)
    rs = O.RenderSpec(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, geometry_mode=geom,
                      geometry_factor=20.0, photometric_loss=photo, depth_loss=depth)
    params = O.init_params(fs, F, seed=R, sigma=3.0)
    u_c, u_g = torch.rand(F, R, n_c), torch.rand(F, R, n_g)
    u_c, u_g, t = kink_free_draws(t, pos, quat, params, fs, rs, u_c, u_g)
    with torch.no_grad():
        p0 = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, params, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    thin = (p0["color_vars"].min(-1).values < 1e-4) | (p0["depth_vars"] < 1e-4)
    t["depth_mask"] = t["depth_mask"] & ~thin
    assert int((t["depth_mask"] & (p0["term_probs"] > 0.8)).sum()) >= 5, "too few well-conditioned rays left"
    po = {k: v.clone().requires_grad_() for k, v in params.items()}
    pred = O.render_ijs(t["ijs"], t["c2ws"], NRGBD, pos, quat, po, fs, rs, t["near"], t["far"], t["gt"], u_c, u_g)
    loss = O.compute_losses(pred, t["rgbds"], t["depth_mask"], t["term_mask"], t["term_probs"], rs)
    loss["combined"].backward()
    r = make_renderer(fkw, ckw, F, params)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    res = r.optimization_iteration(make_target(t, torch.arange(F)), u_c.to(DEV), u_g.to(DEV), update=False)
    assert K.lib().ngm_debug_last_comp_fused() == 0 and K.lib().ngm_debug_last_bwd_variant() == 3
    close(res["prediction"].rgbds, pred["rgbds"].detach())
    close(res["prediction"].color_vars, pred["color_vars"].detach(), rtol=1e-3, atol=1e-6)
    close(res["prediction"].depth_vars, pred["depth_vars"].detach(), rtol=1e-3, atol=1e-6)
    for k in ("photometric_" + photo, "depth_" + depth, "combined"):
        close(res[k], loss[k].detach(), rtol=2e-3, atol=1e-5)
    for k in po:
        grad_close(res["grads"][k], po[k].grad, 5e-3, k)


# ------------------------------------------------------------------------------------------------ fused image path
def _image_cases():
    cases = [("nrgbd", 24, 2, 1000, True, "fourier"), ("nrgbd", 640, 2, 700, False, "fourier"),
             ("density", 96, 3, 4096, False, "fourier"), ("occupancy", 64, 1, 333, True, "fourier"),
             ("neus", 40, 2, 512, False, "fourier"), ("nrgbd", 128, 4, 600, False, "hash"),
             ("nrgbd", 64, 2, 2048, True, "fourier_f32"), ("occupancy", 192, 7, 900, False, "fourier"), ("nrgbd", 50, 5, 640, True, "fourier")]
    import random
    rnd = random.Random(77)                       # NGM_FUZZ_IMAGE=40: that many random combinations on top
    for _ in range(int(os.environ.get("NGM_FUZZ_IMAGE", "0"))):
        cases.append((rnd.choice(["nrgbd", "occupancy", "density", "neus"]), rnd.choice([1, 7, 33, 64, 100, 128, 256, 320, 640]),
                      rnd.randint(1, 8), rnd.choice([257, 512, 1000, 4096]), rnd.random() < 0.4, rnd.choice(["fourier", "fourier", "hash"])))
    return cases


@pytest.mark.parametrize("geo,S,K_,block,explicit_u,net", _image_cases())
def test_fused_image_path_equals_the_staged_entry_points(geo, S, K_, block, explicit_u, net):
    """render_pixels as ONE call (ngm_render_eval_knn: samples drawn inside the neighbour assignment, blend inside the
    quadrature, grid over the centres built once) against the staged per-block entry points (ngm_sample_rays_world ->
    ngm_field_eval_knn -> ngm_composite_fwd_packed): the same blocks, draws and arithmetic, so the images are EQUAL bit for
    bit -- explicit jitter or in-kernel Philox, ragged last block, every geometry mode, K = 1..3, rays that leave every field
    and (camera inside the map, far plane behind it) samples on both sides of the fields; the default hash network and the
    exact-fp32 evaluation kernel as well."""
    torch.manual_seed(S)
    g = torch.arange(-1.0, 1.01, 0.5)
    pos = torch.stack(torch.meshgrid(g, g, torch.tensor([-2.0, -1.5]), indexing="ij"), -1).reshape(-1, 3)
    pos = pos + 1e-3 * torch.randn_like(pos)
    NF = pos.shape[0]
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1)
    ckw = dict(num_samples_coarse=8, num_samples_depth_guided=16, geometry_mode=geo, eval_near_distance=0.0,
               eval_far_distance=4.0, eval_num_samples=S, pixel_block_size=block, eval_ray_block=block)
    if net == "fourier_f32":
        ckw["mlp_matmul"] = "f32"                                          # the exact-fp32 MFMA evaluation kernel (four waves)
    r = make_renderer(HASH if net == "hash" else FOURIER, ckw, NF)
    r._model._num_knn = K_
    _perturb(r)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    r.eval()
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    begin, end = 640 * 200 + 17, 640 * 200 + 17 + 2500                      # not aligned to anything
    u = torch.rand(640 * 480, S, device=DEV) if explicit_u else None
    outs = []
    for fused in (True, False):
        r.eval_fused = fused
        outs.append(r.render_pixels(c2w.to(DEV), begin, end, u=u, seed=11))
    assert outs[0][0].shape == (end - begin, 4) and torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    if geo == "nrgbd":
        assert bool((outs[0][0][:, :3] != outs[0][0][:1, :3]).any())        # the image is not one constant colour


def test_knn_path_does_not_depend_on_stale_workspace_contents():
    """tools/knn_stress.py: the caching allocator's free blocks (which the workspace is carved from) are filled with random bits
    before every call; maps of 3 .. 40 000 fields, K = 1 .. 4; every blended output against a brute-force fp64 neighbour
    search (constant-output fields, so the output identifies the neighbours and their weights)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import knn_stress
    assert knn_stress.main(10) == 0


def test_fused_image_entry_with_per_ray_poses_and_bounds():
    """ngm_render_eval_knn with everything per ray (c2ws (N,4,4), near (N,), far (N,)) and in-kernel Philox, against the three
    staged operators called block by block with the seeds the entry documents (seed + block start): equal bit for bit."""
    torch.manual_seed(5)
    N, S, K_, block, seed = 3000, 64, 2, 1024, 77
    g = torch.arange(-1.0, 1.01, 0.5)
    pos = torch.stack(torch.meshgrid(g, g, torch.tensor([-2.0, -1.5]), indexing="ij"), -1).reshape(-1, 3)
    pos = (pos + 1e-3 * torch.randn_like(pos)).to(DEV)
    NF = pos.shape[0]
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1).to(DEV)
    r = make_renderer(FOURIER, dict(num_samples_coarse=8, num_samples_depth_guided=16), NF)
    _perturb(r)
    params = {k: v for k, v in r._model.kernel_params().items() if k != "_neus_sd"}
    fc = r._fc
    rc = K.render_cfg(num_samples_coarse=S, num_samples_guided=0, fx=554.2562584220408, fy=554.2562584220408, cx=319.5, cy=239.5)
    ijs = torch.stack((torch.randint(0, 480, (N,)), torch.randint(0, 640, (N,))), -1).to(DEV)
    c2ws = torch.eye(4).repeat(N, 1, 1)
    c2ws[:, :3, 3] = 0.2 * torch.randn(N, 3)
    c2ws = c2ws.to(DEV)
    near, far = (0.5 * torch.rand(N)).to(DEV), (3.0 + torch.rand(N)).to(DEV)
    rgbd, cv, dv, term = ops.render_eval_knn(fc, rc, params, ijs, c2ws, pos, quat, K_, 10.0, 1.0, near=near, far=far, seed=seed,
                                             ray_block=block)
    outs = []
    for s0 in range(0, N, block):
        sl = slice(s0, s0 + block)
        pc, pw, dist = ops.sample_rays_world(rc, ijs[sl][None], c2ws[sl][None], near[sl][None], far[sl][None], seed=seed + s0)
        o4 = ops.field_eval_knn(fc, params, pw.view(-1, 3), pos, quat, K_, 10.0, 1.0)
        outs.append(ops.composite_packed(rc, o4, dist.view(-1, S), pc.view(-1, S, 3)))
    for i, t in enumerate((rgbd, cv, dv, term)):
        assert torch.equal(t, torch.cat([o[i] for o in outs])), i
    assert bool((term > 0.5).any()) and bool((rgbd[:, :3] != rgbd[:1, :3]).any())   # the rays do meet fields, and different ones


@pytest.mark.parametrize("enc,P", [("fourier", 1111), ("fourier", 70000), ("permuto", 1500), ("permuto", 40000), ("nerf", 300)])
def test_standalone_encode_backward_stage_vs_oracle_autograd(enc, P):
    """ngm_encode_bwd: d_enc (F,P,dim_enc) -> the encoding's own parameter gradients, against autograd
    through the oracle's `encode` (Fourier: d sin(W x) / dW; hash: the table gradient, through the training step's
    k_hash_grad -- one chunk and several chunks per level; NeRF octaves: no parameters, nothing returned)."""
    torch.manual_seed(7)
    F = 3
    if enc == "permuto":
        fs = O.FieldSpec(**HASH)
        fc = K.field_cfg(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
        name = "_encoding.lattice_values"
    elif enc == "fourier":
        fs = O.FieldSpec(**FOURIER)
        fc = K.field_cfg(encoding="fourier", dim_enc=64, num_layers=2)
        name = "_encoding._linear.weight"
    else:
        fs = O.FieldSpec(encoding="nerf", num_octaves=8, num_layers=1)
        fc = K.field_cfg(encoding="nerf", num_octaves=8, num_layers=1)
        name = None
    params = O.init_params(fs, F, seed=2)
    if enc == "permuto":
        params[name] += 0.1 * torch.randn_like(params[name])
    pos = 0.5 * torch.randn(F, 3)
    quat = torch.nn.functional.normalize(torch.randn(F, 4), dim=-1)
    pts = pos[:, None] + 0.6 * torch.randn(F, P, 3)
    d_enc = torch.randn(F, P, fc.dim_enc)
    got = ops.encode_bwd(fc, {k: v.to(DEV) for k, v in params.items()}, pts.to(DEV), d_enc.to(DEV), pos.to(DEV), quat.to(DEV))
    if name is None:
        assert got == {}
        return
    pr = {k: v.clone().requires_grad_(k == name) for k, v in params.items()}
    (O.encode(O.world_to_field(pts, pos, quat, 1.0, "unit_cube"), pr, fs) * d_enc).sum().backward()
    ref = pr[name].grad
    assert got[name].shape == ref.shape
    # sums of up to 70 000 terms of either sign: compared against the gradient's scale, as every other gradient test is
    if enc == "permuto":
        from gpu_common import hash_grad_close
        hash_grad_close(got[name], ref, name)
    else:
        grad_close(got[name], ref, 2e-3, name)


# ------------------------------------------------------------------------------------------------ activation stash modes
# (round 5: a process-wide debug switch; ABI 10: `activation_stash` is part of a renderer's field configuration)
STASH = {0: "full", 1: "half"}


@pytest.mark.parametrize("stash_mode", [0, 1], ids=lambda m: STASH[m])
@pytest.mark.parametrize("shape", [(1, 256, 16, 16), (3, 41, 9, 5), (2, 96, 8, 16), (1, 7, 64, 64), (4, 130, 2, 5)])
def test_stash_modes_ragged_train_step_vs_oracle(stash_mode, shape):
    """The two activation-stash modes of the two-hidden-layer split path (include/ngm_hip.h, ngm_activation_stash): both layers'
    outputs / layer 0's only with layer 1 recomputed on the matrix pipe (k_field_bwd_b3<HS>) -- each against the oracle at the
    usual bars on ragged shapes (rays of 7 .. 128 samples against 32-sample tiles, fields whose sample count is not a multiple
    of 32), and the mode that really ran is read back from the library."""
    F, R, n_c, n_g = shape
    ragged_case(F, R, n_c, n_g, dict(FOURIER), activation_stash=STASH[stash_mode])
    L = K.lib()
    assert L.ngm_debug_last_bwd_variant() == 3 and L.ngm_debug_last_stash_mode() == stash_mode


@pytest.mark.parametrize("enc", ["nerf", "none61"])
def test_stash_modes_other_encodings(enc):
    # (ten octaves: 60 features -- the stash exists for 49..64-wide layers; eight octaves = 48 run the recompute kernels)
    fkw = dict(encoding="nerf", num_octaves=10, num_layers=2) if enc == "nerf" else dict(encoding="fourier", dim_enc=61, num_layers=2)
    # ten octaves put arguments up to 2^9 pi into fp32 sines: the forward tolerance of the NeRF fixtures (G4 / G6), not 2e-4
    ragged_case(3, 70, 6, 7, fkw, fwd_tol=dict(rtol=5e-3, atol=5e-4) if enc == "nerf" else None, grad_tol=5e-3 if enc == "nerf" else 2e-3,
                activation_stash="half")
    assert K.lib().ngm_debug_last_stash_mode() == 1


def test_stash_modes_bitwise_deterministic_and_close_to_full():
    """200 launches of a ragged batch give bitwise the same gradients; the gradients agree with the full-stash kernel's to
    fp32 round-off (the recomputed layer is the same arithmetic in another summation order).  The two renderers live in ONE
    process with DIFFERENT stash modes and are used alternately (ABI 10: the mode travels in ngm_field_cfg, workspaces are
    sized per configuration -- as a process-wide switch the second renderer's mode broke the first one's cached workspace)."""
    F, R = 3, 97
    pos, quat, t = synth_target(F, R, seed=5)
    ckw = dict(num_samples_coarse=11, num_samples_depth_guided=13, termination_weight=0.3)
    r = make_renderer(FOURIER, {**ckw, "activation_stash": "half"}, F)
    _perturb(r)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    tgt = make_target(t, torch.arange(F))
    first = {k: v.clone() for k, v in r.optimization_iteration(tgt, seed=9, update=False)["grads"].items()}
    for _ in range(200):
        g = r.optimization_iteration(tgt, seed=9, update=False)["grads"]
        for k in first:
            assert torch.equal(g[k], first[k]), k
    assert K.lib().ngm_debug_last_stash_mode() == 1
    r0 = make_renderer(FOURIER, ckw, F)                                  # does not name a mode: the default, full
    for k, v in r._model.all_fields_params.items():
        r0._model.all_fields_params[k].copy_(v)
    r0.set_field_poses(pos.to(DEV), quat.to(DEV))
    full = {k: v.clone() for k, v in r0.optimization_iteration(tgt, seed=9, update=False)["grads"].items()}
    assert K.lib().ngm_debug_last_stash_mode() == 0
    for k in first:
        grad_close(first[k], full[k], 2e-5, "vs full stash " + k)
    ws_half, ws_full = r._workspace(F, R)["wsb"], r0._workspace(F, R)["wsb"]
    assert ws_half < ws_full                                             # each sized for its own configuration
    for _ in range(3):                                                    # alternate: cached workspaces, both modes, one process
        g1 = r.optimization_iteration(tgt, seed=9, update=False)["grads"]
        assert K.lib().ngm_debug_last_stash_mode() == 1
        for k in first:
            assert torch.equal(g1[k], first[k]), k
        g0 = r0.optimization_iteration(tgt, seed=9, update=False)["grads"]
        assert K.lib().ngm_debug_last_stash_mode() == 0
        for k in first:
            assert torch.equal(g0[k], full[k]), k


def test_backward_the_plan_refuses_launches_nothing():
    """A forward that wrote a half stash, then a backward whose configuration says f32: no kernel reads a half stash in fp32
    MFMA, so the backward plan refuses (NGM_E_INVALID) -- before k_stash_bwd, which would have overwritten the forward's stash
    and advanced the device counter.  Workspace, counters, parameters, moments and the gradient arena keep their bits, and
    the renderer's next iteration is that of a renderer which never saw the refusal.  (2, 33, 1, 1): one ragged tile per field."""
    F, R = 2, 33
    pos, quat, t = synth_target(F, R, seed=5)
    ckw = dict(num_samples_coarse=1, num_samples_depth_guided=1, termination_weight=0.3, activation_stash="half", mlp_matmul="auto")
    r, ref = make_renderer(FOURIER, ckw, F), make_renderer(FOURIER, ckw, F)
    _perturb(r)
    for k, v in r._model.all_fields_params.items():
        ref._model.all_fields_params[k].copy_(v)
    tgt = make_target(t, torch.arange(F))
    for x in (r, ref):
        x.set_field_poses(pos.to(DEV), quat.to(DEV))
        x.optimization_iteration(tgt, seed=9, update=False)              # workspace, gradient arena and moments exist from here on
    assert K.lib().ngm_debug_last_bwd_variant() == 3 and K.lib().ngm_debug_last_stash_mode() == 1
    ctx = r._iteration_forward(tgt, seed=9)
    w = ctx["w"]

    def state():
        torch.cuda.synchronize()
        s = dict(ws=w["ws"], step_dev=r._step_dev, gflat=w["gflat"], **{"p." + k: v for k, v in r._model.all_fields_params.items()})
        for k, st in r._optim_state.items():
            s["m." + k], s["v." + k] = st["exp_avg"], st["exp_avg_sq"]
        return {k: v.clone() for k, v in s.items()}, r._step

    before, step = state()
    fc32 = K.FieldCfg.from_buffer_copy(ctx["fc"])
    fc32.matmul_mode = K.MATMUL["f32"]
    with pytest.raises(K.NgmError) as ex:
        r._iteration_backward(dict(ctx, fc=fc32), update=True)
    assert ex.value.code == K.NGM_E_INVALID
    after, step_after = state()
    assert step_after == step
    for k in before:
        assert torch.equal(after[k], before[k]), k
    got = r.optimization_iteration(tgt, seed=9, update=False)["grads"]
    want = ref.optimization_iteration(tgt, seed=9, update=False)["grads"]
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("num_knn,S", [(6, 64), (8, 640), (5, 40), (10, 64), (16, 40)])
def test_image_path_with_more_than_four_neighbours(num_knn, S):
    """K = 5..8: assignment, evaluation and -- since the end of round 5 -- the blend inside the one-call image path's quadrature
    take up to 8 neighbours (whole-ray and generic quadrature kernels, two wave steps gathered at a time instead of five):
    the fused call runs and equals the three staged entry points per block bit for bit."""
    from neural_graph_mapping_amd import models as M
    from neural_graph_mapping_amd import renderer as Rr
    torch.manual_seed(3)
    g = torch.arange(-1.0, 1.01, 0.5)
    pos = torch.stack(torch.meshgrid(g, g, torch.tensor([-2.5, -2.0]), indexing="ij"), -1).reshape(-1, 3)
    NF = pos.shape[0]
    quat = torch.nn.functional.normalize(torch.randn(NF, 4), dim=-1)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=32, mu=0.0, sigma=3.0, raw_coords=True), num_layers=1, dim_out=4),
        num_knn=num_knn, distance_factor=10.0, outside_value=1.0, field_radius=0.6, scale_mode="unit_cube").to(DEV)
    cam = Rr.Camera(64, 48, 55.0, 55.0, 31.5, 23.5, pixel_center=0.0)
    r = Rr.NeuralGraphRenderer(model, cam, Rr.shipped_config(field_radius=0.6, eval_num_samples=S, eval_far_distance=4.0,
                                                           pixel_block_size=1000, eval_ray_block=1000), device=DEV)
    r.add_fields(NF)
    _perturb(r)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    r.eval()
    c2w = torch.eye(4, device=DEV)
    img, dv = r.render_image(c2w, seed=5)
    if num_knn <= 8:
        assert r.last_eval_path.startswith("fused") and not r.eval_fallbacks
    else:          # K = 9..16 (round 6): the one-call image path reports NGM_E_UNSUPPORTED once, the staged entry points serve the image
        assert r.last_eval_path.startswith("staged") and len(r.eval_fallbacks) == 1 and "[1,8]" in r.eval_fallbacks[0]
    r.eval_fused = False
    img2, dv2 = r.render_image(c2w, seed=5)
    assert torch.equal(img, img2) and torch.equal(dv, dv2)
    if num_knn > 8:                                  # ... and equals the oracle's blend of K neighbours on the same samples
        from oracle import ngm_oracle as O
        ospec = O.FieldSpec(encoding="fourier", dim_enc=32, num_layers=1)
        pcpu = {k: v.cpu() for k, v in model.all_fields_params.items() if k != "_neus_sd"}
        pts = torch.rand(4000, 3) * torch.tensor([3.0, 3.0, 1.5]) + torch.tensor([-1.5, -1.5, -3.0])
        ref = O.field_set_forward_knn(pts, pos, quat, pcpu, ospec, num_knn=num_knn, distance_factor=10.0, outside_value=1.0, radius=0.6)
        out = model(pts.to(DEV), pos.to(DEV), quat.to(DEV), None, False)
        close(out, ref, rtol=3e-4, atol=3e-5)
    assert torch.isfinite(img).all() and float((img[..., :3] != 1.0).float().mean()) > 0.05      # the map is in view


_ONE_TILE_SCRIPT = r"""
import sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from gpu_common import DEV, make_renderer, make_target, synth_target
from test_gpu_configs import FOURIER, HASH, _perturb
out = {}
for n_c, n_g, F, net in ((8, 16, 1, FOURIER), (16, 16, 4, FOURIER), (5, 0, 2, FOURIER), (8, 16, 4, HASH), (3, 7, 1, HASH)):
    R = 512
    torch.manual_seed(1234 + n_c)          # the prototype's initialisation: the same network in both processes
    r = make_renderer(net, dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g), F)
    _perturb(r)
    pos, quat, t = synth_target(F, R, seed=31 + n_c)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    o = r.optimization_iteration(make_target(t, torch.arange(F)), seed=9, update=False)
    p = o["prediction"]
    from neural_graph_mapping_amd import _capi as K
    out[(n_c, n_g, F, net["encoding"])] = dict(one_tile=torch.tensor(K.lib().ngm_debug_last_fwd_one_tile()), rgbds=p.rgbds.cpu(), cv=p.color_vars.cpu(), dv=p.depth_vars.cpu(), term=p.term_probs.cpu(),
                             loss=o["combined"].cpu(), **{"g::" + k: v.cpu() for k, v in o["grads"].items()})
torch.save(out, sys.argv[3])
"""


def test_one_tile_wave_step_equals_the_two_tile_step_bitwise(tmp_path):
    """Round 6: batches of at most 32 samples per wave (one field x 512 rays x 24 samples: a 24-sample ray per wave; what a rank of
    an 8-GPU run sees) run the k_render_fwd instance whose wave step evaluates ONE 32-sample tile (eval_32).  The same iteration
    with that instance switched off (NGM_NO_HALF_STEP=1, read once per process: two child processes) must give the same BITS:
    predictions, loss, every gradient (the activation stash the backward reads is written by the step in question) -- for the
    Fourier network on the bf16 split and for the reference's default hash network (one encode_hash per step instead of two)."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    outs = []
    for tag, extra in (("half", {}), ("full", {"NGM_NO_HALF_STEP": "1"})):
        pth = str(tmp_path / f"{tag}.pt")
        env = {k: v for k, v in os.environ.items() if k != "NGM_NO_HALF_STEP"}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", _ONE_TILE_SCRIPT, os.path.dirname(here), here, pth], capture_output=True, text=True,
                           env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(pth))
    a, b = outs
    assert a.keys() == b.keys() and len(a) == 5
    for case in a:
        assert int(a[case]["one_tile"]) == 1 and int(b[case]["one_tile"]) == 0, case      # the switch did select the other instance
        for k in a[case]:
            if k == "one_tile":
                continue
            x, y = a[case][k], b[case][k]
            assert torch.equal(torch.isnan(x), torch.isnan(y)) and torch.equal(x.nan_to_num(), y.nan_to_num()), (case, k)
