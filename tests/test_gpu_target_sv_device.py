"""The single-view training-target sampler on the device (ngm_target_sample_sv, NeuralGraphRenderer.sample_target_sv_device,
capture_training_sv) against its numpy mirror (tests/_target_sv_host.py, held to the oracle in test_target_sv_host_cpu.py):
every decision exactly, the floats bit for bit; fixture G16 through the device path with its recorded draws; invariances,
degenerate inputs, uniformity of the ray draw, the captured training graph, guard bands."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _target_sv_host as SV  # noqa: E402
import scene  # noqa: E402
from gpu_common import DEV, close, make_renderer  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from test_gpu_safety import guard_bands  # noqa: E402

pytestmark = pytest.mark.gpu

M1 = dict(encoding="fourier", dim_enc=64, num_layers=2)
LOSS_KEYS = ("combined", "termination", "photometric_l1", "depth_huber", "freespace", "tsdf")


def dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to(DEV).contiguous()


def run_ops(s, active, num_points, T, R, seed, iteration=0, img=None, c2w=None, num_fields=None, **kw):
    """ops.target_sample_sv on the scene `s`; the outputs as numpy"""
    pos = dev(s["positions"])
    o = ops.target_sample_sv(dev(s["img"]) if img is None else img, dev(s["c2w"]) if c2w is None else c2w,
                             dev(active, torch.int64), pos, *s["intrinsics"], s["radius"],
                             pos.shape[0] if num_fields is None else num_fields, T, R, num_points=num_points, seed=seed,
                             iteration=iteration, **kw)
    torch.cuda.synchronize()
    return {k: int(v) if k in ("count", "num_used", "num_candidates") else v.cpu().numpy() for k, v in o.items()}


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if k != "pixels") and \
        np.array_equal(np.sort(a["pixels"]), np.sort(b["pixels"]))


# ------------------------------------------------------------------------------------------------ 1. exact against the mirror
@pytest.mark.parametrize("name", list(SV.CASES))
def test_exact_against_the_mirror(name):
    c = SV.CASES[name]
    s, m64 = SV.run_case(name, dt=np.float64)
    print(f"{name}: float64 margins (box, hit, gt) = {m64['margins']}")
    assert min(m64["margins"]) > SV.MARGIN, m64["margins"]               # a condition on the inputs
    _, m = SV.run_case(name)
    got = run_ops(s, c["active"], c["num_points"], c["T"], c["R"], c["seed"])
    for k in ("near", "far", "gt"):
        print(f"{name}: {k} max |device - mirror| = {np.abs(got[k][:m['count']] - m[k][:m['count']]).max():.3e}")
    SV.compare(got, m, float_tol=0.0)
    assert m["count"] > 0 and got["pixels"].shape == (c["num_points"],)
    if name == "boundary":                                               # hits == R is in, hits == R - 1 is out, in one call
        act, ids = list(c["active"]), list(got["field_ids"][:got["count"]])
        assert got["hits"][act.index(SV.BOUNDARY_IN)] == c["R"] and got["hits"][act.index(SV.BOUNDARY_OUT)] == c["R"] - 1
        assert SV.BOUNDARY_IN in ids and SV.BOUNDARY_OUT not in ids and got["num_candidates"] == got["count"]
    if name == "all_pixels":                                             # fewer valid pixels than num_points: all are used
        assert int(got["num_used"]) == int((s["img"][..., 3] != 0).sum()) and (got["pixels"] == -1).sum() == 65536 - int(got["num_used"])


# ------------------------------------------------------------------------------------------------ 2. both branches of the field draw
def test_both_branches_of_the_field_draw():
    c = SV.CASES["p2000"]
    s = SV.g16_scene()
    for T in (4, 12):
        m = SV.sample(s["img"], s["c2w"], s["positions"], np.array(c["active"]), s["radius"], s["intrinsics"], 2000, T, c["R"], 1, 0)
        got = run_ops(s, c["active"], 2000, T, c["R"], 1)
        SV.compare(got, m)
        n = m["count"]
        if T == 12:
            assert m["num_candidates"] == n <= T and list(got["field_ids"][:n]) == [g for g, h in zip(c["active"], m["hits"]) if h >= c["R"]]
        else:
            assert m["num_candidates"] > T == n
            keys = SV.field_keys(got["field_ids"][:n], 1, 0)
            assert (np.diff(keys.astype(np.float64)) > 0).all()          # key order
    # hits == R makes a candidate, hits == R - 1 does not: R runs over every field's hit count h and over h + 1
    hs = np.sort(SV.sample(s["img"], s["c2w"], s["positions"], np.array(c["active"]), s["radius"], s["intrinsics"], 2000, 12, 1, 1, 0)["hits"])
    for R in sorted({int(h) for h in hs if h > 0} | {int(h) + 1 for h in hs if h > 0}):
        m = SV.sample(s["img"], s["c2w"], s["positions"], np.array(c["active"]), s["radius"], s["intrinsics"], 2000, 12, R, 1, 0)
        got = run_ops(s, c["active"], 2000, 12, R, 1)
        SV.compare(got, m)
        assert m["num_candidates"] == int((hs >= R).sum())


# ------------------------------------------------------------------------------------------------ 3. G16 through the device path
def g16_renderer(s, positions=None, **ckw):
    pos = s["positions"] if positions is None else positions
    r = make_renderer(M1, dict(num_samples_coarse=4, num_samples_depth_guided=4, field_radius=s["radius"], **ckw), len(pos))
    quat = torch.zeros(len(pos), 4)
    quat[:, 0] = 1.0
    r.set_field_poses(dev(pos), quat.to(DEV))
    return r


CAM = Rr.Camera(scene.SV_W, scene.SV_H, scene.SV_FX, scene.SV_FY, scene.SV_CX, scene.SV_CY, pixel_center=0.0)


def test_g16_recorded_draws_through_the_device_path():
    s = SV.g16_scene()
    g = {k: torch.from_numpy(np.asarray(v)) for k, v in s["g"].items()}
    img = torch.from_numpy(s["img"])
    r = g16_renderer(s)
    T, R = int(g["num_train_fields"]), int(g["num_rays_per_field"])
    ij = torch.nonzero(img[..., 3])[g["d_subset_points"].long()]
    draws = dict(pixels=ij[:, 0] * scene.SV_W + ij[:, 1], subset_fields=g["d_subset_fields"], segments=g["d_segments"])
    t = r.sample_target_sv_device(img.to(DEV), g["c2w"].to(DEV), g["active_field_ids"], T, R, num_points=50000, camera=CAM, iteration=0,
                                  draws=draws)
    n = int(t.count)
    assert n == len(g["o_field_ids"]) and t.subset_observed is None and t.u_xy is None
    assert torch.equal(t.field_ids[:n].cpu(), g["o_field_ids"]) and torch.equal(t.ijs[:n].cpu(), g["o_ijs"].long())
    for a, b in ((t.near_distances, "o_near"), (t.far_distances, "o_far"), (t.gt_distances, "o_gt"), (t.rgbds, "o_rgbds"),
                 (t.term_probs, "o_term_probs")):
        close(a[:n], g[b], rtol=2e-6, atol=2e-6)
    close(t.c2ws[:n], g["o_c2ws"].expand(n, R, 4, 4), rtol=2e-6, atol=2e-6)
    for a, b in ((t.rgb_mask, "o_rgb_mask"), (t.depth_mask, "o_depth_mask"), (t.term_mask, "o_term_mask")):
        assert torch.equal(a[:n].cpu(), g[b]), b
    m = t.materialize()
    assert m.ijs.shape == (n, R, 2) and torch.equal(m.field_ids.cpu(), g["o_field_ids"])
    # hits against the existing intersect kernel on the same points (fields outside the points' box are not counted)
    pos_c = (g["positions"][g["active_field_ids"]] - g["c2w"][:3, 3]) @ g["c2w"][:3, :3]
    dv = img[ij[:, 0], ij[:, 1], 3]
    pts = torch.stack(((ij[:, 1].float() - scene.SV_CX) * dv / scene.SV_FX, -(ij[:, 0].float() - scene.SV_CY) * dv / scene.SV_FY, -dv), -1)
    in_box = ((pos_c - s["radius"]) <= pts.max(0)[0]).all(-1) & ((pos_c + s["radius"]) >= pts.min(0)[0]).all(-1)
    want = ops.target_sv_intersect(pos_c.to(DEV), pts.to(DEV), s["radius"]).sum(-1).cpu() * in_box
    assert torch.equal(t.hits.cpu().long(), want.long())
    # the draws come back in the conventions of sample_target_sv(draws=...)
    d = t.draws()
    assert torch.equal(d["subset_points"].cpu(), g["d_subset_points"].long()) and torch.equal(d["segments"].cpu(), g["d_segments"])
    assert torch.equal(d["subset_fields"].cpu(), g["d_subset_fields"])


# ------------------------------------------------------------------------------------------------ 4. invariances
def rows_by_field(o):
    n = int(o["count"])
    return {int(g): {k: o[k][i] for k in ("segments", "ijs", "near", "far", "gt", "rgbds", "rgb_mask", "c2ws")}
            for i, g in enumerate(o["field_ids"][:n])}


def assert_rows_equal(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_invariances():
    c = SV.CASES["p2000"]
    s = SV.g16_scene()
    args = (2000, 12, c["R"], 1)
    one = run_ops(s, c["active"], *args)
    assert same(one, run_ops(s, c["active"], *args)), "two calls differ"
    base = rows_by_field(one)
    assert len(base) >= 6
    # fewer fields in active_field_ids: the rows of those that stay are unchanged
    part = rows_by_field(run_ops(s, c["active"][::2], *args))
    assert part and set(part) < set(base)
    for g in part:
        assert_rows_equal(part[g], base[g])
    # sharding: every rank's rows are the single-process rows of its fields, in draw order
    for W in (2, 3):
        for rank in range(W):
            o = run_ops(s, c["active"], *args, world_size=W, rank=rank)
            ids = [int(g) for g in one["field_ids"][:int(one["count"])] if g % W == rank]
            assert [int(g) for g in o["field_ids"][:int(o["count"])]] == ids and len(o["field_ids"]) >= len(ids)
            assert np.array_equal(o["hits"], one["hits"]) and np.array_equal(o["subset_fields"], one["subset_fields"])
            mine = rows_by_field(o)
            for g in ids:
                assert_rows_equal(mine[g], base[g])
    # a frame stack with slot == the single-frame call on that slot (out-of-range slots are clamped)
    frames = [SV.g16_scene(frame_seed=fs)["img"] for fs in (170, 161, 171)]
    stack, poses = dev(np.stack(frames)), dev(np.stack([np.eye(4, dtype=np.float32), s["c2w"], s["c2w"]]))
    for slot, want in ((1, 1), (2, 2), (7, 2), (-3, 0)):
        o = run_ops(s, c["active"], *args, img=stack, c2w=poses, slot=torch.tensor([slot], dtype=torch.int32, device=DEV))
        assert same(o, run_ops(s, c["active"], *args, img=stack[want].contiguous(), c2w=poses[want].contiguous())), slot
    assert same(one, run_ops(s, c["active"], *args, img=stack, c2w=poses, slot=torch.tensor([1], dtype=torch.int32, device=DEV)))
    # num_fields_dev below the largest active id drops those ids
    o = run_ops(s, c["active"], *args, num_fields_dev=torch.tensor([9], dtype=torch.int32, device=DEV))
    m = SV.sample(s["img"], s["c2w"], s["positions"], np.array(c["active"]), s["radius"], s["intrinsics"], *args, 0, num_fields=9,
                  capacity=len(o["field_ids"]))
    SV.compare(o, m)
    assert int(o["count"]) < int(one["count"]) and (o["field_ids"] < 9).all()


# ------------------------------------------------------------------------------------------------ 5. degenerate inputs
def state(r):
    s = {"param " + k: v.clone() for k, v in r._model.all_fields_params.items()}
    for k, st in r._optim_state.items():
        s["exp_avg " + k], s["exp_avg_sq " + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    return s


def assert_all_padding(o):
    assert int(o["count"]) == 0 and (o["field_ids"] == -1).all() and (o["segments"] == -1).all()
    for k in ("ijs", "near", "far", "gt", "rgbds", "rgb_mask", "depth_mask", "term_probs", "term_mask", "c2ws"):
        assert not o[k].any(), k


def test_degenerate_inputs():
    c = SV.CASES["p2000"]
    s = SV.g16_scene()
    blank = dict(s, img=s["img"].copy())
    blank["img"][..., 3] = 0.0
    o = run_ops(blank, c["active"], 2000, 4, 24, 1)                      # no valid depth
    assert_all_padding(o)
    assert int(o["num_used"]) == 0 and (o["pixels"] == -1).all() and not o["hits"].any() and int(o["num_candidates"]) == 0
    o = run_ops(s, c["active"], 2000, 4, 2000, 1)                        # no field is crossed by 2000 of 2000 segments
    assert_all_padding(o)
    assert int(o["num_used"]) == 2000 and o["hits"].any() and int(o["num_candidates"]) == 0 and (o["subset_fields"] == -1).all()
    o = run_ops(s, (-1, -5, 99), 2000, 4, 24, 1)                         # nothing but skipped entries
    assert_all_padding(o)
    # the counted step on a target without rows trains nothing
    r = g16_renderer(s)
    warm = r.sample_target_sv_device(dev(s["img"]), dev(s["c2w"]), torch.tensor(c["active"]), 4, 24, num_points=2000, camera=CAM, iteration=0)
    r.optimization_iteration(warm, seed=3, update=True)                  # moments exist and are not zero
    before = state(r)
    t = r.sample_target_sv_device(dev(blank["img"]), dev(s["c2w"]), torch.tensor(c["active"]), 4, 24, num_points=2000, camera=CAM,
                                  iteration=1)
    assert int(t.count) == 0 and t.ijs.shape[0] == 4
    r.optimization_iteration(t, seed=3, update=True)
    torch.cuda.synchronize()
    after = state(r)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 6. uniformity of the ray draw
def test_ray_draw_is_uniform_over_the_hit_points():
    s = SV.g16_scene()
    m = SV.sample(s["img"], s["c2w"], s["positions"], np.array([3]), s["radius"], s["intrinsics"], 2000, 1, 1, 1, 0)
    # the points depend on the iteration, so they are replayed: one fixed point set, 256 iterations of the ray draw over it
    pixels = dev(m["pixels"], torch.int64)
    c = int(m["hits"][0])
    R = c // 4
    assert c >= 2 * R and R >= 16
    hit_pixels = set(int(p) for p in SV.sample(s["img"], s["c2w"], s["positions"], np.array([3]), s["radius"], s["intrinsics"], 2000, 1, c, 1,
                                               0, draws=dict(pixels=m["pixels"]))["segments"][0])
    assert len(hit_pixels) == c
    img, c2w, pos, act = dev(s["img"]), dev(s["c2w"]), dev(s["positions"]), torch.tensor([3], device=DEV)
    counts = {}
    N = 256
    for it in range(N):
        o = ops.target_sample_sv(img, c2w, act, pos, *s["intrinsics"], s["radius"], pos.shape[0], 1, R, num_points=2000, seed=11,
                                 iteration=it, pixels_in=pixels)
        seg = o["segments"][0].cpu().numpy()
        assert len(set(seg.tolist())) == R
        for p in seg:
            counts[int(p)] = counts.get(int(p), 0) + 1
    assert set(counts) <= hit_pixels, "a pixel that is no hit point was selected"
    q = R / c
    mean, sigma = N * q, (N * q * (1 - q)) ** 0.5                          # binomial: derived, not tuned
    worst = max(abs(counts.get(p, 0) - mean) for p in hit_pixels)
    print(f"uniformity: c = {c}, R = {R}, mean {mean:.1f}, sigma {sigma:.2f}, worst deviation {worst:.1f} = {worst / sigma:.2f} sigma")
    assert worst <= 6 * sigma


# ------------------------------------------------------------------------------------------------ 7. training
def train_scene():
    s = SV.g16_scene()
    frames = np.stack([SV.g16_scene(frame_seed=fs)["img"] for fs in (161, 165, 170)])
    poses = np.stack([s["c2w"]] * 3)
    act = torch.full((16,), -1, dtype=torch.int64)
    act[:12] = torch.tensor(SV.CASES["p2000"]["active"])
    return s, dev(frames), dev(poses), act.to(DEV)


def test_capture_training_sv_equals_the_eager_loop():
    s, frames, poses, act = train_scene()
    T, R, NP, SEED, NIT = 4, 24, 2000, 5, 6
    torch.manual_seed(0)
    ra = g16_renderer(s)
    torch.manual_seed(0)
    rb = g16_renderer(s)
    start = state(ra)
    assert all(torch.equal(v, state(rb)[k]) for k, v in start.items())
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    step = ra.capture_training_sv(frames, poses, act, T, R, num_points=NP, seed=SEED, camera=CAM, slot=slot)
    assert isinstance(step.graph, torch.cuda.CUDAGraph) and isinstance(step.target, Rr.DeviceTarget)
    assert all(torch.equal(v, start[k]) for k, v in state(ra).items()), "capture_training_sv trains nothing by itself"
    assert int(ra._target_iter_dev) == 0 and ra._step == 0
    slots = [0, 2, 1, 1, 0, 2]
    for i in range(NIT):
        slot.fill_(slots[i])
        la = step()
        lb = rb.optimization_iteration(rb.sample_target_sv_device(frames, poses, act, T, R, num_points=NP, seed=SEED, iteration=i,
                                                                  camera=CAM, slot=slot), seed=SEED)
        torch.cuda.synchronize()
        assert 0 < int(step.target.count) <= T
        for k in LOSS_KEYS:
            assert torch.equal(la[k], lb[k]) or (bool(torch.isnan(la[k])) and bool(torch.isnan(lb[k]))), (i, k, la[k], lb[k])
    sa, sb = state(ra), state(rb)
    assert all(torch.equal(sa[k], sb[k]) for k in sa), "6 replays vs 6 eager iterations"
    assert any(not torch.equal(sa[k], start[k]) for k in sa), "nothing was trained"
    assert int(ra._target_iter_dev) == NIT == ra._step
    ra.add_fields(1)                                                     # no reservation: the stacked tensors were replaced
    with pytest.raises(RuntimeError, match="capture again"):
        step()


def test_capture_training_sv_over_reserved_rows_and_refusals():
    s, frames, poses, act = train_scene()
    r = g16_renderer(s)
    r.reserve_fields(20)
    slot = torch.ones(1, dtype=torch.int32, device=DEV)
    step = r.capture_training_sv(frames, poses, act, 4, 24, num_points=2000, seed=5, camera=CAM, slot=slot)
    step()
    quat = torch.zeros(2, 4, device=DEV)
    quat[:, 0] = 1.0
    r.add_fields(2, positions=dev(s["positions"][3:5] + np.float32(0.01)), orientations=quat)      # legal between replays
    act[12:14] = torch.tensor([14, 15], device=DEV)
    out = step()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["combined"])) and int(step.target.num_candidates) >= 4
    assert int(step.target.hits[12]) > 0 and int(step.target.hits[13]) > 0          # the new fields are seen by the old graph
    # refusals, before any launch
    with pytest.raises(ValueError, match="capture_training_sv: rgbd must be a contiguous device tensor"):
        r.capture_training_sv(frames.cpu(), poses, act, 4, 24, camera=CAM)
    with pytest.raises(ValueError, match="capture_training_sv: c2w must be a contiguous device tensor"):
        r.capture_training_sv(frames, poses.transpose(1, 2), act, 4, 24, camera=CAM)
    with pytest.raises(TypeError, match="active_field_ids must be int64"):
        r.capture_training_sv(frames, poses, act.int(), 4, 24, camera=CAM)
    with pytest.raises(ValueError, match="capacity is 0"):
        r.capture_training_sv(frames, poses, act, 0, 24, num_points=2000, camera=CAM)
    rn = g16_renderer(s, geometry_mode="neus")
    with pytest.raises(RuntimeError, match="capture_training_sv: geometry mode 'neus' is outside the counted step"):
        rn.capture_training_sv(frames, poses, act, 4, 24, camera=CAM)
    pos = dev(s["positions"])
    bad = dict(num_points=K.NGM_SV_MAX_POINTS + 1), dict(num_points=0), dict(world_size=2, rank=2), dict(capacity=1)
    for kw in bad:
        with pytest.raises(ValueError, match="target_sample_sv"):
            ops.target_sample_sv(frames[0], poses[0], act, pos, *s["intrinsics"], s["radius"], 14, 4, 24, iteration=0, **kw)
    with pytest.raises(ValueError, match="num_train_fields"):
        ops.target_sample_sv(frames[0], poses[0], act, pos, *s["intrinsics"], s["radius"], 14, K.NGM_TARGET_MAX_DRAW + 1, 24, iteration=0)


def test_example_single_view_loss_falls():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fit_synthetic", os.path.join(root, "examples", "fit_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    losses, psnr, _ = mod.main(iters=51, device=DEV + ":0", quiet=True, loop="single_view")
    print(f"fit_synthetic --single-view, 51 iterations: losses {losses}, PSNR {psnr:.2f} dB")
    assert len(losses) == 3 and all(np.isfinite(losses)) and losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------------ 8. memory safety
def test_guard_bands_odd_sizes():
    """odd H x W, num_points no multiple of any workgroup size, capacity above the rows: nothing is written outside a buffer"""
    s = SV.g16_scene()
    img = dev(s["img"][:199, :317].copy())
    with guard_bands() as bands:
        pos, c2w, act = dev(s["positions"]), dev(s["c2w"]), dev(SV.CASES["p2000"]["active"], torch.int64)
        for kw in (dict(), dict(num_train_fields=12), dict(num_train_fields=12, world_size=3, rank=1)):
            T = kw.pop("num_train_fields", 3)
            o = ops.target_sample_sv(img, c2w, act, pos, *s["intrinsics"], s["radius"], 14, T, 23, num_points=1777, seed=2,
                                     iteration=4, capacity=13, **kw)
            assert 0 < int(o["count"]) < 13 and o["ijs"].shape == (13, 23, 2)
        assert bands.check() > 10
