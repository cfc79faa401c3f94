"""End-to-end smoke of the drop-in path on one MI355X: keyframe store -> training-target sampler -> fused
training step (forward, losses, backward, sparse Adam) -> kNN-blended render -> PSNR.

    python examples/fit_synthetic.py [--iters 300] [--device-iteration | --single-view | --live [--grow [--cover]] [--loop-closure]]
                                     [--mesh-metrics [--cull]] [--frame-metrics]

A synthetic RGB-D "scan" of a textured wall with a sphere in front of it is observed from a few keyframes; fields
on a grid in front of the cameras are trained exactly as NeuralGraphMap._optimization_iteration would
(rm.py:1123-1221), with every tensor operation of the hot path running in the HIP kernels.
--device-iteration trains through NeuralGraphRenderer.capture_training instead: targets drawn on the device and consumed at
their fixed capacity, sampler + training step replayed as one captured graph per iteration (no host synchronisation).
--single-view trains in the reference's `update_mode: single_view` through NeuralGraphRenderer.capture_training_sv: the
keyframes form a frame stack, odd iterations draw their targets from the newest frame and even iterations from a random stored
one (a device write into the graph's `slot` between replays), sampler + training step again one captured graph.
--live runs the mapping loop's shape instead of a frozen scene: a new current frame every five iterations, keyframes added
to a KeyframeStore while training, the observed fields recomputed per frame on the device -- and still ONE capture.
--live --grow also GROWS the map while that one graph keeps replaying: the renderer reserves rows for the whole map
(reserve_fields), starts with half of it and appends the rest across the keyframes (add_fields(n, positions=, orientations=):
one launch each, the number of fields read on the device).
--live --grow --cover takes each keyframe's fields not from that prepared list but from extend_map on the keyframe's depth
(the reference's _extend_global_map_dict on the device: grid cells that hold uncovered points and no field yet), anchored to
the keyframe; the same run with the prepared list follows, and both final PSNRs are printed (the two maps differ by construction).
--live --loop-closure anchors every field to a keyframe (anchor_fields) and, once the last keyframe is in, lets the pose graph
move ALL keyframe poses rigidly: KeyframeStore.set_keyframe_poses + repose_fields re-pose the map on the device, the same
graph keeps replaying, and the PSNR of keyframe 0 is reported before and right after the closure.
--mesh-metrics also scores the map as a mesh on the device (NeuralGraphRenderer.evaluate_mesh): the mesh extracted from the
fields around the sphere against the scene's analytic sphere, triangulated here -- the ten numbers of the reference's mesh
evaluation (accuracy, completion, their ratios at 5 cm and 1 cm, F1).  The cameras see the front of the sphere only, so
completion counts its unseen back as missing.  The ten numbers are printed twice: for the mesh as extracted, and for the mesh
aligned to the sphere by point-to-plane ICP on the device first (mesh.align_mesh), the reference's eval_mesh_alignment.
--mesh-metrics --cull also scores the two meshes the way the reference's evaluate_raw_mesh does: both culled first by what the
keyframes see (NeuralGraphRenderer.evaluate_raw_mesh, method "occlusion": frusta and self-occlusion from every keyframe pose),
so the sphere's unseen back no longer counts against completion.
--frame-metrics also scores keyframe 0 the way the reference's _evaluate_frame does (NeuralGraphRenderer.evaluate_frame): the
frame re-rendered in eval mode against the keyframe's image, PSNR, SSIM and depth L1 over the whole frame, in fp64 on the device.
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402

W, H, FOC = 160, 120, 140.0


def look_at(eye, target):
    f = torch.nn.functional.normalize(target - eye, dim=-1)
    up = torch.tensor([0.0, 1.0, 0.0])
    s = torch.nn.functional.normalize(torch.linalg.cross(f, up), dim=-1)
    u = torch.linalg.cross(s, f)
    T = torch.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = s, u, -f, eye          # OpenGL camera: x right, y up, z back
    return T


def synth_keyframe(c2w):
    """Ray-cast an analytic scene: wall z = -3 with a checker texture, unit-radius sphere at (0, 0, -2.2)."""
    ii, jj = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    d = torch.stack([(jj - (W - 1) / 2) / FOC, -(ii - (H - 1) / 2) / FOC, -torch.ones_like(ii)], -1)
    d = torch.nn.functional.normalize(d, dim=-1)
    dw = d @ c2w[:3, :3].T
    o = c2w[:3, 3]
    t_wall = (-3.0 - o[2]) / dw[..., 2]
    c = torch.tensor([0.0, 0.0, -2.2])
    oc = o - c
    b = (dw * oc).sum(-1)
    disc = b * b - (oc @ oc - 0.6 ** 2)
    t_sph = torch.where(disc > 0, -b - torch.sqrt(disc.clamp_min(0)), torch.full_like(b, float("inf")))
    t = torch.minimum(torch.where(t_wall > 0, t_wall, torch.full_like(t_wall, float("inf"))),
                      torch.where(t_sph > 0, t_sph, torch.full_like(t_sph, float("inf"))))
    p = o + dw * t[..., None]
    wall = ((torch.floor(p[..., 0] * 2) + torch.floor(p[..., 1] * 2)) % 2)[..., None] * torch.tensor([0.6, 0.5, 0.2]) + 0.2
    sph = torch.tensor([0.8, 0.2, 0.2]).expand_as(wall) * (0.5 + 0.5 * torch.nn.functional.normalize(p - c, dim=-1)[..., 1:2])
    rgb = torch.where((t_sph < t_wall)[..., None], sph, wall)
    depth = t * d[..., 2].abs()                                     # depth along the optical axis
    return torch.cat([rgb, depth[..., None]], -1)


def sphere_mesh(centre, radius, n_lat=48, n_lon=96):
    """the scene's sphere as a triangle mesh (n_lat bands x n_lon sectors, vertices on the sphere): (verts (V, 3), faces (T, 3))"""
    th = torch.linspace(0, math.pi, n_lat + 1)
    ph = torch.arange(n_lon) * (2 * math.pi / n_lon)
    v = torch.stack([torch.sin(th)[:, None] * torch.cos(ph)[None], torch.sin(th)[:, None] * torch.sin(ph)[None],
                     torch.cos(th)[:, None].expand(-1, n_lon)], -1).reshape(-1, 3)
    i, j = torch.arange(n_lat)[:, None] * n_lon, torch.arange(n_lon)[None]
    a, b = i + j, i + (j + 1) % n_lon
    f = torch.cat([torch.stack([a, a + n_lon, b], -1).reshape(-1, 3), torch.stack([b, a + n_lon, b + n_lon], -1).reshape(-1, 3)])
    return radius * v + torch.tensor(centre), f.to(torch.int64)


def main(iters=300, device="cuda:0", quiet=False, loop="torch", jitter_seed=0, grow=False, loop_closure=False, mesh_metrics=False, cull=False, frame_metrics=False,
         cover=False):
    """loop: "torch" -- sample_target_mv (torch draws) -> optimization_iteration, the reference's loop;
    "device" -- capture_training: one graph replay per iteration;
    "materialize" -- the same device-drawn targets and jitter stream as "device" (sampler seed 0, iteration i; jitter
    seed `jitter_seed`), but sliced to their count on the host every iteration (DeviceTarget.materialize: one
    synchronisation, a data-dependent batch shape);
    "live" -- capture_training once over fixed-capacity buffers (KeyframeStore, observed_fields_device(out=...)): the
    current frame changes every 5 iterations, each camera's first visit adds a keyframe, the graph is never re-captured.
    grow (with "live"): rows are reserved for the whole map, half of it is there at the capture, every keyframe appends a
    share of the rest in place.
    cover (with "live" and grow): the fields a keyframe brings are not taken from the prepared list but placed by
    extend_map on that keyframe's depth (the reference's _extend_global_map_dict), anchored to it; the reservation is larger,
    since the number of fields is then the scene's and the grid's business.
    loop_closure (with "live"): the fields are anchored to the keyframes; after the last keyframe all keyframe poses are
    perturbed rigidly and the map is re-posed on the device between two replays of the one graph.
    "single_view" -- capture_training_sv over the keyframes as a frame stack: odd iterations read the newest frame, even
    iterations a random stored one (torch.randint on the device into `slot`), rm.py:1130-1149."""
    if loop not in ("torch", "device", "materialize", "live", "single_view"):
        raise ValueError(loop)
    if (grow or loop_closure) and loop != "live":
        raise ValueError("grow and loop_closure go with the live loop")
    if cover and not (grow and loop == "live"):
        raise ValueError("cover goes with the live loop and grow")
    if cover and (loop_closure or mesh_metrics):
        raise ValueError("cover places its own fields: the loop-closure and mesh-metrics legs index the prepared map")
    torch.manual_seed(0)
    dev = torch.device(device)
    cam = Rr.Camera(W, H, FOC, FOC, (W - 1) / 2, (H - 1) / 2, pixel_center=0.0)
    radius = 0.5
    # fields on a grid covering the visible surfaces
    gx, gy, gz = torch.meshgrid(torch.arange(-2.0, 2.01, 0.5), torch.arange(-1.5, 1.51, 0.5), torch.tensor([-2.9]), indexing="ij")
    sx, sy, sz = torch.meshgrid(torch.arange(-0.5, 0.51, 0.5), torch.arange(-0.5, 0.51, 0.5), torch.tensor([-2.4, -1.9]),
                                indexing="ij")
    pos = torch.cat([torch.stack([gx, gy, gz], -1).reshape(-1, 3), torch.stack([sx, sy, sz], -1).reshape(-1, 3)])
    NF = pos.shape[0]
    quat = torch.zeros(NF, 4)
    quat[:, 0] = 1
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=64, mu=0.0, sigma=4.0, raw_coords=True), num_layers=2, dim_out=4),
        num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=radius, scale_mode="unit_cube").to(dev)
    cfg = dict(geometry_mode="nrgbd", geometry_factor=20.0, color_factor=1.0, truncation_distance=0.1, field_radius=radius,
               termination_weight=0.0, photometric_weight=1.0, photometric_loss="l1", depth_weight=1.0, depth_loss="huber",
               freespace_weight=40.0, tsdf_weight=50.0,
               learning_rate=2e-3, adam_eps=1e-15, adam_weight_decay=1e-5, num_samples_coarse=8, num_samples_depth_guided=16,
               near_distance=0.0, far_distance=5.0, eval_near_distance=0.5, eval_far_distance=4.5, eval_num_samples=160)
    r = Rr.NeuralGraphRenderer(model, cam, cfg, device=dev)
    n0 = NF // 2 if grow else NF
    r.add_fields(n0)
    r.set_field_poses(pos[:n0].to(dev), quat[:n0].to(dev))
    if grow:
        CAP = NF + 512 if cover else NF                             # cover: as many fields as the keyframes' depth asks for
        r.reserve_fields(CAP)                                       # once; from here on nothing of the map is reallocated
    eyes = torch.tensor([[0.0, 0.0, 0.0], [0.7, 0.2, 0.1], [-0.7, -0.1, 0.2], [0.2, 0.5, 0.3]])
    c2ws = torch.stack([look_at(e, torch.tensor([0.0, 0.0, -2.6])) for e in eyes])
    store = torch.stack([synth_keyframe(T) for T in c2ws]).contiguous().to(dev)
    c2ws = c2ws.to(dev)
    cid = torch.arange(len(eyes), device=dev)
    cur = torch.arange(NF, device=dev)

    def evaluate():
        """keyframe 0 re-rendered from its pose in force: (PSNR, median |depth error|, share of pixels compared)"""
        r.eval()                                                    # as rm.py:1978 before an evaluation render
        rgbd, _ = r.render_image(c2ws[0], camera=cam)
        r.train()
        ref = store[0]
        valid = torch.isfinite(ref[..., 3]) & (rgbd[..., 3] > 0.1)  # pixels whose ray meets a trained field
        mse = ((rgbd[..., :3].clamp(0, 1) - ref[..., :3]) ** 2)[valid].mean()
        return (float(10 * torch.log10(1.0 / mse)), float((rgbd[..., 3] - ref[..., 3]).abs()[valid].median()),
                float(valid.float().mean()))

    losses, closure = [], None
    step = r.capture_training(cur, c2ws, store, cid, 32, 256, seed=jitter_seed, camera=cam) if loop == "device" else None
    if loop == "single_view":
        slot = torch.zeros(1, dtype=torch.int32, device=dev)
        slot_gen = torch.Generator(device=dev).manual_seed(0)
        step = r.capture_training_sv(store, c2ws, cur, 32, 256, num_points=min(50000, H * W), seed=jitter_seed, camera=cam, slot=slot)
    if loop == "live":
        from neural_graph_mapping_amd.keyframes import KeyframeStore
        ks = KeyframeStore(len(eyes) + 1, H, W, device=dev)
        ids_buf = torch.full((CAP if grow else NF,), -1, dtype=torch.int64, device=dev)
        cnt_buf = torch.zeros(1, dtype=torch.int32, device=dev)
        r.track_training_iterations = True
        cover_gen = torch.Generator(device=dev).manual_seed(0)      # extend_map draws the grid's shift from it

        def next_frame(f):
            nonlocal c2ws, closure
            k = f % len(eyes)
            if loop_closure and f == len(eyes):                     # every keyframe is in: the pose graph closes a loop
                before = evaluate()[0]
                r.anchor_fields(ks, [i % len(eyes) for i in range(NF)])        # keyframe f has frame id f
                a = 0.05
                D = torch.tensor([[math.cos(a), 0.0, math.sin(a), 0.08], [0.0, 1.0, 0.0, -0.05],
                                  [-math.sin(a), 0.0, math.cos(a), 0.04], [0.0, 0.0, 0.0, 1.0]], device=dev)
                c2ws = D @ c2ws                                     # all poses move rigidly, keyframes and later frames alike
                ks.set_keyframe_poses(c2ws[ks.frame_ids])
                r.repose_fields(ks)                                 # one launch; the graph reads the poses in place
                closure = (before, evaluate()[0])
            ks.set_current(store[k], c2ws[k], frame_id=f)
            if f < len(eyes):
                ks.add_keyframe(store[k], f)                        # a camera's first visit becomes a keyframe
                if cover:                                           # ... and is covered with new fields where the map has none
                    r.extend_map(ks.nc_rgbd[ks.slot_of(f)], f, c2ws[k], store=ks, generator=cover_gen, camera=cam)
                elif grow:                                          # ... or brings its share of the fields still missing
                    new = torch.tensor_split(torch.arange(n0, NF), len(eyes))[k]
                    r.add_fields(len(new), positions=pos[new].to(dev), orientations=quat[new].to(dev))
            r.observed_fields_device(ks.nc_rgbd[0], ks.c_c2w[0], seed=0, frame=f, out=(ids_buf, cnt_buf), camera=cam)
    for it in range(iters):
        if loop == "live":
            if it % 5 == 0:                                         # num_iterations_per_frame: 5
                next_frame(it // 5)
            if step is None:
                step = r.capture_training(ids_buf, ks.c_c2w, ks.nc_rgbd, ks.frame_cid_to_ncid, 32, 256, seed=jitter_seed,
                                          camera=cam, current_count=cnt_buf, num_frames=ks.num_frames)
                graph = step.graph
            out = step()
            assert step.graph is graph                              # one capture serves every frame and keyframe
        elif loop == "device":
            out = step()
        elif loop == "single_view":
            if it % 2 == 1:
                slot.fill_(len(eyes) - 1)                           # the newest frame
            else:
                slot.copy_(torch.randint(0, len(eyes), (1,), device=dev, generator=slot_gen, dtype=torch.int32))
            out = step()
        elif loop == "materialize":
            tgt = r.sample_target_mv_device(cur, c2ws, store, cid, 32, 256, camera=cam, seed=0, iteration=it).materialize()
            out = r.optimization_iteration(tgt, seed=jitter_seed)
        else:
            tgt = r.sample_target_mv(cur, c2ws, store, cid, num_train_fields=32, num_rays_per_field=256, camera=cam)
            out = r.optimization_iteration(tgt, seed=it)
        if it % 25 == 0 or it == iters - 1:
            losses.append(float(out["combined"]))
            if not quiet:
                print(f"iter {it:4d}  loss {losses[-1]:.4f}  (photo {float(out['photometric_l1']):.4f} depth {float(out['depth_huber']):.4f} "
                      f"fs {float(out['freespace']):.4f} tsdf {float(out['tsdf']):.4f})")
    psnr, derr, share = evaluate()
    if not quiet:
        print(f"keyframe 0 re-rendered: PSNR {psnr:.2f} dB, median |depth error| {derr:.3f} m over "
              f"{100 * share:.0f} % of the pixels ({r._global_map_dict['num']} fields)")
        if loop == "live":
            print(f"{ks.num_keyframes} keyframes, {int(cnt_buf)} fields observed by the last frame, "
                  f"{int(r.get_field_ids(50).numel())} fields trained in at least 50 iterations")
            if closure is not None:
                print(f"loop closure after the last keyframe: PSNR {closure[0]:.2f} dB before, {closure[1]:.2f} dB right after "
                      "the re-pose, under the same graph")
            if grow:
                print(f"the map grew from {n0} to {r._global_map_dict['num']} fields under that one graph")
    if frame_metrics:
        fm = r.evaluate_frame(c2ws[0], store[0], camera=cam, metrics=["psnr", "ssim", "depthl1"], crop=10)
        print(f"keyframe 0 as the reference's _evaluate_frame scores it (whole frame, crop 10): PSNR {fm['psnr']:.2f} dB, "
              f"SSIM {fm['ssim']:.4f}, depth L1 {fm['depthl1']:.4f} m")
    if mesh_metrics:
        gv, gf = sphere_mesh([0.0, 0.0, -2.2], 0.6)
        around = torch.arange(NF - 18, NF, device=dev)              # the 3 x 3 x 2 fields around the sphere
        m = r.evaluate_mesh((gv.to(dev), gf.to(dev)), num_points=200000, seed=0, resolution=0.02, field_ids=around)
        if m is None:
            print("mesh metrics: the fields around the sphere hold no surface yet")
        else:
            print("mesh of the fields around the sphere against the analytic sphere (metres; ratios at 5 cm / 1 cm):")
            print("  " + "  ".join(f"{k} {v:.4f}" for k, v in m.items()))
            # once more as the reference's eval_mesh_alignment scores it: the extracted mesh aligned to the ground truth by
            # point-to-plane ICP on the device first (mesh.align_mesh; evaluate_raw_mesh(align="icp") does it between its two cullings)
            from neural_graph_mapping_amd import mesh as ngm_mesh
            est = r.extract_mesh(resolution=0.02, field_ids=around)
            aligned, icp = ngm_mesh.align_mesh((est[0], est[1]), (gv.to(dev), gf.to(dev)))
            ma = ngm_mesh.evaluate_mesh(aligned, (gv.to(dev), gf.to(dev)), num_points=200000, seed=0)
            print(f"the same after ICP alignment ({int(icp.iterations)} iterations, converged {bool(icp.converged)}, fitness {float(icp.fitness):.4f}, "
                  f"inlier rmse {float(icp.inlier_rmse):.4f} m):")
            print("  " + "  ".join(f"{k} {v:.4f}" for k, v in ma.items()))
        if cull and m is not None:
            m = r.evaluate_raw_mesh((gv.to(dev), gf.to(dev)), c2ws, cam, "occlusion", "occlusion", num_points=200000, seed=0, resolution=0.02,
                                    field_ids=around)
            print("the same two meshes, both culled to what the keyframes see (frusta and self-occlusion) before they are scored:")
            print("  " + "  ".join(f"{k} {v:.4f}" for k, v in m.items()))
    return losses, psnr, derr


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--device-iteration", action="store_true",
                    help="train through capture_training: device-drawn targets, one captured graph per iteration")
    ap.add_argument("--single-view", action="store_true",
                    help="train through capture_training_sv: single-view targets from a frame stack, one captured graph per iteration")
    ap.add_argument("--live", action="store_true",
                    help="one captured graph across changing frames and keyframes (KeyframeStore + observed_fields_device)")
    ap.add_argument("--grow", action="store_true",
                    help="with --live: reserve rows for the whole map, start with half of it, append the rest across keyframes")
    ap.add_argument("--cover", action="store_true",
                    help="with --live --grow: each keyframe's fields come from extend_map on its depth, not from the prepared list")
    ap.add_argument("--loop-closure", action="store_true",
                    help="with --live: anchor the fields to keyframes, move all keyframe poses rigidly after the last keyframe, re-pose")
    ap.add_argument("--mesh-metrics", action="store_true",
                    help="score the mesh of the fields around the sphere against the analytic sphere on the device (ten numbers)")
    ap.add_argument("--cull", action="store_true",
                    help="with --mesh-metrics: also score the two meshes after culling both to what the keyframes see (evaluate_raw_mesh)")
    ap.add_argument("--frame-metrics", action="store_true",
                    help="score keyframe 0 with PSNR, SSIM and depth L1 on the device (evaluate_frame)")
    a = ap.parse_args()
    loop = "live" if a.live else "device" if a.device_iteration else "single_view" if a.single_view else "torch"
    res = main(a.iters, loop=loop, grow=a.grow, loop_closure=a.loop_closure, mesh_metrics=a.mesh_metrics, cull=a.cull,
               frame_metrics=a.frame_metrics, cover=a.cover)
    if a.cover:                                                    # the two maps differ by construction: no bar, both numbers
        prepared = main(a.iters, loop=loop, grow=True, quiet=True)
        print(f"final PSNR of keyframe 0: {res[1]:.2f} dB with the fields extend_map placed, {prepared[1]:.2f} dB with the prepared "
              "list (--grow)")
