"""A loop-closure frame under the live training graph: the keyframe poses move, the map follows, five replays.

    python tools/repose_bench.py [--out profiles/r12_repose.json] [--reps 5] [--frames 4] [--bench-json FILE]

Two ways to make the map follow, alternated in one process after warm-up (same box, same clocks), --reps blocks each:
  repose  KeyframeStore.set_keyframe_poses + NeuralGraphRenderer.repose_fields (ngm_fields_repose: one launch + the advance
          of the previous-pose table) + 5 replays of the captured graph
  torch   set_keyframe_poses + the reference's two steps written in torch on the device (rm.py:844-885: index_select, batched
          4x4 inverse, einsums, matrix_to_quaternion, quaternion products, every field whether its keyframe moved or not) +
          set_field_poses (a copy into the reserved rows) + 5 replays of the same kind of graph
Two sizes: 200 fields / 100 keyframes and 20 000 fields / 1000 keyframes (M1 Fourier network, 32 fields x 512 rays per
iteration, 640 x 480 keyframes); each with ALL keyframes moved and with ONE moved.  Wall-clock per frame ends in one
synchronisation.  Also recorded: the re-pose alone between device events (both paths), and the device kernels each path's
pose update launches (torch.profiler; None where the profiler gives no device events).  --bench-json merges a file holding
bench.py's result lines of the parent commit and of this tree from the same box.  No speed-up is promised: these are the
numbers nobody had measured."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, H, W, FX, CX, CY, T, R, SEED, NETWORKS, _write  # noqa: E402
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from neural_graph_mapping_amd.keyframes import KeyframeStore  # noqa: E402

PER_FRAME, NUM_POINTS, NETWORK = 5, 500, "m1_fourier"
SIZES = ((200, 100), (20000, 1000))


def stats(v, digits=3):
    return dict(values=[round(x, digits) for x in v], median=round(statistics.median(v), digits), spread=round(max(v) - min(v), digits))


def renderer(pos, quat):
    enc, ekw, layers = NETWORKS[NETWORK]
    torch.manual_seed(0)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type=enc, encoding_kwargs=ekw, num_layers=layers, dim_out=4, neus_initial_sd=1.0), num_knn=2,
        distance_factor=10.0, outside_value=1.0, field_radius=1.0, scale_mode="unit_cube").to(DEV)
    r = Rr.NeuralGraphRenderer(model, Rr.Camera(W, H, FX, FX, CX, CY, pixel_center=0.0), Rr.shipped_config(), device=DEV)
    r.add_fields(pos.shape[0])
    r.set_field_poses(pos.clone(), quat.clone())
    r.reserve_fields(pos.shape[0])                            # set_field_poses then copies in place: the graph stays valid
    return r


def scene(nf, nkf):
    g = torch.Generator(device=DEV).manual_seed(0)
    pos = torch.rand(nf, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 5.0], device=DEV) - torch.tensor([4.0, 3.0, 7.0], device=DEV)
    quat = torch.zeros(nf, 4, device=DEV)
    quat[:, 0] = 1.0
    store = KeyframeStore(nkf + 1, H, W, device=DEV)
    for k in range(nkf):
        img = torch.rand(H, W, 4, device=DEV, generator=g)
        img[..., 3] = 2.0 + 8.0 * img[..., 3]
        c2w = torch.eye(4, device=DEV)
        c2w[:3, 3] = torch.rand(3, device=DEV, generator=g) * 4.0 - 2.0
        store.add_keyframe(img, k, c2w=c2w)
    img = torch.rand(H, W, 4, device=DEV, generator=g)
    img[..., 3] = 2.0 + 8.0 * img[..., 3]
    store.set_current(img, torch.eye(4, device=DEV), frame_id=nkf)
    return pos, quat, store


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def matrix_to_quaternion(m):
    """pytorch3d's, in torch: the best-conditioned of four candidates"""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.reshape(-1, 9).unbind(-1)
    q_abs = torch.stack((1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22), -1).clamp_min(0).sqrt()
    cand = torch.stack((torch.stack((q_abs[:, 0] ** 2, m21 - m12, m02 - m20, m10 - m01), -1),
                        torch.stack((m21 - m12, q_abs[:, 1] ** 2, m10 + m01, m02 + m20), -1),
                        torch.stack((m02 - m20, m10 + m01, q_abs[:, 2] ** 2, m12 + m21), -1),
                        torch.stack((m10 - m01, m20 + m02, m21 + m12, q_abs[:, 3] ** 2), -1)), -2)
    cand = cand / (2.0 * q_abs[..., None].clamp_min(0.1))
    best = torch.nn.functional.one_hot(q_abs.argmax(-1), 4) > 0.5
    return cand[best].reshape(-1, 4)


def torch_repose(pos, quat, kf_rows, prev, new):
    """rm.py:864-885 then :844-862, all fields"""
    w2kf = prev.index_select(0, kf_rows).inverse()
    rel_p = torch.einsum("fdk,fk->fd", w2kf[:, :3, :3], pos) + w2kf[:, :3, 3]
    rel_q = quat_mul(matrix_to_quaternion(w2kf[:, :3, :3]), quat)
    kf2w = new.index_select(0, kf_rows)
    return (torch.einsum("fdk,fk->fd", kf2w[:, :3, :3], rel_p) + kf2w[:, :3, 3],
            quat_mul(matrix_to_quaternion(kf2w[:, :3, :3]), rel_q))


def frame_ms(fn, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        fn()
        torch.cuda.synchronize()                              # a frame ends in one synchronisation
    return (time.perf_counter() - t0) * 1000.0 / frames


def event_us(fn, before=None, n=20):
    out = []
    for _ in range(n):
        if before is not None:
            before()                                          # outside the events
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0)
    return round(statistics.median(out), 2)


def device_kernels(fn):
    """device kernels one call launches, by name"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = {}
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                names[e.name] = names.get(e.name, 0) + 1
        return dict(launches=sum(names.values()), kernels=names) if names else None
    except Exception as err:                                  # a measurement aid: its failure must not cost the timings
        return dict(error=str(err)[:200])


def measure(nf, nkf, reps, frames):
    pos, quat, store = scene(nf, nkf)
    ra, rb = renderer(pos, quat), renderer(pos, quat)
    g = torch.Generator().manual_seed(1)
    kf_of_field = torch.randint(0, nkf, (nf,), generator=g)
    ra.anchor_fields(store, kf_of_field)
    kf_rows = ra._anchor["slot"][:nf].long()                  # the torch path's index into the slot tables
    ids, cnt = torch.full((nf,), -1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    steps = []
    for r in (ra, rb):
        r.observed_fields_device(store.nc_rgbd[0], store.c_c2w[0], num_points=NUM_POINTS, seed=SEED, out=(ids, cnt))
        steps.append(r.capture_training(ids, store.c_c2w, store.nc_rgbd, store.frame_cid_to_ncid, T, R, seed=SEED, current_count=cnt,
                                        num_frames=store.num_frames))
    base = store.slot_c2w[[store.slot_of(f) for f in store.frame_ids]].clone()    # in the order set_keyframe_poses takes
    a = 0.02
    D = torch.tensor([[1.0, 0.0, 0.0, 0.03], [0.0, math.cos(a), -math.sin(a), -0.02], [0.0, math.sin(a), math.cos(a), 0.01],
                      [0.0, 0.0, 0.0, 1.0]], device=DEV)
    moved_all = D @ base
    moved_one = base.clone()
    moved_one[nkf // 2] = moved_all[nkf // 2]
    prev_b = store.slot_c2w.clone()                           # the torch path keeps its own previous-pose table
    flip = [0]

    def poses(which):
        flip[0] ^= 1                                          # the poses alternate, so every frame moves them
        return (moved_all if which == "all" else moved_one) if flip[0] else base

    def pose_update_repose(which):
        store.set_keyframe_poses(poses(which))
        ra.repose_fields(store)

    def pose_update_torch(which):
        store.set_keyframe_poses(poses(which))
        md = rb._global_map_dict
        p, q = torch_repose(md["positions"], md["orientations"], kf_rows, prev_b, store.slot_c2w)
        rb.set_field_poses(p, q)
        prev_b.copy_(store.slot_c2w)

    def frame(update, step, which):
        update(which)
        for _ in range(PER_FRAME):
            step()

    res = dict(num_fields=nf, num_keyframes=nkf, network=NETWORK, num_train_fields=T, rays_per_field=R, replays_per_frame=PER_FRAME,
               frames_per_block=frames, blocks_per_path=reps)
    for which in ("all", "one"):
        paths = dict(repose=lambda: frame(pose_update_repose, steps[0], which), torch=lambda: frame(pose_update_torch, steps[1], which))
        for fn in paths.values():                             # warm-up
            fn()
            fn()
        ms = {n: [] for n in paths}
        for i in range(reps):
            for n, fn in (list(paths.items()) if i % 2 == 0 else list(paths.items())[::-1]):
                ms[n].append(frame_ms(fn, frames))
        res[f"moved_{which}"] = dict(
            frame_ms={n: stats(v) for n, v in ms.items()},
            pose_update_device_us=dict(repose=event_us(lambda: pose_update_repose(which)), torch=event_us(lambda: pose_update_torch(which))),
            repose_call_device_us=event_us(lambda: ra.repose_fields(store), before=lambda: store.set_keyframe_poses(poses(which))))
    res["device_kernels_per_pose_update"] = dict(repose=device_kernels(lambda: pose_update_repose("all")),
                                                 torch=device_kernels(lambda: pose_update_torch("all")))
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--bench-json", default=None, help="bench.py's result lines of the parent commit and this tree, same box")
    a = ap.parse_args()
    out = dict(tool="tools/repose_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing="frames: perf_counter around one loop-closure frame (pose update + 5 replays) ending in one synchronisation, "
                      "averaged over --frames; --reps blocks per path, the paths alternated in one process after warm-up; "
                      "pose_update_device_us: median of 20, HIP events around the pose update (set_keyframe_poses included); "
                      "repose_call_device_us: around repose_fields alone (ngm_fields_repose + the advance)",
               sizes=[])
    for nf, nkf in SIZES:
        out["sizes"].append(measure(nf, nkf, a.reps, a.frames))
        print(json.dumps(out["sizes"][-1]), flush=True)
        _write(a.out, out)                                    # the larger size may not fit every box: keep what is measured
    if a.bench_json and os.path.exists(a.bench_json):
        out["bench_py_parent_and_this_tree_same_box"] = json.load(open(a.bench_json))
        _write(a.out, out)


if __name__ == "__main__":
    main()
