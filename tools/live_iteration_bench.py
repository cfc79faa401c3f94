"""One captured training graph across frames: what a FRAME of the mapping loop costs before and after.

    python tools/live_iteration_bench.py [--out profiles/r09_live_iteration.json] [--frames 10] [--reps 5]

The reference's iteration (32 fields x 512 rays x (8 + 16) samples, 5 iterations per frame) on a 200-field map and a
640 x 480 keyframe store holding 100 keyframes + the current frame, for the hash and the M1 Fourier network.  Per frame the
current image and pose change and the observed fields are recomputed, so `current_field_ids` has another length every frame.
All loops run in this one process, alternated block by block after warm-up (same box, same clocks):
  a1 recapture   torch transcription of _get_observed_fields (nonzero + multinomial + AABB + the segment kernel) -> a new
                 capture_training on tensors of this frame's shapes -> 5 replays        (what the static capture needs per frame)
  a2 eager       the same transcription -> 5 x (sample_target_mv_device -> optimization_iteration(DeviceTarget))
  b  live        KeyframeStore.set_current -> observed_fields_device(out=...) -> 5 replays of ONE capture_training(
                 current_count=, num_frames=) made before the first frame
  c  replay      per-iteration time of the live replay against a static capture_training replay on inputs of the same shapes
                 (HIP events around blocks of --iters replays); the static loop's own spread between blocks is the yardstick
  d  observe     observed_fields_device alone against the torch transcription alone
  e  syncs       Tensor.item / torch.cuda.synchronize calls per frame of loop b
Frame times are wall-clock (perf_counter around a block of frames that ends in one synchronisation): loops a1 / a2
synchronise with the host inside a frame, so events alone would not see their cost.  The shader clock is read while the live
replay runs."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, H, W, NF, NKF, T, R, SEED, NETWORKS, SyncCounter, _write, block_us, renderer, sclk_while  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd.keyframes import KeyframeStore  # noqa: E402

PER_FRAME, NUM_POINTS, NUM_CURRENT_IMAGES = 5, 500, 4


def scene():
    g = torch.Generator(device=DEV).manual_seed(0)
    pos = torch.rand(NF, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 5.0], device=DEV) - torch.tensor([4.0, 3.0, 7.0], device=DEV)
    quat = torch.zeros(NF, 4, device=DEV)
    quat[:, 0] = 1.0
    store = KeyframeStore(NKF + 28, H, W, device=DEV)
    for k in range(NKF):
        img = torch.rand(H, W, 4, device=DEV, generator=g)
        img[..., 3] = 2.0 + 8.0 * img[..., 3]
        c2w = torch.eye(4, device=DEV)
        c2w[:3, 3] = torch.rand(3, device=DEV, generator=g) * 4.0 - 2.0
        store.add_keyframe(img, k, c2w=c2w)
    current = []
    for k in range(NUM_CURRENT_IMAGES):                       # the frames the camera delivers, cycled
        img = torch.rand(H, W, 4, device=DEV, generator=g)
        img[..., 3] = 2.0 + 8.0 * img[..., 3]
        img[..., 3][torch.rand(H, W, device=DEV, generator=g) < 0.1] = 0.0
        c2w = torch.eye(4, device=DEV)
        c2w[:3, 3] = torch.rand(3, device=DEV, generator=g) * 4.0 - 2.0
        current.append((img.contiguous(), c2w))
    return pos, quat, store, current


def observe_torch(r, rgbd, c2w):
    """_get_observed_fields (rm.py:1642-1670) as the parent commit can run it: torch for the data-dependent steps, the
    segment-sphere test in the existing HIP kernel (as sample_target_sv does)"""
    cam, radius = r._camera, r._field_radius + 0.0
    num = r._global_map_dict["num"]
    pos_c = (r._global_map_dict["positions"][:num] - c2w[:3, 3]) @ c2w[:3, :3]
    fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
    depth = rgbd[..., 3]
    ijs = torch.nonzero(depth)
    dv = depth[ijs[:, 0], ijs[:, 1]]
    points = torch.stack(((ijs[:, 1].float() - cx) * dv / fx, -(ijs[:, 0].float() - cy) * dv / fy, -dv), -1)
    points = points[torch.multinomial(torch.ones(len(points), device=points.device), NUM_POINTS)].contiguous()
    mins, maxs = points.min(0)[0], points.max(0)[0]
    aabb = ((pos_c - radius) <= maxs).all(-1) & ((pos_c + radius) >= mins).all(-1)
    hit = ops.target_sv_intersect(pos_c[aabb].contiguous(), points, radius)
    return torch.arange(num, device=points.device)[aabb][hit.any(-1)]


def frames_ms(fn, frames):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in range(frames):
        fn(f)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0 / frames


def stats(v, digits=3):
    return dict(values=[round(x, digits) for x in v], median=round(statistics.median(v), digits), spread=round(max(v) - min(v), digits))


def measure(network, frames, reps, iters, warmup):
    pos, quat, store, current = scene()
    ra1, ra2, rb, rs = (renderer(network, pos, quat) for _ in range(4))
    nc_rgbd, f2s_full = store.nc_rgbd, store.frame_cid_to_ncid

    def set_frame(f):
        img, c2w = current[f % len(current)]
        store.set_current(img, c2w, frame_id=f)
        return img, c2w

    # a1 / a2: the parent's options, on tensors of this frame's shapes
    def frame_recapture(f):
        img, c2w = set_frame(f)
        cur = observe_torch(ra1, img, c2w).contiguous()
        m = store.count
        step = ra1.capture_training(cur, store.c_c2w[:m].contiguous(), nc_rgbd, f2s_full[:m].contiguous(), T, R, seed=SEED)
        for _ in range(PER_FRAME):
            step()

    def frame_eager(f):
        img, c2w = set_frame(f)
        cur = observe_torch(ra2, img, c2w).contiguous()
        m = store.count
        c, s = store.c_c2w[:m], f2s_full[:m]
        for _ in range(PER_FRAME):
            ra2.optimization_iteration(ra2.sample_target_mv_device(cur, c, nc_rgbd, s, T, R, seed=SEED), seed=SEED)

    # b: one capture for every frame
    ids_buf = torch.full((NF,), -1, dtype=torch.int64, device=DEV)
    cnt_buf = torch.zeros(1, dtype=torch.int32, device=DEV)
    set_frame(0)
    rb.observed_fields_device(nc_rgbd[0], store.c_c2w[0], num_points=NUM_POINTS, seed=SEED, out=(ids_buf, cnt_buf))
    live = rb.capture_training(ids_buf, store.c_c2w, nc_rgbd, f2s_full, T, R, seed=SEED, current_count=cnt_buf,
                               num_frames=store.num_frames)

    def frame_live(f):
        set_frame(f)
        rb.observed_fields_device(nc_rgbd[0], store.c_c2w[0], num_points=NUM_POINTS, seed=SEED, out=(ids_buf, cnt_buf))
        for _ in range(PER_FRAME):
            live()

    # c: a static capture on inputs of the shapes frame 0 has
    n0, m0 = int(cnt_buf), store.count
    static = rs.capture_training(ids_buf[:n0].clone(), store.c_c2w[:m0].clone(), nc_rgbd, f2s_full[:m0].clone(), T, R, seed=SEED)

    loops = dict(recapture=frame_recapture, eager=frame_eager, live=frame_live)
    for fn in loops.values():
        for f in range(max(2, warmup // PER_FRAME // 5)):
            fn(f)
    for _ in range(warmup):
        live()
        static()
    frame_blocks = {n: [] for n in loops}
    for _ in range(reps):
        for n, fn in loops.items():
            frame_blocks[n].append(frames_ms(fn, frames))
    replay_blocks = dict(live=[], static=[])
    for _ in range(reps):
        replay_blocks["static"].append(block_us(static, iters))
        replay_blocks["live"].append(block_us(live, iters))
    img0, c2w0 = current[0]
    obs_blocks = dict(device=[], torch=[])
    for _ in range(reps):
        obs_blocks["torch"].append(block_us(lambda: observe_torch(ra2, img0, c2w0), 50))
        obs_blocks["device"].append(block_us(lambda: rb.observed_fields_device(img0, c2w0, num_points=NUM_POINTS, seed=SEED,
                                                                               out=(ids_buf, cnt_buf)), 50))
    with SyncCounter() as sc:
        for f in range(20):
            frame_live(f)
    torch.cuda.synchronize()
    res = dict(network=network, num_fields=NF, keyframes=NKF, store_capacity=store.capacity, image=[H, W],
               num_train_fields=T, rays_per_field=R, samples_per_ray=[8, 16], iterations_per_frame=PER_FRAME,
               frames_per_block=frames, blocks_per_loop=reps, observed_fields_first_frame=n0,
               a_parent_frame_ms=dict(recapture=stats(frame_blocks["recapture"]), eager=stats(frame_blocks["eager"])),
               b_live_frame_ms=stats(frame_blocks["live"]),
               c_replay_us=dict(iters_per_block=iters, static=stats(replay_blocks["static"], 2), live=stats(replay_blocks["live"], 2)),
               d_observe_us=dict(torch_transcription=stats(obs_blocks["torch"], 2), device=stats(obs_blocks["device"], 2)),
               e_host_syncs_per_frame_live=sc.n / 20)
    best = min(res["a_parent_frame_ms"][k]["median"] for k in ("recapture", "eager"))
    res["a_parent_best_frame_ms"] = best
    res["frame_speedup_live_vs_parent_best"] = round(best / res["b_live_frame_ms"]["median"], 3)
    c = res["c_replay_us"]
    c["live_minus_static_us"] = round(c["live"]["median"] - c["static"]["median"], 2)
    c["live_within_static_spread"] = bool(c["live_minus_static_us"] <= c["static"]["spread"])
    res["sclk_mhz_during_live_replay"] = sclk_while(live)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    out = dict(tool="tools/live_iteration_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing="frames: perf_counter around blocks of --frames frames ending in one synchronisation; replays / observe: "
                      "HIP events around blocks; --reps blocks per loop, the loops alternated in one process after warm-up",
               networks=[])
    for net in NETWORKS:
        out["networks"].append(measure(net, a.frames, a.reps, a.iters, a.warmup))
        print(json.dumps(out["networks"][-1]), flush=True)
    _write(a.out, out)


if __name__ == "__main__":
    main()
