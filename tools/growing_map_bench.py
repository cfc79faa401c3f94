"""A map that grows under the live training graph: what the reservation costs per replay and what a keyframe that adds
fields costs with and without it.

    python tools/growing_map_bench.py [--out profiles/r10_growing_map.json] [--reps 5] [--iters 300]
                                      [--parent-json FILE] [--kernel-resources FILE]

The shapes of tools/live_iteration_bench.py (r09): 200 fields, 100 keyframes of 640 x 480 + the current frame, 32 fields x
512 rays x (8 + 16) samples, the hash and the M1 Fourier network.  One process, the loops alternated block by block after
warm-up (same box, same clocks):
  a  replay     per-iteration time of the live replay of a map with 256 reserved rows (capture_training after
                reserve_fields(256): ngm_target_sample_mv_grow, the field count read on the device) against the live replay
                of the unreserved map (ngm_target_sample_mv_live, the parent commit's path); HIP events around blocks of
                --iters replays.  The yardstick is the unreserved loop's own spread between blocks.  A third loop reserves
                exactly the 200 rows the map has (the grow code path without the larger allocation).
  b  keyframe   a keyframe that adds 8 fields, wall-clock per keyframe ending in one synchronisation:
                  reserved    add_fields(8, positions=, orientations=) (one launch) + 5 replays of the SAME graph
                  unreserved  add_fields(8) + set_field_poses + a fresh capture_training + 5 replays   (the parent's frame)
                the reserved map is put back to 200 fields between blocks (host bookkeeping only; the rows stay allocated)
On a tree without reserve_fields (the parent commit) only the unreserved loops run, so that the same file measures both
commits' binaries; --parent-json merges such a run's result.  --kernel-resources merges a JSON of the compiler's per-kernel
register / scratch report for the kernels this changed (made where the library is built)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, NF, T, R, SEED, NETWORKS, _write, block_us, renderer, sclk_while  # noqa: E402
from live_iteration_bench import NUM_POINTS, PER_FRAME, scene, stats  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402

RESERVE, GROW = 256, 8
HAVE = hasattr(Rr.NeuralGraphRenderer, "reserve_fields")


def live_capture(r, store, ids_buf, cnt_buf):
    r.observed_fields_device(store.nc_rgbd[0], store.c_c2w[0], num_points=NUM_POINTS, seed=SEED, out=(ids_buf, cnt_buf))
    return r.capture_training(ids_buf, store.c_c2w, store.nc_rgbd, store.frame_cid_to_ncid, T, R, seed=SEED, current_count=cnt_buf,
                              num_frames=store.num_frames)


def keyframe_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0 / n


def measure(network, reps, iters, warmup, keyframes):
    pos, quat, store, current = scene()
    img, c2w = current[0]
    store.set_current(img, c2w, frame_id=0)
    g = torch.Generator(device=DEV).manual_seed(1)
    new_pos = torch.rand(GROW, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 5.0], device=DEV) - torch.tensor([4.0, 3.0, 7.0], device=DEV)
    new_quat = quat[:GROW].clone()
    bufs = lambda n: (torch.full((n,), -1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))

    ru = renderer(network, pos, quat)                                  # unreserved: the parent's live path
    ids_u, cnt_u = bufs(NF)
    live_u = live_capture(ru, store, ids_u, cnt_u)
    loops = dict(unreserved=live_u)
    if HAVE:
        rr = renderer(network, pos, quat)
        rr.reserve_fields(RESERVE)
        ids_r, cnt_r = bufs(RESERVE)
        loops["reserved"] = live_capture(rr, store, ids_r, cnt_r)
        rx = renderer(network, pos, quat)                              # the grow path at the unreserved map's own size: tells the
        rx.reserve_fields(NF)                                          # cost of the code path from that of the larger allocation
        ids_x, cnt_x = bufs(NF)
        loops["reserved_exact"] = live_capture(rx, store, ids_x, cnt_x)
    for _ in range(warmup):
        for fn in loops.values():
            fn()
    replay = {n: [] for n in loops}
    for i in range(reps):                                              # order reversed every other block
        for n, fn in (list(loops.items()) if i % 2 == 0 else list(loops.items())[::-1]):
            replay[n].append(block_us(fn, iters))

    # b: the keyframe that adds GROW fields
    rk = None                                                          # a fresh 200-field map per keyframe (built outside the timing)
    ids_k, cnt_k = bufs(NF + GROW)

    def keyframe_unreserved():
        rk.add_fields(GROW)
        rk.set_field_poses(torch.cat((pos, new_pos)), torch.cat((quat, new_quat)))
        step = live_capture(rk, store, ids_k, cnt_k)
        for _ in range(PER_FRAME):
            step()

    def timed_unreserved(n):
        """per keyframe: the growth, the capture and the replays; building the 200-field map it starts from is outside"""
        nonlocal rk
        total = 0.0
        for _ in range(n):
            rk = renderer(network, pos, quat)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keyframe_unreserved()
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        return total * 1000.0 / n

    def keyframe_reserved():
        rr.add_fields(GROW, positions=new_pos, orientations=new_quat)
        for _ in range(PER_FRAME):
            loops["reserved"]()
        # back to NF fields for the next block: host mirrors and the device count only, nothing is reallocated
        rr._model._set_num(NF)
        rr._set_num(NF)
        rr._reserved["num_fields_dev"].fill_(NF)

    kf = dict(unreserved=[])
    timed_unreserved(1)
    if HAVE:
        kf["reserved"] = []
        keyframe_reserved()
    for _ in range(reps):
        kf["unreserved"].append(timed_unreserved(keyframes))
        if HAVE:
            kf["reserved"].append(keyframe_ms(keyframe_reserved, keyframes))
    torch.cuda.synchronize()
    res = dict(network=network, num_fields=NF, reserved_rows=RESERVE if HAVE else None, fields_added_per_keyframe=GROW,
               num_train_fields=T, rays_per_field=R, iterations_per_frame=PER_FRAME, blocks_per_loop=reps,
               a_replay_us=dict(iters_per_block=iters, **{n: stats(v, 2) for n, v in replay.items()}),
               b_keyframe_ms=dict(keyframes_per_block=keyframes, **{n: stats(v) for n, v in kf.items()}))
    if HAVE:
        a = res["a_replay_us"]
        a["reserved_minus_unreserved_us"] = round(a["reserved"]["median"] - a["unreserved"]["median"], 2)
        a["reserved_within_unreserved_spread"] = bool(a["reserved_minus_unreserved_us"] <= a["unreserved"]["spread"])
        a["reserved_exact_minus_unreserved_us"] = round(a["reserved_exact"]["median"] - a["unreserved"]["median"], 2)
        b = res["b_keyframe_ms"]
        b["speedup_reserved_vs_unreserved"] = round(b["unreserved"]["median"] / b["reserved"]["median"], 2)
    res["sclk_mhz_during_replay"] = sclk_while(loops["reserved" if HAVE else "unreserved"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--keyframes", type=int, default=3)
    ap.add_argument("--parent-json", default=None, help="the result of this tool run on the parent commit's tree")
    ap.add_argument("--kernel-resources", default=None, help="JSON of the compiler's register / scratch report")
    a = ap.parse_args()
    out = dict(tool="tools/growing_map_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               has_reserve_fields=HAVE,
               timing="replays: HIP events around blocks of --iters replays; keyframes: perf_counter around one keyframe ending in one "
                      "synchronisation, averaged over --keyframes; --reps blocks per loop, the loops alternated in one process "
                      "after warm-up",
               networks=[])
    for net in NETWORKS:
        out["networks"].append(measure(net, a.reps, a.iters, a.warmup, a.keyframes))
        print(json.dumps(out["networks"][-1]), flush=True)
    for key, path in (("parent_commit_same_box", a.parent_json), ("c_kernel_resources", a.kernel_resources)):
        if path and os.path.exists(path):
            out[key] = json.load(open(path))
    _write(a.out, out)


if __name__ == "__main__":
    main()
