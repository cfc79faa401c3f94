"""Covering a 640 x 480 keyframe's depth with new fields: ngm_cover_depth, extend_map, and the reference's steps in torch.

    python tools/cover_depth_bench.py [--out profiles/r18_cover_depth.json] [--reps 5] [--bench-json FILE]

One process, the items in turn, --reps repeats each after warm-up.  The frame is a box room seen from inside
(tests/_cover_host.box_scene at 480 x 640, a tenth of the pixels without depth), radius 1.0; the map holds 200 or 20 000 active
fields at one density (the room's volume for 200, a hundred rooms' floor area for 20 000), so about the same share of the
frame is covered at both sizes.
  call        ngm_cover_depth alone on preallocated buffers, device events around 20 calls
  kernels     its launches by name, device durations from torch.profiler (one profiled call; None where the profiler gives
              no device events), and the insertions into the global set against the valid pixels (ngm_cover_depth_counters)
  torch       the reference's steps on the device: nonzero, the einsum, a chunked any(d^2 < r^2) for the ball query, the
              three unique calls, the boolean index (rm.py:278-325); it synchronises by itself, host clock ending in a
              synchronise
  extend_map  NeuralGraphRenderer.extend_map on a map with reserved rows, host clock ending in a synchronise: with an idle
              stream, and with five replays of the live training graph enqueued just before (the read-back of the counts
              then waits for them) next to those five replays alone
--bench-json merges a file holding bench.py's result lines of the parent commit and of this tree from the same box.
No speed-up is promised: these are numbers nobody had measured."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cover_host as CH  # noqa: E402
from device_iteration_bench import DEV, T, R, SEED, NETWORKS, _write, sclk_while  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from neural_graph_mapping_amd.keyframes import KeyframeStore  # noqa: E402

H, W, RADIUS, MAX_NEW, PER_FRAME, NUM_POINTS = 480, 640, 1.0, 4096, 5, 500
SIZES = (200, 20000)


def stats(v, digits=3):
    return dict(values=[round(x, digits) for x in v], median=round(statistics.median(v), digits), min=round(min(v), digits),
                max=round(max(v), digits))


def scene(nf):
    depth, c2w, Kx = CH.box_scene(0, H, W)
    g = np.random.default_rng(nf)
    spread = 1.0 if nf <= 200 else 10.0                       # the same density of fields at both sizes
    pos = ((g.random((nf, 3)) - 0.5) * CH.ROOM * [spread, spread, 1.0]).astype(np.float32)
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return to(depth), to(c2w), Kx, to(pos)


class RawCall:
    """ngm_cover_depth on buffers allocated once"""

    def __init__(self, depth, c2w, Kx, pos, shift):
        self.L, nf = K.lib(), pos.shape[0]
        self.shape = (H, W, nf, MAX_NEW)
        self.wsb = self.L.ngm_cover_depth_workspace(*self.shape)
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=DEV)
        self.out, self.counts = torch.zeros(MAX_NEW, 3, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
        self.keep = (depth, c2w, pos, shift)
        self.a = K.CoverDepthArgs(depth.data_ptr(), c2w.data_ptr(), shift.data_ptr(), pos.data_ptr(), None, self.out.data_ptr(),
                                  self.counts.data_ptr(), 1, nf, nf, H, W, MAX_NEW, *Kx, RADIUS, ops.cover_cell(RADIUS))

    def __call__(self):
        K.check(self.L.ngm_cover_depth(C.byref(self.a), self.ws.data_ptr(), self.wsb, ops._stream()), "ngm_cover_depth")

    def counters(self):
        out = (C.c_int32 * 5)()
        K.check(self.L.ngm_cover_depth_counters(*self.shape, self.ws.data_ptr(), out, ops._stream()), "ngm_cover_depth_counters")
        return list(out)


def torch_cover(depth, c2w, Kx, pos, shift, chunk=4096):
    """rm.py:278-325 on the device; the ball query as a chunked any(d^2 < r^2)"""
    fx, fy, cx, cy = Kx
    ijs = torch.nonzero(depth)
    d = depth[ijs[:, 0], ijs[:, 1]]
    cam = torch.stack(((ijs[:, 1].float() - cx) * d / fx, -(ijs[:, 0].float() - cy) * d / fy, -d), -1)
    xyz = torch.einsum("dk,nk->nd", c2w[:3, :3], cam) + c2w[:3, 3]
    covered = torch.cat([(((xyz[s:s + chunk, None] - pos[None]) ** 2).sum(-1) < RADIUS * RADIUS).any(-1) for s in range(0, xyz.shape[0], chunk)])
    xyz = xyz[~covered]
    cell = 2 * RADIUS / np.sqrt(3)
    want = ((xyz + shift) / cell).floor().unique(dim=0)
    have = ((pos + shift) / cell).floor().unique(dim=0)
    _, inv, counts = torch.cat((want, have)).unique(dim=0, return_inverse=True, return_counts=True)
    new = want[counts[inv[:len(want)]] == 1]
    return (new - shift + 0.5) * cell


def event_us(fn, n=20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / n


def wall_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1000.0 / n


def kernel_split(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                us = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0) or 0.0)
                name = e.name.split("(")[0]
                out[name] = round(out.get(name, 0.0) + us, 2)
        return out or None
    except Exception as err:                                  # a measurement aid: its failure must not cost the timings
        return dict(error=str(err)[:200])


def live_renderer(pos, reserve):
    enc, ekw, layers = NETWORKS["m1_fourier"]
    torch.manual_seed(0)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type=enc, encoding_kwargs=ekw, num_layers=layers, dim_out=4, neus_initial_sd=1.0), num_knn=2,
        distance_factor=10.0, outside_value=1.0, field_radius=RADIUS, scale_mode="unit_cube").to(DEV)
    fx, fy, cx, cy = CH.box_scene(0, H, W)[2]
    r = Rr.NeuralGraphRenderer(model, Rr.Camera(W, H, fx, fy, cx, cy, pixel_center=0.0), Rr.shipped_config(), device=DEV)
    nf = pos.shape[0]
    quat = torch.zeros(nf, 4, device=DEV)
    quat[:, 0] = 1.0
    r.add_fields(nf)
    r.set_field_poses(pos.clone(), quat)
    r.reserve_fields(reserve)
    return r


def measure(nf, reps):
    depth, c2w, Kx, pos = scene(nf)
    shift = torch.tensor([0.31, 0.77, 0.52], device=DEV) * ops.cover_cell(RADIUS)
    raw = RawCall(depth, c2w, Kx, pos, shift)
    for _ in range(5):
        raw()
    torch.cuda.synchronize()
    counts = raw.counts.tolist()
    ctr = raw.counters()
    ref = torch_cover(depth, c2w, Kx, pos, shift)
    same = bool(ref.shape[0] == counts[0] and torch.equal(ref, raw.out[:counts[0]]))
    res = dict(num_active=nf, frame=[H, W], radius=RADIUS, counts=dict(num_new=counts[0], status=counts[1], uncovered_valid=counts[2], valid=counts[3]),
               torch_baseline_gives_the_same_rows=same,
               global_set_insertions=ctr[4], insertions_per_valid_pixel=round(ctr[4] / max(ctr[3], 1), 5),
               call_device_us=stats([event_us(raw) for _ in range(reps)], 2),
               kernels_device_us=kernel_split(raw))
    torch_cover(depth, c2w, Kx, pos, shift)
    res["torch_baseline_ms"] = stats([wall_ms(lambda: torch_cover(depth, c2w, Kx, pos, shift), 5) for _ in range(reps)])
    res["call_below_torch_baseline_in_every_repeat"] = bool(max(res["call_device_us"]["values"]) / 1000.0 < min(res["torch_baseline_ms"]["values"]))

    # extend_map on a live map
    r = live_renderer(pos, nf + MAX_NEW)
    store = KeyframeStore(8, H, W, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    rgbd = torch.rand(H, W, 4, device=DEV, generator=g)
    rgbd[..., 3] = depth
    for k in range(3):
        pose = c2w.clone()
        pose[:3, 3] += 0.2 * k
        store.add_keyframe(rgbd, k, c2w=pose)
    store.set_current(rgbd, c2w, frame_id=3)
    ids, cnt = torch.full((nf + MAX_NEW,), -1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    r.observed_fields_device(store.nc_rgbd[0], store.c_c2w[0], num_points=NUM_POINTS, seed=SEED, out=(ids, cnt))
    step = r.capture_training(ids, store.c_c2w, store.nc_rgbd, store.frame_cid_to_ncid, T, R, seed=SEED, current_count=cnt,
                              num_frames=store.num_frames)

    def shrink():                                             # back to nf fields: host mirrors and the device count only
        r._model._set_num(nf)
        r._set_num(nf)
        r._reserved["num_fields_dev"].fill_(nf)

    def extend():
        added = r.extend_map(store.nc_rgbd[1], 0, c2w, store=store, shift=shift)
        assert len(added) == counts[0]
        shrink()

    def replays():
        for _ in range(PER_FRAME):
            step()

    def replays_then_extend():
        replays()
        extend()
    for fn in (extend, replays, replays_then_extend):
        fn()
        fn()
    res["extend_map_ms"] = dict(idle_stream=stats([wall_ms(extend, 10) for _ in range(reps)]),
                                five_replays_alone=stats([wall_ms(replays, 10) for _ in range(reps)]),
                                five_replays_then_extend_map=stats([wall_ms(replays_then_extend, 10) for _ in range(reps)]),
                                fields_added=counts[0])
    res["sclk_mhz_during_calls"] = sclk_while(raw, 500)
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-json", default=None, help="bench.py's result lines of the parent commit and this tree, same box")
    a = ap.parse_args()
    out = dict(tool="tools/cover_depth_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing="call_device_us: HIP events around 20 calls of ngm_cover_depth on preallocated buffers (memset + five launches), "
                      "--reps repeats; kernels_device_us: device durations of one profiled call by kernel name (torch.profiler); "
                      "torch_baseline_ms and extend_map_ms: perf_counter around one call ending in a synchronise, averaged over 5 / 10 "
                      "calls, --reps repeats; extend_map_ms shrinks the map back afterwards (two host mirrors and one fill)",
               sizes=[])
    for nf in SIZES:
        out["sizes"].append(measure(nf, a.reps))
        print(json.dumps(out["sizes"][-1]), flush=True)
        _write(a.out, out)
    if a.bench_json and os.path.exists(a.bench_json):
        out["bench_py_parent_and_this_tree_same_box"] = json.load(open(a.bench_json))
        _write(a.out, out)


if __name__ == "__main__":
    main()
