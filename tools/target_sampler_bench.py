"""Training-target sampler: the torch-draw sampler (sample_target_mv) against the device sampler (sample_target_mv_device).

    python tools/target_sampler_bench.py [--out profiles/r07_target_sampler.json] [--calls 200]

Synthetic scenes on the device: 200- and 10 000-field maps, 100 and 1 000 keyframes of 640 x 480, 100 current fields,
32 fields x 512 rays.  Per scene, HIP-event medians over --calls calls of
  eager          sample_target_mv (torch draws: multinomial / unique / randn / rand + boolean compactions, host syncs)
  device_padded  sample_target_mv_device (three kernels, no host sync, padded DeviceTarget)
  device_materialize  the same + DeviceTarget.materialize() (one host sync: reading the count)
  graph_replay   a torch.cuda.graph replay of the padded call (iteration counter advanced inside the graph)
The shader clock is read while the padded call runs; the launches per call come from one child run under
`rocprofv3 --kernel-trace --stats` (--trace-child: a few padded calls of the first scene)."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402

DEV = "cuda"
H, W, FX, CX, CY = 480, 640, 554.2562584220408, 319.5, 239.5
T, R, NCUR = 32, 512, 100
SCENES = [(200, 100), (200, 1000), (10000, 100), (10000, 1000)]
TRACE_CALLS = 10


def scene(num_fields, num_frames, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    pos = torch.rand(num_fields, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 5.0], device=DEV) - torch.tensor([4.0, 3.0, 7.0], device=DEV)
    c2w = torch.eye(4, device=DEV).repeat(num_frames, 1, 1)
    c2w[:, :3, 3] = torch.rand(num_frames, 3, device=DEV, generator=g) * 4.0 - 2.0
    rgbd = torch.rand(num_frames, H, W, 4, device=DEV, generator=g)
    rgbd[..., 3] = 2.0 + 8.0 * rgbd[..., 3]
    cur = torch.randperm(num_fields, device=DEV, generator=g)[:NCUR]
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=32, mu=0.0, sigma=4.0, raw_coords=True), num_layers=1, dim_out=4,
        neus_initial_sd=1.0, skip_mode="no"), num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=1.0,
        scale_mode="unit_cube").to(DEV)
    cam = Rr.Camera(W, H, FX, FX, CX, CY, pixel_center=0.0)
    cfg = dict(geometry_mode="nrgbd", geometry_factor=20.0, color_factor=1.0, truncation_distance=0.1, field_radius=1.0,
               termination_weight=0.0, photometric_weight=1.0, photometric_loss="l1", depth_weight=1.0, depth_loss="huber",
               freespace_weight=40.0, tsdf_weight=50.0, learning_rate=1e-3, adam_eps=1e-15, adam_weight_decay=1e-5,
               near_distance=0.0, far_distance=8.0, num_samples_coarse=4, num_samples_depth_guided=4)
    r = Rr.NeuralGraphRenderer(model, cam, cfg, device=DEV)
    r.set_field_poses(pos, torch.zeros(num_fields, 4, device=DEV))
    args = (cur, c2w, rgbd.contiguous(), torch.arange(num_frames, device=DEV), T, R)
    return r, args


def event_median(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1000.0 for a, b in ev)
    return dict(median_us=round(statistics.median(t), 2), p10_us=round(t[len(t) // 10], 2), p90_us=round(t[(9 * len(t)) // 10], 2))


def sclk_while(fn, n=3000):
    """sclk as rocm-smi reports it while n more calls are queued (None if it cannot be read)"""
    try:
        for _ in range(n):
            fn()
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        torch.cuda.synchronize()
        js = json.loads(out[out.index("{"):])
        card = js[sorted(js)[0]]
        for k, v in card.items():
            m = re.search(r"(\d+)\s*Mhz", str(v), re.I) if "sclk" in k.lower() else None
            if m:
                return int(m.group(1))
    except Exception:
        torch.cuda.synchronize()
    return None


def measure(num_fields, num_frames, calls, warmup):
    r, args = scene(num_fields, num_frames)
    torch.manual_seed(0)
    eager = lambda: r.sample_target_mv(*args)
    padded = lambda: r.sample_target_mv_device(*args, seed=1)
    mat = lambda: r.sample_target_mv_device(*args, seed=1).materialize()
    t = padded()
    counts = [int(r.sample_target_mv_device(*args, seed=1, iteration=i).count) for i in range(20)]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        padded()
    res = dict(num_fields=num_fields, num_frames=num_frames, image=[H, W], current_fields=NCUR, num_train_fields=T,
               rays_per_field=R, capacity=int(t.field_ids.shape[0]), surviving_fields_first20=counts)
    res["eager_us"] = event_median(eager, calls, warmup)
    res["device_padded_us"] = event_median(padded, calls, warmup)
    res["device_materialize_us"] = event_median(mat, calls, warmup)
    res["graph_replay_us"] = event_median(g.replay, calls, warmup)
    res["sclk_mhz_during_padded"] = sclk_while(padded)
    return res


def trace_child():
    r, args = scene(*SCENES[0])
    r.sample_target_mv_device(*args, seed=1)
    torch.cuda.synchronize()
    for _ in range(TRACE_CALLS):
        r.sample_target_mv_device(*args, seed=1)
    torch.cuda.synchronize()


def launch_counts():
    """kernels per padded call from `rocprofv3 --kernel-trace --stats` over 1 + TRACE_CALLS calls of a fresh child process"""
    d = tempfile.mkdtemp(prefix="tsmv_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except Exception as e:                                          # no profiler on this machine
        return dict(error=f"{type(e).__name__}: {e}")
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not stats:
        return dict(error=f"rocprofv3 exit {p.returncode}", tail=p.stderr[-600:])
    rows = list(csv.DictReader(open(stats[0])))
    per = {row["Name"]: int(row["Calls"]) for row in rows}
    mine = {k.split("(")[0]: v for k, v in per.items() if "tsmv" in k}
    avg = {row["Name"].split("(")[0]: round(float(row["AverageNs"]) / 1000.0, 2) for row in rows if "tsmv" in row["Name"]}
    calls = 1 + TRACE_CALLS
    return dict(command="rocprofv3 --kernel-trace --stats --output-format csv -- python tools/target_sampler_bench.py --trace-child",
                scene=list(SCENES[0]), calls=calls, sampler_kernels=mine, sampler_kernels_per_call=sum(mine.values()) / calls,
                sampler_kernel_avg_us=avg, all_kernels_in_process=sum(per.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child()
        return
    out = dict(tool="tools/target_sampler_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing="HIP-event median per call over --calls calls after --warmup untimed ones", calls=a.calls, scenes=[])
    for nf, nc in SCENES:
        out["scenes"].append(measure(nf, nc, a.calls, a.warmup))
        print(json.dumps(out["scenes"][-1]), flush=True)
    out["launches"] = launch_counts()
    print(json.dumps(out["launches"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
