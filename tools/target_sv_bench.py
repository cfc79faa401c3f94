"""Single-view training-target sampler: the torch-draw sampler (sample_target_sv) against the device sampler
(sample_target_sv_device), and one capture_training_sv replay against the eager sampler + counted step.

    python tools/target_sv_bench.py [--out profiles/r19_target_sv.json] [--calls 50] [--repeats 5]

One process, the items in turn, --repeats repeats of HIP-event medians over --calls calls each.  A 640 x 480 frame of a
synthetic room (a back wall with a box in front of it), 50 000 points, 32 fields x 512 rays, 200 and 20 000 active fields
scattered through the room (a share of them on the visible surfaces).  Per size
  eager          sample_target_sv (torch draws: nonzero, three multinomial, boolean compaction of the hit matrix, host syncs)
  device         sample_target_sv_device (no host sync, padded SvDeviceTarget)
  graph_replay   a torch.cuda.graph replay of the device call
  train_eager / train_replay   sampler + counted optimization_iteration, eager and as one capture_training_sv replay
The shader clock is read while the device call runs; the per-kernel split comes from one child run under
`rocprofv3 --kernel-trace --stats` per size (--trace-child N: a few device calls with N active fields)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from target_sampler_bench import event_median, sclk_while  # noqa: E402

DEV = "cuda"
H, W, FX, CX, CY = 480, 640, 554.2562584220408, 319.5, 239.5
T, R, NP = 32, 512, 50000
SIZES = [200, 20000]
TRACE_CALLS = 10


def room_frame():
    """(H, W, 4): a wall at 5 m with a box at 3 m in front of it, a strip of missing depth"""
    i = torch.arange(H, dtype=torch.float32, device=DEV)[:, None].expand(H, W)
    j = torch.arange(W, dtype=torch.float32, device=DEV)[None, :].expand(H, W)
    depth = torch.full((H, W), 5.0, device=DEV) + 0.3 * torch.sin(j / 90.0)
    depth[160:360, 220:460] = 3.0
    depth[100:110, 50:400] = 0.0
    return torch.stack((i / H, j / W, 0.5 * (i / H + j / W), depth), -1).contiguous()


def scene(num_fields, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    img = room_frame()
    pos = torch.rand(num_fields, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 6.0], device=DEV) - torch.tensor([4.0, 3.0, 7.0], device=DEV)
    n_surf = min(num_fields, 100)                                       # fields on the visible surfaces: the candidates
    ii = torch.randint(120, H, (n_surf,), device=DEV, generator=g)
    jj = torch.randint(0, W, (n_surf,), device=DEV, generator=g)
    d = img[ii, jj, 3]
    pos[:n_surf] = torch.stack(((jj.float() - CX) * d / FX, -(ii.float() - CY) * d / FX, -d), -1)
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
    r.add_fields(num_fields)
    quat = torch.zeros(num_fields, 4, device=DEV)
    quat[:, 0] = 1.0
    r.set_field_poses(pos, quat)
    return r, (img, torch.eye(4, device=DEV), torch.arange(num_fields, device=DEV), T, R)


def repeats(fn, n, calls, warmup):
    runs = [event_median(fn, calls, warmup) for _ in range(n)]
    return dict(median_us=[x["median_us"] for x in runs], median_of_medians_us=statistics.median(x["median_us"] for x in runs))


def measure(num_fields, calls, warmup, n):
    r, args = scene(num_fields)
    torch.manual_seed(0)
    eager = lambda: r.sample_target_sv(*args, num_points=NP)
    device = lambda: r.sample_target_sv_device(*args, num_points=NP, seed=1)
    t = device()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        device()
    res = dict(active_fields=num_fields, image=[H, W], num_points=NP, num_train_fields=T, rays_per_field=R,
               capacity=int(t.field_ids.shape[0]), rows=int(t.count), candidates=int(t.num_candidates))
    res["eager_us"] = repeats(eager, n, calls, warmup)
    res["device_us"] = repeats(device, n, calls, warmup)
    res["graph_replay_us"] = repeats(g.replay, n, calls, warmup)
    res["device_below_eager_in_every_repeat"] = max(res["device_us"]["median_us"]) < min(res["eager_us"]["median_us"])
    res["sclk_mhz_during_device"] = sclk_while(device, n=500)
    train_eager = lambda: r.optimization_iteration(r.sample_target_sv_device(*args, num_points=NP, seed=1), seed=1)
    res["train_eager_us"] = repeats(train_eager, n, calls, warmup)
    step = r.capture_training_sv(*args, num_points=NP, seed=1)
    res["train_replay_us"] = repeats(step, n, calls, warmup)
    return res


def trace_child(num_fields):
    r, args = scene(num_fields)
    for _ in range(1 + TRACE_CALLS):
        r.sample_target_sv_device(*args, num_points=NP, seed=1)
    torch.cuda.synchronize()


def kernel_split(num_fields):
    """average time per kernel of the device call from `rocprofv3 --kernel-trace --stats` over a fresh child process"""
    d = tempfile.mkdtemp(prefix="tssv_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", str(num_fields)]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except Exception as e:                                          # no profiler on this machine
        return dict(error=f"{type(e).__name__}: {e}")
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not stats:
        return dict(error=f"rocprofv3 exit {p.returncode}", tail=p.stderr[-600:])
    rows = [row for row in csv.DictReader(open(stats[0])) if "k_tssv" in row["Name"] or "k_obs" in row["Name"]]
    calls = 1 + TRACE_CALLS
    return dict(active_fields=num_fields, calls=calls,
                launches_per_call={row["Name"].split("(")[0]: int(row["Calls"]) / calls for row in rows},
                avg_us={row["Name"].split("(")[0]: round(float(row["AverageNs"]) / 1000.0, 2) for row in rows})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-child", type=int, default=None, metavar="ACTIVE_FIELDS")
    a = ap.parse_args()
    if a.trace_child is not None:
        trace_child(a.trace_child)
        return
    out = dict(tool="tools/target_sv_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing="HIP-event median per call over --calls calls after --warmup untimed ones, --repeats times in turn",
               calls=a.calls, repeats=a.repeats, sizes=[])
    for nf in SIZES:
        out["sizes"].append(measure(nf, a.calls, a.warmup, a.repeats))
        print(json.dumps(out["sizes"][-1]), flush=True)
    out["kernels"] = [kernel_split(nf) for nf in SIZES]
    print(json.dumps(out["kernels"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
