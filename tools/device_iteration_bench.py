"""Training iteration fed from the device sampler: materialised, counted eager, and one captured graph.

    python tools/device_iteration_bench.py [--out profiles/r08_device_iteration.json] [--iters 300] [--reps 5]

Map and keyframe store of tools/target_sampler_bench.py's first scene (200 fields, 100 keyframes of 640 x 480, 100 current
fields), 32 train fields x 512 rays x (8 + 16) samples, once with the reference's default hash network and once with the
M1 Fourier network (64 + 2 x 64).  Three loops, each on a renderer of its own, alternated inside this one process after
warm-up; every timed block is --iters iterations between two HIP events, --reps blocks per loop:
  1 materialised  sample_target_mv_device -> DeviceTarget.materialize() -> optimization_iteration   (one host sync, F varies)
  2 counted       sample_target_mv_device -> optimization_iteration(DeviceTarget)                    (eager launches at Fcap)
  3 graph         one capture_training replay                                                           (sampler + step, one graph)
Reported per loop: us per iteration of every block, their median and spread (max - min), the host synchronisations per
iteration (calls of Tensor.item / torch.cuda.synchronize counted while the loop runs), and -- first network only -- the
kernel launches per iteration from child runs under `rocprofv3 --kernel-trace --stats` (two run lengths, differenced, so
that set-up and capture do not count).  The shader clock is read while loop 3 runs."""
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
NF, NKF, T, R, NCUR, SEED = 200, 100, 32, 512, 100, 1
NETWORKS = {
    "hash": ("neural_graph_mapping.positional_encodings.PermutohedralEncoding",
             dict(pos_dim=3, log2_hashmap_size=12, nr_levels=16, nr_feat_per_level=2, coarsest_scale=1, finest_scale=0.0001,
                  init_scale=0.00001), 1),
    "m1_fourier": ("neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
                   dict(dim_in=3, dim_out=64, mu=0.0, sigma=4.0, raw_coords=True), 2),
}
LOOPS = ("materialised", "counted", "graph")
TRACE_SHORT, TRACE_LONG = 10, 40


def scene():
    g = torch.Generator(device=DEV).manual_seed(0)
    pos = torch.rand(NF, 3, device=DEV, generator=g) * torch.tensor([8.0, 6.0, 5.0], device=DEV) - torch.tensor([4.0, 3.0, 7.0], device=DEV)
    c2w = torch.eye(4, device=DEV).repeat(NKF, 1, 1)
    c2w[:, :3, 3] = torch.rand(NKF, 3, device=DEV, generator=g) * 4.0 - 2.0
    rgbd = torch.rand(NKF, H, W, 4, device=DEV, generator=g)
    rgbd[..., 3] = 2.0 + 8.0 * rgbd[..., 3]
    cur = torch.randperm(NF, device=DEV, generator=g)[:NCUR].contiguous()
    quat = torch.zeros(NF, 4, device=DEV)
    quat[:, 0] = 1.0
    return pos, quat, (cur, c2w.contiguous(), rgbd.contiguous(), torch.arange(NKF, device=DEV), T, R)


def renderer(network, pos, quat):
    enc, ekw, layers = NETWORKS[network]
    torch.manual_seed(0)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type=enc, encoding_kwargs=ekw, num_layers=layers, dim_out=4, neus_initial_sd=1.0), num_knn=2,
        distance_factor=10.0, outside_value=1.0, field_radius=1.0, scale_mode="unit_cube").to(DEV)
    cam = Rr.Camera(W, H, FX, FX, CX, CY, pixel_center=0.0)
    r = Rr.NeuralGraphRenderer(model, cam, Rr.shipped_config(), device=DEV)
    r.add_fields(NF)
    r.set_field_poses(pos, quat)
    return r


def make_loop(name, network, pos, quat, args):
    """(callable running ONE iteration, renderer)"""
    r = renderer(network, pos, quat)
    if name == "materialised":
        return (lambda: r.optimization_iteration(r.sample_target_mv_device(*args, seed=SEED).materialize(), seed=SEED)), r
    if name == "counted":
        return (lambda: r.optimization_iteration(r.sample_target_mv_device(*args, seed=SEED), seed=SEED)), r
    step = r.capture_training(*args, seed=SEED)
    return step, r


class SyncCounter:
    """host synchronisations the Python layer asks for: Tensor.item and torch.cuda.synchronize calls while active"""

    def __enter__(self):
        self.n = 0
        self._item, self._sync = torch.Tensor.item, torch.cuda.synchronize

        def item(t):
            self.n += 1
            return self._item(t)

        def sync(*a, **k):
            self.n += 1
            return self._sync(*a, **k)
        torch.Tensor.item, torch.cuda.synchronize = item, sync
        return self

    def __exit__(self, *exc):
        torch.Tensor.item, torch.cuda.synchronize = self._item, self._sync


def block_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters


def sclk_while(fn, n=2000):
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


def measure(network, iters, reps, warmup):
    pos, quat, args = scene()
    loops = {n: make_loop(n, network, pos, quat, args) for n in LOOPS}
    for n in LOOPS:
        for _ in range(warmup):
            loops[n][0]()
    torch.cuda.synchronize()
    blocks = {n: [] for n in LOOPS}
    for _ in range(reps):                                   # alternated: a clock or thermal drift hits all three alike
        for n in LOOPS:
            blocks[n].append(round(block_us(loops[n][0], iters), 2))
    res = dict(network=network, num_fields=NF, num_frames=NKF, image=[H, W], current_fields=NCUR, num_train_fields=T,
               rays_per_field=R, samples_per_ray=[8, 16], iters_per_block=iters, blocks_per_loop=reps, loops={})
    probe = loops["counted"][1].sample_target_mv_device(*args, seed=SEED, iteration=0)
    res["capacity"] = int(probe.field_ids.shape[0])
    res["active_fields_first20"] = [int(loops["counted"][1].sample_target_mv_device(*args, seed=SEED, iteration=i).count)
                                    for i in range(20)]
    for n in LOOPS:
        with SyncCounter() as sc:
            for _ in range(50):
                loops[n][0]()
        torch.cuda.synchronize()
        v = blocks[n]
        res["loops"][n] = dict(us_per_iteration=v, median_us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2),
                               host_syncs_per_iteration=sc.n / 50)
    med = {n: res["loops"][n]["median_us"] for n in LOOPS}
    spread = max(res["loops"][n]["spread_us"] for n in LOOPS)
    res["ordering_graph_lt_counted_lt_materialised"] = bool(med["graph"] < med["counted"] < med["materialised"])
    res["ordering_gaps_us"] = dict(counted_minus_graph=round(med["counted"] - med["graph"], 2),
                                   materialised_minus_counted=round(med["materialised"] - med["counted"], 2),
                                   largest_spread_of_one_loop=spread)
    res["ordering_holds_beyond_spread"] = bool(med["counted"] - med["graph"] > spread and med["materialised"] - med["counted"] > spread)
    res["sclk_mhz_during_graph_loop"] = sclk_while(loops["graph"][0])
    return res


def trace_child(network, loop, n):
    pos, quat, args = scene()
    fn, _ = make_loop(loop, network, pos, quat, args)
    torch.cuda.synchronize()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()


def kernels_in_child(network, loop, n):
    d = tempfile.mkdtemp(prefix="devit_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", network, loop, str(n)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not stats:
        raise RuntimeError(f"rocprofv3 exit {p.returncode}: {p.stderr[-400:]}")
    return sum(int(row["Calls"]) for row in csv.DictReader(open(stats[0])))


def launch_counts(network):
    """kernel launches per iteration: (kernels of a TRACE_LONG-iteration child - kernels of a TRACE_SHORT one) / difference"""
    out = dict(command="rocprofv3 --kernel-trace --stats --output-format csv -- python tools/device_iteration_bench.py "
                       "--trace-child NETWORK LOOP N", network=network, iterations=[TRACE_SHORT, TRACE_LONG])
    for loop in LOOPS:
        try:
            a, b = kernels_in_child(network, loop, TRACE_SHORT), kernels_in_child(network, loop, TRACE_LONG)
        except FileNotFoundError as e:                       # no profiler installed: nothing was started, say so and go on
            out[loop] = dict(error=f"{type(e).__name__}: {e}")
            continue
        except Exception as e:
            # a child failed, faulted or ran into its time limit (its python process may still hold the GPU): record it and
            # start NOTHING more on the card in this call
            out[loop] = dict(error=f"{type(e).__name__}: {e}")
            out["stopped"] = f"after the failure of loop {loop!r}: no further child run"
            break
        out[loop] = dict(kernels=[a, b], launches_per_iteration=(b - a) / (TRACE_LONG - TRACE_SHORT))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", nargs=3, metavar=("NETWORK", "LOOP", "N"))
    a = ap.parse_args()
    if a.trace_child:
        trace_child(a.trace_child[0], a.trace_child[1], int(a.trace_child[2]))
        return
    out = dict(tool="tools/device_iteration_bench.py", device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing="HIP events around blocks of --iters iterations; --reps blocks per loop, the three loops alternated in one "
                      "process after --warmup untimed iterations each", networks=[])
    for net in NETWORKS:
        out["networks"].append(measure(net, a.iters, a.reps, a.warmup))
        print(json.dumps(out["networks"][-1]), flush=True)
    if not a.no_trace:
        out["launches"] = launch_counts(next(iter(NETWORKS)))
        print(json.dumps(out["launches"]), flush=True)
    _write(a.out, out)
    if out.get("launches", {}).get("stopped"):
        sys.exit(1)


def _write(path, out):
    if not path:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
