"""Scoring a mesh on the device: mesh.evaluate_mesh (surface sampler + two exact nearest-point queries + reductions) timed
stage by stage, against the reference's path on the host (scipy.spatial.KDTree build + query, evaluation.py:75-130) and
against chunked brute force in torch on the device.

    python tools/mesh_metrics_bench.py [--out profiles/r13_mesh_metrics.json] [--reps 5] [--points 200000]

Workload: the mesh extract_mesh gives for the room map of tools/mesh_bench.py (200 fields, m1_fourier, 0.02 m) as the estimate
and a perturbed copy of it (every vertex moved by N(0, 1 cm)) as the ground truth, `--points` surface samples of each.
One process; after one warm-up of every item the items are run in turn, `--reps` times: device events around 20 calls of the
sampler and of each of the two nearest-point calls, host clock around 20 calls of the whole evaluate_mesh (each ends in a
transfer of ten numbers) and a final synchronise, around one call of the torch brute force and of the KDTree; times per call.
Also recorded: the nearest-point call on queries binned first (sorted by the cell of a 10 cm grid: the sort's own time and the
query's on the sorted cloud) against the queries as sampled -- the figure behind the decision not to bin inside the call."""
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
from device_iteration_bench import DEV, _write  # noqa: E402
from mesh_bench import extract, make  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402


INNER = 20            # calls per repeat of the sub-millisecond items: a repeat is then several milliseconds of device work


def device_ms(fn, inner=1):
    """ms per call between two device events around `inner` calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner, out


def host_ms(fn, inner=1):
    """ms per call by the host clock around `inner` calls and a final synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def shader_clock_under_load(fn, n=300):
    """sclk as rocm-smi reports it while the GPU works through n more calls (read only); None if it cannot be read"""
    import re
    import subprocess
    try:
        for _ in range(n):
            fn()
        r = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20)
        torch.cuda.synchronize()
        js = json.loads(r.stdout[r.stdout.index("{"):])
        for k, v in js[sorted(js)[0]].items():
            if "sclk" in k.lower():
                m = re.search(r"(\d+)\s*Mhz", str(v), re.I)
                if m:
                    return int(m.group(1))
    except Exception:
        torch.cuda.synchronize()
    return None


def brute_force(q, r, chunk=1024):
    """chunked brute force on the device: explicit differences (no matrix trick), min over the references.  Written out axis
    by axis: torch.cdist(compute_mode="donot_use_mm_for_euclid_dist") on 2048 x 200 000 chunks gave distances up
    to 0.12 m away from the KDTree's on an MI355X, this form agrees to rounding"""
    out = []
    rx, ry, rz = r[:, 0][None], r[:, 1][None], r[:, 2][None]
    for s in range(0, len(q), chunk):
        c = q[s:s + chunk]
        d2 = (c[:, 0:1] - rx).square_()
        d2 += (c[:, 1:2] - ry).square_()
        d2 += (c[:, 2:3] - rz).square_()
        out.append(d2.min(1).values.sqrt_())
    return torch.cat(out)


def bin_queries(q, cell=0.1):
    """queries sorted by the cell of a uniform grid (x fastest): what binning inside the call would have to do first"""
    g = ((q - q.min(0).values) / cell).floor().long()
    n = g.max(0).values + 1
    return q[torch.argsort((g[:, 2] * n[1] + g[:, 1]) * n[0] + g[:, 0])]


def summary(v):
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), all_ms=[round(x, 3) for x in v])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=200000)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_metrics_bench needs the MI355X: there is no CPU fallback to time"
    r = make("m1_fourier")
    verts, faces, _ = extract(r, 0.02, 200, True)
    g = torch.Generator(device=DEV).manual_seed(13)
    gt_verts = verts + 0.01 * torch.randn(verts.shape, device=DEV, generator=g)
    N = a.points
    est_pts = Mh.sample_surface(verts, faces, N, 0)[0]
    gt_pts = Mh.sample_surface(gt_verts, faces, N, 1)[0]
    try:
        from scipy import spatial
        est_np, gt_np = est_pts.cpu().numpy().astype("float64"), gt_pts.cpu().numpy().astype("float64")
        kdtree = lambda: spatial.KDTree(gt_np).query(est_np)[0]
        scipy_note = "scipy " + __import__("scipy").__version__
    except ImportError:
        kdtree, scipy_note = None, "scipy does not import on this machine: no KDTree figure"
    items = dict(
        sampler=lambda: device_ms(lambda: Mh.sample_surface(verts, faces, N, 0), INNER)[0],
        nearest_est_to_gt=lambda: device_ms(lambda: Mh.nearest_distances(est_pts, gt_pts), INNER)[0],
        nearest_gt_to_est=lambda: device_ms(lambda: Mh.nearest_distances(gt_pts, est_pts), INNER)[0],
        evaluate_mesh=lambda: host_ms(lambda: Mh.evaluate_mesh((verts, faces), (gt_verts, faces), N, 0), INNER)[0],
        torch_brute_force_est_to_gt=lambda: host_ms(lambda: brute_force(est_pts, gt_pts))[0],
        bin_queries_sort=lambda: device_ms(lambda: bin_queries(est_pts), INNER)[0],
        nearest_est_to_gt_binned_queries=lambda: device_ms(lambda: Mh.nearest_distances(binned, gt_pts), INNER)[0])
    if kdtree is not None:
        items["scipy_kdtree_build_and_query_est_to_gt"] = lambda: host_ms(kdtree)[0]
    binned = bin_queries(est_pts)
    # the three ways agree before anything is timed
    d = Mh.nearest_distances(est_pts, gt_pts)[0]
    check = dict(max_abs_diff_vs_torch_brute_force=float((d - brute_force(est_pts, gt_pts)).abs().max()))
    if kdtree is not None:
        check["max_abs_diff_vs_scipy_kdtree"] = float((d.cpu().double() - torch.from_numpy(kdtree())).abs().max())
    times = {k: [] for k in items}
    for k, fn in items.items():                                            # warm-up
        fn()
    for _ in range(a.reps):
        for k, fn in items.items():
            times[k].append(fn())
    metrics = Mh.evaluate_mesh((verts, faces), (gt_verts, faces), N, 0)
    sclk = shader_clock_under_load(lambda: Mh.nearest_distances(est_pts, gt_pts))
    res = {k: summary(v) for k, v in times.items()}
    binned_total = [s + q for s, q in zip(times["bin_queries_sort"], times["nearest_est_to_gt_binned_queries"])]
    out = dict(tool="tools/mesh_metrics_bench.py", command=f"python tools/mesh_metrics_bench.py --out profiles/r13_mesh_metrics.json --reps {a.reps} --points {N}",
               device=torch.cuda.get_device_name(0), sclk_mhz=sclk, scipy=scipy_note,
               workload=f"{N} surface samples each of the room map's extracted mesh ({len(verts)} vertices, {len(faces)} faces; tools/mesh_bench.py, "
                        "m1_fourier, 0.02 m) and of a copy with every vertex moved by N(0, 1 cm)",
               procedure=f"one process, one warm-up of every item, then the items in turn, {a.reps} repeats; ms per call: device events around "
                         f"{INNER} calls of the sampler, of each nearest-point call and of the query sort, host clock around {INNER} calls of "
                         "evaluate_mesh (each ends in its transfer of ten numbers) and a final synchronise, host clock around one call of the "
                         "torch brute force and of the KDTree; sclk_mhz: rocm-smi while 300 more nearest-point calls run",
               times=res, agreement=check, metrics=metrics,
               binned_queries=dict(sort_plus_query_median_ms=round(statistics.median(binned_total), 3),
                                   unbinned_query_median_ms=res["nearest_est_to_gt"]["median_ms"],
                                   binning_pays=bool(max(binned_total) < min(times["nearest_est_to_gt"]))))
    _write(a.out, out)
    print(json.dumps(dict(times={k: v["median_ms"] for k, v in res.items()}, agreement=check, binned_queries=out["binned_queries"])))


if __name__ == "__main__":
    main()
