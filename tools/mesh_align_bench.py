"""Aligning a mesh to the ground truth on the device (mesh.align_mesh: ngm_mesh_vertex_normals + ngm_icp_point_to_plane) against
what the tree allowed before: the same point-to-plane ICP written in torch on the device, mesh.nearest_distances per iteration
(the grid rebuilt every time), the normal equations through HBM and the convergence test read on the host.

    python tools/mesh_align_bench.py [--target walls|map] [--out profiles/r16_mesh_align.json] [--reps 5] [--poses 1000] [--bench-json FILE]

Workload: the mesh extract_mesh gives for the room map of tools/mesh_bench.py (m1_fourier, 0.02 m), moved by Rz(1 deg) and 1 cm
so that there is something to align, against (--target walls) the room's two-triangles-per-wall ground truth subdivided to 0.1 m
and culled from `--poses` poses (mesh.cull_mesh(max_edge=0.1)) -- the reference's order; the synthetic map's surfaces are not the
room's walls, so only a twentieth of the vertices finds a correspondence -- or (--target map) the unmoved extracted mesh itself,
culled the same way: a target that fits, two million points on either side.
One process; after one warm-up of every item the items are run in turn, `--reps` times.  Device events around: the normals; an
ICP call that cannot converge (relative_fitness = relative_rmse = -1) with max_iteration 0 and 10, from which a pass (accumulate
+ solve) is (t10 - t0) / 10; the same two calls with ONE source point (an accumulate with nothing to do + solve: the floor of a
pass); ngm_nearest_point on the same clouds and with one query that lies on the target (the grid build), whose difference is the query alone.  Host clock
ending in a synchronise around the whole align_mesh and around the torch loop.  --bench-json merges a file holding bench.py's
result lines of the parent commit and of this tree from the same box."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, _write  # noqa: E402
from mesh_bench import extract, make  # noqa: E402
from mesh_cull_bench import F, H, W, room_mesh, room_poses  # noqa: E402
from mesh_metrics_bench import device_ms, host_ms, shader_clock_under_load, summary  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402
from neural_graph_mapping_amd.renderer import Camera  # noqa: E402


def update_matrix(x):
    ca, sa, cb, sb, cg, sg = (f(x[i]) for i in range(3) for f in (math.cos, math.sin))
    u = np.eye(4)
    u[:3, :3] = [[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa], [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                 [-sb, cb * sa, cb * ca]]
    u[:3, 3] = x[3:6]
    return u


def torch_icp(source, target, normals, threshold=0.1, max_iteration=100, relative_fitness=1e-6, relative_rmse=1e-6):
    """registration_icp (point to plane) as the tree allowed it before: per iteration one nearest_distances call, the sums as torch
    reductions in fp64, ONE transfer of 29 numbers, the 6 x 6 solve and the convergence test on the host"""
    T = np.eye(4)
    s, t, n = source.double(), target.double(), normals.double()
    fitness0 = rmse0 = 0.0
    k = 0
    for k in range(max_iteration + 1):
        Td = torch.from_numpy(T).to(DEV)
        p = s @ Td[:3, :3].T + Td[:3, 3]
        _, idx = Mh.nearest_distances(p.float(), target)
        safe = idx.clamp(min=0)
        diff, nn = p - t[safe], n[safe]
        d2 = (diff * diff).sum(1)
        ok = ((idx >= 0) & (d2.sqrt() < threshold) & torch.isfinite(nn).all(1)).double()
        J = torch.cat([torch.cross(p, nn, dim=1), nn], 1) * ok[:, None]
        r = (diff * nn).sum(1) * ok
        vals = torch.cat([(J.T @ J).reshape(-1), J.T @ r, (d2 * ok).sum()[None], ok.sum()[None]]).tolist()       # the read-back
        A, b, sum_d2, count = np.array(vals[:36]).reshape(6, 6), -np.array(vals[36:42]), vals[42], vals[43]
        fitness, rmse = count / len(s), math.sqrt(sum_d2 / count) if count > 0 else 0.0
        if k >= 1 and abs(fitness - fitness0) < relative_fitness and abs(rmse - rmse0) < relative_rmse:
            return T, fitness, rmse, k, True
        if k == max_iteration:
            break
        fitness0, rmse0 = fitness, rmse
        try:
            x = np.linalg.solve(A, b)
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(x).all() and count > 0:
            T = update_matrix(x) @ T
    return T, fitness, rmse, k, False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--target", choices=("walls", "map"), default="walls",
                    help="walls: the room's ground truth, subdivided and culled; map: the unmoved extracted mesh itself, culled (a target that fits)")
    ap.add_argument("--bench-json", default=None, help="bench.py's result lines of the parent commit and this tree, same box")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_align_bench needs the MI355X: there is no CPU fallback to time"
    r = make("m1_fourier")
    verts, faces, _ = extract(r, 0.02, 200, True)
    motion = update_matrix([0.0, 0.0, math.radians(1.0), 0.01, -0.005, 0.005])
    est_v = Mh.transform_vertices(verts, torch.from_numpy(motion).to(DEV))
    cam = Camera(W, H, F, F, W / 2, H / 2, pixel_center=0.5)
    gt = room_mesh() if a.target == "walls" else (verts, faces)
    gt_v, gt_f = Mh.cull_mesh(gt[0], gt[1], room_poses(a.poses), cam, "occlusion", max_edge=0.1)
    gt_n = Mh.vertex_normals(gt_v, gt_f)
    print(json.dumps(dict(stage="workload", source_vertices=len(est_v), target_vertices=len(gt_v), target_faces=len(gt_f))), flush=True)

    (moved, _), res = Mh.align_mesh((est_v, faces), (gt_v, gt_f))
    ours = dict(iterations=int(res.iterations), converged=bool(res.converged), fitness=float(res.fitness), inlier_rmse=float(res.inlier_rmse))
    tT, tf, tr, tk, tc = torch_icp(est_v, gt_v, gt_n)
    theirs = dict(iterations=tk, converged=tc, fitness=tf, inlier_rmse=tr)
    back = res.transformation.cpu().numpy() @ motion
    agreement = dict(device=ours, torch_loop=theirs, worst_difference_of_the_transformations=float(np.abs(res.transformation.cpu().numpy() - tT).max()),
                     residual_rotation_frobenius=float(np.linalg.norm(back[:3, :3] - np.eye(3))), residual_translation=float(np.linalg.norm(back[:3, 3])),
                     worst_vertex_distance_before=float((est_v - verts).norm(dim=1).max()), worst_vertex_distance_after=float((moved - verts).norm(dim=1).max()))
    print(json.dumps(dict(stage="agreement", **agreement)), flush=True)

    one = est_v[:1].contiguous()
    near = gt_v[:1].contiguous()                          # a query ON the target: its search ends in the first ring, the call is the grid build
    icp = lambda s, it: torch.ops.ngm355.icp_point_to_plane(s, gt_v, gt_n, 0.1, it, -1.0, -1.0, [float(v) for v in np.eye(4).ravel()])
    items = {
        "vertex_normals": lambda: device_ms(lambda: torch.ops.ngm355.mesh_vertex_normals(gt_v, gt_f))[0],
        "vertex_normals_of_the_estimate": lambda: device_ms(lambda: torch.ops.ngm355.mesh_vertex_normals(est_v, faces))[0],
        "icp_0_iterations": lambda: device_ms(lambda: icp(est_v, 0))[0],
        "icp_10_iterations": lambda: device_ms(lambda: icp(est_v, 10))[0],
        "icp_0_iterations_one_point": lambda: device_ms(lambda: icp(one, 0))[0],
        "icp_10_iterations_one_point": lambda: device_ms(lambda: icp(one, 10))[0],
        "nearest_point": lambda: device_ms(lambda: torch.ops.ngm355.nearest_point(est_v, gt_v))[0],
        "nearest_point_one_query": lambda: device_ms(lambda: torch.ops.ngm355.nearest_point(near, gt_v))[0],
        "align_mesh/whole": lambda: host_ms(lambda: Mh.align_mesh((est_v, faces), (gt_v, gt_f)))[0],
        "align_mesh/torch_loop": lambda: host_ms(lambda: torch_icp(est_v, gt_v, Mh.vertex_normals(gt_v, gt_f)))[0],
    }
    times = {k: [] for k in items}
    for k, fn in items.items():
        fn()
        print(json.dumps(dict(stage="warm-up", item=k)), flush=True)
    for rep in range(a.reps):
        for k, fn in items.items():
            times[k].append(fn())
        print(json.dumps(dict(stage="repeat", n=rep, **{k: round(v[-1], 3) for k, v in times.items()})), flush=True)
    sclk = shader_clock_under_load(lambda: icp(est_v, 0), n=50)
    out_times = {k: summary(v) for k, v in times.items()}
    med = {k: v["median_ms"] for k, v in out_times.items()}
    derived = dict(pass_accumulate_plus_solve_ms=round((med["icp_10_iterations"] - med["icp_0_iterations"]) / 10, 4),
                   pass_floor_one_point_ms=round((med["icp_10_iterations_one_point"] - med["icp_0_iterations_one_point"]) / 10, 4),
                   nearest_point_query_alone_ms=round(med["nearest_point"] - med["nearest_point_one_query"], 4),
                   grid_build_ms=med["nearest_point_one_query"],
                   device_below_torch_loop_in_every_repeat=all(o < t for o, t in zip(times["align_mesh/whole"], times["align_mesh/torch_loop"])),
                   speedup_median=round(med["align_mesh/torch_loop"] / med["align_mesh/whole"], 2))
    derived["accumulate_work_ms"] = round(derived["pass_accumulate_plus_solve_ms"] - derived["pass_floor_one_point_ms"], 4)
    out = dict(tool="tools/mesh_align_bench.py",
               command=f"python tools/mesh_align_bench.py --target {a.target} --out <file> --reps {a.reps} --poses {a.poses}"
                       + (" --bench-json <bench.py lines>" if a.bench_json else ""),
               device=torch.cuda.get_device_name(0), torch=torch.__version__, sclk_mhz=sclk,
               workload=f"source: the room map's extracted mesh ({len(est_v)} vertices, {len(faces)} faces; tools/mesh_bench.py, m1_fourier, 0.02 m) moved by "
                        f"Rz(1 deg), t = (0.01, -0.005, 0.005); target: "
                        + ("the room with two triangles per wall" if a.target == "walls" else "the unmoved extracted mesh") + f", subdivided to 0.1 m and culled from {a.poses} poses "
                        f"at {W} x {H} ({len(gt_v)} vertices, {len(gt_f)} faces); threshold 0.1, at most 100 iterations, relative criteria 1e-6",
               procedure=f"one process, one warm-up of every item, then the items in turn, {a.reps} repeats; device events around the ops; icp_*: an ICP call that "
                         "cannot converge (relative criteria -1) with max_iteration 0 / 10, grid build included; *_one_point: the same with one source point; "
                         "a pass = (t10 - t0) / 10; nearest_point: ngm_nearest_point, grid build included, on the same clouds and with one query that lies on the target; align_mesh/*: host "
                         "clock ending in a synchronise, the target's normals included in both",
               agreement=agreement, times=out_times, derived=derived)
    if a.bench_json and os.path.exists(a.bench_json):
        out["bench_py_parent_and_this_tree_same_box"] = json.load(open(a.bench_json))
    _write(a.out, out)
    print(json.dumps(dict(times=med, derived=derived, agreement=agreement, sclk_mhz=sclk)), flush=True)


if __name__ == "__main__":
    main()
