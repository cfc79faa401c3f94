"""Culling a mesh on the device: the depth rasteriser (ngm_mesh_depth), the fused visibility kernel (ngm_mesh_visibility), the
whole mesh.cull_mesh and mesh.evaluate_raw_mesh, against the reference's own vertex path (_apply_culling_strategy,
mesh_culling.py:193-225: a Python loop over the poses, about ten torch kernels per pose) written in torch on the device.

    python tools/mesh_cull_bench.py [--out profiles/r14_mesh_cull.json] [--reps 5] [--poses 1000] [--skip-large-lib LIB]

Workload: the mesh extract_mesh gives for the room map of tools/mesh_bench.py (200 fields, m1_fourier, 0.02 m) as the estimate,
the room itself with two triangles per wall as the ground truth, `--poses` camera poses inside the room at 600 x 340.
One process; after one warm-up of every item the items are run in turn, `--reps` times.  Device events around one chunk of
16 poses for the two kernels (per pose = / 16) and for the torch vertex path over the same 16 poses and depth maps; host clock
(ending in a synchronise) around the whole cull_mesh of either mesh and the whole evaluate_raw_mesh.  The rasteriser has no counterpart that runs here (the reference renders with pyrender under EGL): its time is
absolute, stated with the shader clock.
--skip-large-lib: a variant library built with -DNGM_CULL_SKIP_LARGE (the wave-shared path draws nothing:
NGM_HIPCC_EXTRA=-DNGM_CULL_SKIP_LARGE python -m neural_graph_mapping_amd.build --out=libngm_cull_skip_large.so); a child process
times the rasteriser with it, and 1 - skip / full is the share of the rasteriser's time spent on large triangles."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, _write  # noqa: E402
from mesh_bench import ROOM, extract, make  # noqa: E402
from mesh_metrics_bench import device_ms, host_ms, shader_clock_under_load, summary  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402
from neural_graph_mapping_amd.renderer import Camera  # noqa: E402

CHUNK, W, H, F = 16, 600, 340, 300.0
DEPTH_TEST = dict(depth_worst_relative_error=1.122e-05, depth_bar=4.488e-05,
                  note="tests/test_gpu_mesh_cull.py: worst |z - z64| / z64 against the fp64 mirror over all its scenes (the floor 5 cm under the "
                       "camera; scenes within 80 degrees of incidence stay below 2.4e-06), and the bar = 4 x worst")


def room_mesh():
    x, y, z = ROOM
    v = torch.tensor([(0, 0, 0), (x, 0, 0), (x, y, 0), (0, y, 0), (0, 0, z), (x, 0, z), (x, y, z), (0, y, z)], dtype=torch.float32)
    f = torch.tensor([(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7), (0, 1, 5), (0, 5, 4), (1, 2, 6), (1, 6, 5), (2, 3, 7), (2, 7, 6), (3, 0, 4), (3, 4, 7)])
    return v.to(DEV), f.to(DEV)


def room_poses(n, seed=14):
    """OpenGL camera-to-world poses: eyes at least 0.5 m from every wall, looking at random points of the room"""
    g = torch.Generator().manual_seed(seed)
    room = torch.tensor(ROOM)
    eye = 0.5 + torch.rand(n, 3, generator=g) * (room - 1.0)
    fwd = torch.nn.functional.normalize(torch.rand(n, 3, generator=g) * room - eye, dim=-1)
    right = torch.nn.functional.normalize(torch.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand(n, 3), dim=-1), dim=-1)
    up = torch.cross(right, fwd, dim=-1)
    c2w = torch.eye(4).repeat(n, 1, 1)
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, up, -fwd, eye
    return c2w.to(DEV)


def torch_vertex_path(points, c2ws, cam, depth, eps=0.03, virt_cam_starts=-1):
    """_apply_culling_strategy with _cull_from_one_pose inlined (mesh_culling.py:143-225), on the device as it stands there: a loop
    over the poses, float accumulators, the projection matrix made per pose"""
    width, height = cam.width, cam.height
    in_frustum_mask = torch.zeros(points.shape[0], device=DEV)
    obs_mask = torch.zeros(points.shape[0], device=DEV)
    fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.5)
    for i in range(c2ws.shape[0]):
        c2w = c2ws[i].clone()
        c2w[:3, 1] *= -1
        c2w[:3, 2] *= -1
        w2c = torch.linalg.inv(c2w)
        camera_space = w2c[:3, :3] @ points.T + w2c[:3, 3][:, None]
        uvz = (torch.tensor([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=torch.float).to(DEV) @ camera_space).T
        pz = uvz[:, 2] + 1e-8
        px = uvz[:, 0] / pz
        py = uvz[:, 1] / pz
        in_frustum = (0 <= px) & (px <= width - 1) & (0 <= py) & (py <= height - 1) & (pz > 0)
        u = torch.clip(px, 0, width - 1).int()
        v = torch.clip(py, 0, height - 1).int()
        obs = in_frustum & (pz < (depth[i][v, u] + eps))
        obs_mask = obs_mask + obs.int()
        if virt_cam_starts < 0 or i < virt_cam_starts:
            in_frustum_mask = in_frustum_mask + in_frustum.int()
    return in_frustum_mask, obs_mask


def depth_only(verts, faces, gt, c2ws, cam, reps):
    """the two rasteriser items alone (the child process of --skip-large-lib runs only this)"""
    items = dict(depth_estimate_chunk=lambda: device_ms(lambda: Mh.render_mesh_depth(verts, faces, c2ws[:CHUNK], cam))[0],
                 depth_ground_truth_chunk=lambda: device_ms(lambda: Mh.render_mesh_depth(gt[0], gt[1], c2ws[:CHUNK], cam), 20)[0])
    times = {k: [] for k in items}
    for fn in items.values():
        fn()
    for _ in range(reps):
        for k, fn in items.items():
            times[k].append(fn())
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--skip-large-lib", default=None)
    ap.add_argument("--depth-only", action="store_true", help="internal: print the rasteriser's times as JSON and exit")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_cull_bench needs the MI355X: there is no CPU fallback to time"
    r = make("m1_fourier")
    verts, faces, _ = extract(r, 0.02, 200, True)
    gt = room_mesh()
    cam = Camera(W, H, F, F, W / 2, H / 2, pixel_center=0.5)
    c2ws = room_poses(a.poses)
    print(json.dumps(dict(stage="workload", vertices=len(verts), faces=len(faces), poses=a.poses)), flush=True)
    if a.depth_only:
        print("DEPTH_ONLY " + json.dumps(depth_only(verts, faces, gt, c2ws, cam, a.reps)), flush=True)
        return
    depth16 = Mh.render_mesh_depth(verts, faces, c2ws[:CHUNK], cam)
    # the fused kernel and the torch loop agree before anything is timed (counts may differ where fp32 rounds differently)
    inf, obs = Mh.mesh_visibility(verts, c2ws[:CHUNK], cam, depth16)
    t_inf, t_obs = torch_vertex_path(verts, c2ws[:CHUNK], cam, depth16)
    agreement = dict(vertices=len(verts), poses=CHUNK, in_frustum_counts_differ=int((inf != t_inf.int()).sum()), observed_counts_differ=int((obs != t_obs.int()).sum()))
    print(json.dumps(dict(stage="agreement", **agreement)), flush=True)

    items = dict(
        visibility_fused_chunk=lambda: device_ms(lambda: Mh.mesh_visibility(verts, c2ws[:CHUNK], cam, depth16))[0],
        visibility_torch_loop_chunk=lambda: device_ms(lambda: torch_vertex_path(verts, c2ws[:CHUNK], cam, depth16))[0],
        cull_mesh_estimate=lambda: host_ms(lambda: Mh.cull_mesh(verts, faces, c2ws, cam, "occlusion"))[0],
        cull_mesh_ground_truth=lambda: host_ms(lambda: Mh.cull_mesh(gt[0], gt[1], c2ws, cam, "occlusion"))[0],
        evaluate_raw_mesh=lambda: host_ms(lambda: Mh.evaluate_raw_mesh((verts, faces), gt, c2ws, cam, "occlusion", "occlusion", a.points))[0])
    times = {k: [] for k in items}
    for k, fn in items.items():
        fn()
        print(json.dumps(dict(stage="warm-up", item=k)), flush=True)
    dtimes = depth_only(verts, faces, gt, c2ws, cam, a.reps)
    for rep in range(a.reps):
        for k, fn in items.items():
            times[k].append(fn())
        print(json.dumps(dict(stage="repeat", n=rep, **{k: round(v[-1], 3) for k, v in times.items()})), flush=True)
    times.update(dtimes)
    sclk = shader_clock_under_load(lambda: Mh.render_mesh_depth(gt[0], gt[1], c2ws[:CHUNK], cam))
    res = {k: summary(v) for k, v in times.items()}
    per_pose = {k.replace("_chunk", "_per_pose"): round(v["median_ms"] / CHUNK, 4) for k, v in res.items() if k.endswith("_chunk")}
    fused_faster_every_repeat = all(f < t for f, t in zip(times["visibility_fused_chunk"], times["visibility_torch_loop_chunk"]))
    culled = Mh.cull_mesh(verts, faces, c2ws, cam, "occlusion")
    large = None
    if a.skip_large_lib:
        env = dict(os.environ, NGM_LIB_PATH=os.path.abspath(a.skip_large_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--depth-only", "--reps", str(a.reps), "--poses", str(a.poses)], env=env,
                           capture_output=True, text=True, timeout=900)
        line = [l for l in p.stdout.splitlines() if l.startswith("DEPTH_ONLY ")]
        if p.returncode == 0 and line:
            skip = {k: statistics.median(v) for k, v in json.loads(line[0][len("DEPTH_ONLY "):]).items()}
            large = {k.replace("_chunk", ""): dict(skip_large_median_ms=round(skip[k], 3), full_median_ms=res[k]["median_ms"],
                                                   share_of_time_in_large_path=round(1 - skip[k] / res[k]["median_ms"], 3)) for k in skip}
        else:
            large = dict(error=(p.stderr or p.stdout)[-400:])
    metrics = Mh.evaluate_raw_mesh((verts, faces), gt, c2ws, cam, "occlusion", "occlusion", a.points)
    out = dict(tool="tools/mesh_cull_bench.py",
               command=f"python tools/mesh_cull_bench.py --out profiles/r14_mesh_cull.json --reps {a.reps} --poses {a.poses}" + (" --skip-large-lib <variant>" if a.skip_large_lib else ""),
               device=torch.cuda.get_device_name(0), sclk_mhz=sclk,
               workload=f"the room map's extracted mesh ({len(verts)} vertices, {len(faces)} faces; tools/mesh_bench.py, m1_fourier, 0.02 m), the room with two "
                        f"triangles per wall (8 vertices, 12 faces), {a.poses} poses inside the room at {W} x {H}, fx = fy = {F}, method occlusion",
               procedure=f"one process, one warm-up of every item, then the items in turn, {a.reps} repeats; *_chunk: ms between device events around {CHUNK} poses "
                         "(20 calls for the ground truth's rasteriser), the torch loop on the same poses and depth maps; cull_mesh_* / evaluate_raw_mesh: host clock "
                         "ending in a synchronise; the rasteriser has no counterpart that runs here (pyrender is absent): its time is absolute",
               times=res, per_pose_ms=per_pose, visibility_fused_faster_than_torch_loop_in_every_repeat=fused_faster_every_repeat,
               visibility_speedup_median=round(res["visibility_torch_loop_chunk"]["median_ms"] / res["visibility_fused_chunk"]["median_ms"], 2),
               agreement=agreement, culled_estimate=dict(vertices=int(culled[0].shape[0]), faces=int(culled[1].shape[0])),
               large_triangle_path=large if large is not None else "not measured in this run (no --skip-large-lib)",
               metrics=metrics, **DEPTH_TEST)
    _write(a.out, out)
    print(json.dumps(dict(times={k: v["median_ms"] for k, v in res.items()}, per_pose_ms=per_pose, fused_faster_every_repeat=fused_faster_every_repeat,
                          large_triangle_path=large, sclk_mhz=sclk, culled=out["culled_estimate"])), flush=True)
    assert math.isfinite(metrics["acc"])


if __name__ == "__main__":
    main()
