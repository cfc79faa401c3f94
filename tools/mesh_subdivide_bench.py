"""Subdividing a mesh to a maximum edge length on the device (mesh.subdivide_to_size: ngm_mesh_subdivide_count / _emit) against
trimesh's loop (subdivide_to_size: split every face that is too long into four by its unique edge midpoints, set the others aside,
repeat) written in torch on the device, fp64 and one torch.unique per round as trimesh works; and mesh.cull_mesh on the
two-triangles-per-wall ground truth with and without max_edge.

    python tools/mesh_subdivide_bench.py [--out profiles/r15_mesh_subdivide.json] [--reps 5] [--poses 1000] [--bench-json FILE]

Meshes: the room of tools/mesh_bench.py with two triangles per wall at max_edge 0.1; the mesh extract_mesh gives for the room map
(m1_fourier, 0.02 m) at 0.1 -- nothing to split: the path that returns the input -- and at 0.01, where most faces split.
One process; after one warm-up of every item the items are run in turn, `--reps` times.  count / emit: ms between device events
around the op; whole: host clock around subdivide_to_size ending in a synchronise (the read-back of the totals included); torch:
host clock around the torch loop.  emit_gb_per_s: the bytes of the emit call's outputs (12 per vertex, 24 + 8 per face) over its
time.  --bench-json merges a file holding bench.py's result lines of the parent commit and of this tree from the same box."""
import argparse
import json
import os
import sys

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


def torch_subdivide_to_size(verts, faces, max_edge, max_iter=10):
    """trimesh.Trimesh.subdivide_to_size on the device as it stands there: float64 copy, per round the edge lengths of every
    face, the short faces set aside with their vertices (unique), the long ones split by one midpoint per unique edge"""
    cur_v, cur_f = verts.double(), faces
    done_v, done_f = [], []
    for it in range(max_iter + 1):
        c = cur_v[cur_f[:, [0, 1, 2, 0]]]
        too_long = (((c[:, 1:] - c[:, :-1]) ** 2).sum(2) ** 0.5 > max_edge).any(1)
        unique, inverse = torch.unique(cur_f[~too_long].reshape(-1), return_inverse=True)
        done_v.append(cur_v[unique])
        done_f.append(inverse.reshape(-1, 3))
        if not bool(too_long.any()):
            break
        if it == max_iter:
            raise ValueError("max_iter exceeded")
        f = cur_f[too_long]
        edges = torch.sort(f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), dim=1).values
        unique, inverse = torch.unique(edges[:, 0] * len(cur_v) + edges[:, 1], return_inverse=True)     # a row as one key
        mid = 0.5 * (cur_v[unique // len(cur_v)] + cur_v[unique % len(cur_v)])
        m = inverse.reshape(-1, 3) + len(cur_v)
        cur_f = torch.stack([f[:, 0], m[:, 0], m[:, 2], m[:, 0], f[:, 1], m[:, 1], m[:, 2], m[:, 1], f[:, 2], m[:, 0], m[:, 1], m[:, 2]], 1).reshape(-1, 3)
        cur_v = torch.cat([cur_v, mid])
    offsets = [0]
    for v in done_v[:-1]:
        offsets.append(offsets[-1] + len(v))
    return torch.cat(done_v), torch.cat([f + o for f, o in zip(done_f, offsets)])


def area(verts, faces):
    c = verts.double()[faces]
    return float(0.5 * torch.linalg.norm(torch.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0], dim=-1), dim=-1).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--bench-json", default=None, help="bench.py's result lines of the parent commit and this tree, same box")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mesh_subdivide_bench needs the MI355X: there is no CPU fallback to time"
    r = make("m1_fourier")
    verts, faces, _ = extract(r, 0.02, 200, True)
    gt = room_mesh()
    cases = dict(ground_truth_at_0p1=(gt[0], gt[1], 0.1), extracted_at_0p1=(verts, faces, 0.1), extracted_at_0p01=(verts, faces, 0.01))
    print(json.dumps(dict(stage="workload", vertices=len(verts), faces=len(faces))), flush=True)

    items, shapes, emits = {}, {}, {}
    for name, (v, f, max_edge) in cases.items():
        totals, ws = torch.ops.ngm355.mesh_subdivide_count(v, f, max_edge, 10)
        new_vertices, out_faces, max_level = (int(t) for t in totals.tolist())
        ours = Mh.subdivide_to_size(v, f, max_edge)
        theirs = torch_subdivide_to_size(v, f, max_edge)
        shapes[name] = dict(max_edge=max_edge, vertices_in=len(v), faces_in=len(f), new_vertices=new_vertices, faces_out=out_faces, max_level=max_level,
                            vertices_out=len(ours[0]), torch_loop_vertices_out=len(theirs[0]), torch_loop_faces_out=len(theirs[1]),
                            area_in=area(v, f), area_out=area(*ours), torch_loop_area_out=area(*theirs),
                            returns_the_input_tensors=ours[0] is v and ours[1] is f,
                            emit_output_bytes=12 * (len(v) + new_vertices) + 32 * out_faces if new_vertices else 0)
        assert out_faces == len(theirs[1]) == len(ours[1]), (name, out_faces, len(theirs[1]))
        print(json.dumps(dict(stage="agreement", item=name, **shapes[name])), flush=True)
        del ours, theirs
        items[name + "/count"] = (lambda v=v, f=f, e=max_edge: device_ms(lambda: torch.ops.ngm355.mesh_subdivide_count(v, f, e, 10))[0])
        if new_vertices:
            emits[name] = ws
            items[name + "/emit"] = (lambda v=v, f=f, ws=ws, n=new_vertices, t=out_faces:
                                     device_ms(lambda: torch.ops.ngm355.mesh_subdivide_emit(v, f, None, ws, n, t))[0])
        items[name + "/whole"] = (lambda v=v, f=f, e=max_edge: host_ms(lambda: Mh.subdivide_to_size(v, f, e))[0])
        items[name + "/torch_loop"] = (lambda v=v, f=f, e=max_edge: host_ms(lambda: torch_subdivide_to_size(v, f, e))[0])

    cam = Camera(W, H, F, F, W / 2, H / 2, pixel_center=0.5)
    c2ws = room_poses(a.poses)
    items["cull_mesh_ground_truth"] = lambda: host_ms(lambda: Mh.cull_mesh(gt[0], gt[1], c2ws, cam, "occlusion"))[0]
    items["cull_mesh_ground_truth_max_edge_0p1"] = lambda: host_ms(lambda: Mh.cull_mesh(gt[0], gt[1], c2ws, cam, "occlusion", max_edge=0.1))[0]

    times = {k: [] for k in items}
    for k, fn in items.items():
        fn()
        print(json.dumps(dict(stage="warm-up", item=k)), flush=True)
    for rep in range(a.reps):
        for k, fn in items.items():
            times[k].append(fn())
        print(json.dumps(dict(stage="repeat", n=rep, **{k: round(v[-1], 3) for k, v in times.items()})), flush=True)
    sclk = shader_clock_under_load(lambda: torch.ops.ngm355.mesh_subdivide_count(verts, faces, 0.01, 10), n=100)
    res = {k: summary(v) for k, v in times.items()}
    for name, s in shapes.items():
        if name in emits:
            s["emit_gb_per_s"] = round(s["emit_output_bytes"] / (res[name + "/emit"]["median_ms"] * 1e-3) / 1e9, 1)
        s["kernel_path_below_torch_loop_in_every_repeat"] = all(o < t for o, t in zip(times[name + "/whole"], times[name + "/torch_loop"]))
        s["speedup_median"] = round(res[name + "/torch_loop"]["median_ms"] / res[name + "/whole"]["median_ms"], 2)
    plain = Mh.cull_mesh(gt[0], gt[1], c2ws, cam, "occlusion")
    fine = Mh.cull_mesh(gt[0], gt[1], c2ws, cam, "occlusion", max_edge=0.1)
    culled = dict(without_max_edge=dict(vertices=len(plain[0]), faces=len(plain[1]), area=area(*plain)),
                  max_edge_0p1=dict(vertices=len(fine[0]), faces=len(fine[1]), area=area(*fine)), area_of_the_room=area(*gt))
    out = dict(tool="tools/mesh_subdivide_bench.py",
               command=f"python tools/mesh_subdivide_bench.py --out profiles/r15_mesh_subdivide.json --reps {a.reps} --poses {a.poses}"
                       + (" --bench-json <bench.py lines>" if a.bench_json else ""),
               device=torch.cuda.get_device_name(0), torch=torch.__version__, sclk_mhz=sclk,
               workload=f"the room with two triangles per wall (8 vertices, 12 faces) at max_edge 0.1; the room map's extracted mesh ({len(verts)} vertices, "
                        f"{len(faces)} faces; tools/mesh_bench.py, m1_fourier, 0.02 m) at 0.1 (nothing to split) and at 0.01; cull_mesh: {a.poses} poses inside "
                        f"the room at {W} x {H}, fx = fy = {F}, method occlusion",
               procedure=f"one process, one warm-up of every item, then the items in turn, {a.reps} repeats; */count, */emit: ms between device events around the "
                         "op (emit: copy of the originals, new vertices, faces and parents; no attributes); */whole: host clock around subdivide_to_size ending "
                         "in a synchronise, the read-back of the three totals included; */torch_loop: host clock around trimesh's loop in torch on the device "
                         "(fp64, torch.unique per round; an edge is one int64 key); cull_mesh_*: host clock ending in a synchronise",
               meshes=shapes, times=res, cull_mesh_ground_truth=culled)
    if a.bench_json and os.path.exists(a.bench_json):
        out["bench_py_parent_and_this_tree_same_box"] = json.load(open(a.bench_json))
    _write(a.out, out)
    print(json.dumps(dict(times={k: v["median_ms"] for k, v in res.items()}, meshes=shapes, culled=culled, sclk_mhz=sclk)), flush=True)


if __name__ == "__main__":
    main()
