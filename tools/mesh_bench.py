"""Mesh extraction: extract_mesh(fused=True) -- one ngm_grid_eval_knn call per grid block, blocks no field can reach skipped --
against extract_mesh(fused=False), the staged path (cartesian_prod -> field_eval_knn in block_size chunks -> slice / reshape /
negate) over every block.

    python tools/mesh_bench.py [--out profiles/r11_mesh_extract.json] [--reps 5] [--networks hash,m1_fourier]
                               [--resolutions 0.02,default] [--block 200] [--trace] [--parent-tree DIR]
                               [--merge KEY=FILE ...] [--readme profiles/README.md]
    python tools/mesh_bench.py --kernel-resources PARENT_TREE

Map: 200 fields of the shipped radius (1 m) on the nodes of the reference's cover grid (spacing 2 r / sqrt 3, rm.py:299)
nearest to the walls and the floor of an 8 x 6 x 3 m room -- the room's own shell has only ~120 such nodes, so the nodes one
spacing outside the walls and below the floor fill up to 200 (as a map grown from depth images that see through doors
would); seeded, random weights (timing needs no trained map).  Resolutions: 0.02 m (the reference's final mesh) and the
default derived from the sampling (2 * truncation_distance / num_samples_depth_guided = 0.0125 m at the shipped config).
One process, the two paths alternated after a warm-up of each; host clock around a final device synchronise.  Reported per
(network, resolution): median / min / max of both paths, `stats`, torch.cuda.max_memory_allocated of each path, torch.equal
of the two meshes, and -- from one instrumented extraction per path, device events at the stage boundaries -- the split
into volume evaluation, marching cubes and vertex colours.  --trace: per-kernel rows from child runs of their own under
`rocprofv3 --kernel-trace --stats` (one per path).  --parent-tree DIR (a checkout of the parent commit with its library
built): the image path (tools/eval_bench.py) and bench.py on that tree and on this one, alternating child processes of the same
call.  --kernel-resources PARENT_TREE (no GPU; a mode of its own): the compiler's register / scratch / occupancy report of
csrc/ngm_knn.hip for both trees -> profiles/r11_mesh_kernel_resources.{json,md}; --merge kernel_resources=FILE puts its
summary into the result.  --readme profiles/README.md: the result's row there is written by this tool."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from device_iteration_bench import DEV, NETWORKS, _write, renderer  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402

NF, RADIUS, ROOM = 200, 1.0, (8.0, 6.0, 3.0)


def room_map():
    """(pos (200, 3), quat (200, 4)) on the device: see the module docstring"""
    g = torch.Generator().manual_seed(0)
    s = 2 * RADIUS / 3 ** 0.5
    ax = [torch.arange(-1, int(e / s) + 2) * s for e in ROOM]
    nodes = torch.cartesian_prod(*ax)
    nodes = nodes[nodes[:, 2] < ROOM[2]]                                  # no layer above the ceiling: walls and floor
    x, y, z = nodes.unbind(-1)
    d_wall = torch.minimum(torch.minimum(x.abs(), (x - ROOM[0]).abs()), torch.minimum(y.abs(), (y - ROOM[1]).abs()))
    d = torch.minimum(d_wall, z.abs()) + 1e-3 * torch.rand(len(nodes), generator=g)      # distance to the nearest wall / floor
    pos = nodes[d.argsort()[:NF]] + 1e-3 * torch.randn(NF, 3, generator=g)
    quat = torch.nn.functional.normalize(torch.randn(NF, 4, generator=g), dim=-1)
    return pos.to(DEV), quat.to(DEV)


def make(network):
    pos, quat = room_map()
    r = renderer(network, pos, quat)                                     # 200 fields, shipped config, radius 1
    # random weights as the constructor draws them, plus a per-field offset of the geometry output in [-0.5, 0.5]: about half
    # the fields are "inside" (nrgbd: geometry < 0), so the level set is a 2-D surface of roughly a room's area -- a noisy
    # geometry would cross the level in every cell and time marching cubes and the colours, which both paths share
    g = torch.Generator(device=DEV).manual_seed(1)
    p = r._model.all_fields_params
    with torch.no_grad():
        p[f"_linears.{NETWORKS[network][2]}.bias"][:, 3] += torch.rand(NF, device=DEV, generator=g) - 0.5
        if "_encoding.lattice_values" in p:                              # (the hash table starts at 1e-5)
            p["_encoding.lattice_values"].add_(0.05 * torch.randn(p["_encoding.lattice_values"].shape, device=DEV, generator=g))
    r._model.refresh_lp()
    return r


def extract(r, res, block, fused, stats=None):
    return r.extract_mesh(None, resolution=res, block=block, fused=fused, stats=stats)


def timed(r, res, block, fused):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = extract(r, res, block, fused)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stage_split(r, res, block, fused):
    """one instrumented extraction: device events at marching cubes' and the colour evaluation's entry and exit; the time
    before a marching-cubes call that is neither is the block's volume evaluation (staged: cartesian_prod and the slice /
    reshape / negate passes included)"""
    marks = []

    def mark(label):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        marks.append((label, e))

    real_mc, real_knn = Mh.marching_cubes, ops.field_eval_knn

    def mc(vol, iso):
        mark("mc_in")
        out = real_mc(vol, iso)
        mark("mc_out")
        return out

    def knn(*a, **kw):
        colour = (len(a) > 9 and a[9] is not None) or kw.get("mask_radius") is not None
        if colour:
            mark("col_in")
        out = real_knn(*a, **kw)
        if colour:
            mark("col_out")
        return out

    Mh.marching_cubes, ops.field_eval_knn = mc, knn
    try:
        mark("start")
        extract(r, res, block, fused)
        mark("end")
        torch.cuda.synchronize()
    finally:
        Mh.marching_cubes, ops.field_eval_knn = real_mc, real_knn
    ms = dict(volume=0.0, marching_cubes=0.0, colours=0.0, other=0.0)
    for (la, ea), (lb, eb) in zip(marks, marks[1:]):
        key = ("marching_cubes" if la == "mc_in" else "colours" if la == "col_in" or (la == "mc_out" and lb == "col_in")
               else "other" if lb == "end" else "volume")
        ms[key] += ea.elapsed_time(eb)
    return {k: round(v, 3) for k, v in ms.items()}


def summary(v):
    return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3), repeats=len(v))


def measure(network, res, block, reps):
    r = make(network)
    res_val = None if res == "default" else float(res)
    out = dict(network=network, resolution=res, block=block, fields=NF)
    meshes, times, mem, st = {}, dict(fused=[], staged=[]), {}, {}
    for name, fused in (("fused", True), ("staged", False)):              # warm-up: every shape of the timed window, and the check
        torch.cuda.reset_peak_memory_stats()
        st[name] = {}
        meshes[name] = extract(r, res_val, block, fused, st[name])
        torch.cuda.synchronize()
        mem[name] = int(torch.cuda.max_memory_allocated())
    a, b = meshes["fused"], meshes["staged"]
    out["meshes_equal"] = bool(a is not None and b is not None and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)))
    out["vertices"], out["faces"] = (int(len(a[0])), int(len(a[1]))) if a is not None else (0, 0)
    del meshes, a, b
    for _ in range(reps):                                                  # alternating, same process, same clocks
        for name, fused in (("fused", True), ("staged", False)):
            times[name].append(timed(r, res_val, block, fused)[0])
    for name, fused in (("fused", True), ("staged", False)):
        out[name] = dict(**summary(times[name]), all_ms=[round(t, 3) for t in times[name]], stats=st[name],
                         max_memory_allocated_bytes=mem[name], split_ms=stage_split(r, res_val, block, fused))
    lo_s, hi_f = min(times["staged"]), max(times["fused"])
    out["fused_faster_beyond_the_spread"] = bool(hi_f < lo_s)             # every fused repeat below every staged repeat
    out["speedup_median"] = round(out["staged"]["median_ms"] / out["fused"]["median_ms"], 3)
    return out


def trace_child(network, res, block, path):
    r = make(network)
    res_val = None if res == "default" else float(res)
    extract(r, res_val, block, path == "fused")
    torch.cuda.synchronize()


def _short(name):
    """a kernel's name without its argument list (the last top-level parenthesis), at most 110 characters"""
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0 and name[i] == "(" and name.endswith(")"):
            return name[:i][:110]
        if depth == 0 and not name.endswith(")"):
            break
    return name[:110]


def kernel_rows(network, res, block, path):
    d = tempfile.mkdtemp(prefix="mesh_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
           sys.executable, os.path.abspath(__file__), "--trace-child", network, str(res), str(block), path]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if p.returncode != 0 or not files:
        raise RuntimeError(f"rocprofv3 exit {p.returncode}: {p.stderr[-400:]}")
    rows = []
    for row in csv.DictReader(open(files[0])):
        rows.append(dict(kernel=_short(row["Name"]), calls=int(row["Calls"]), total_ms=round(float(row["TotalDurationNs"]) / 1e6, 3),
                         avg_us=round(float(row["AverageNs"]) / 1e3, 2), percent=round(float(row["Percentage"]), 2)))
    return sorted(rows, key=lambda x: -x["total_ms"])[:14]


def parent_vs_new(parent_tree, eval_reps, bench_pairs):
    """the paths this change must not move, on the parent commit's tree (a checkout with its own library built) and on this
    one, as alternating child processes in this call: tools/eval_bench.py (the image path, 640 samples per ray) and
    bench.py --steps 200 --warmup 20 of both variants in mirrored pairs.  A child that fails ends the comparison."""
    trees = dict(parent=os.path.abspath(parent_tree), new=ROOT)

    def child(tree, argv, env=None):
        p = subprocess.run([sys.executable] + argv, cwd=tree, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise RuntimeError(f"{argv[0]} in {tree}: exit {p.returncode}: {p.stderr[-300:]}")
        return json.loads(p.stdout.strip().splitlines()[-1])

    def spread(vals):
        return dict(all=[round(v, 5) for v in vals], median=round(statistics.median(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))

    img = dict(command="tools/eval_bench.py with NGM_EVAL_S=640 in a checkout of the parent commit and in this tree, alternating "
                       "processes in one call; ms per 640 x 480 x 640 image", repeats=eval_reps)
    ev = dict(parent=dict(S640=[], S640_hash=[]), new=dict(S640=[], S640_hash=[]))
    for i in range(eval_reps):
        for side in (("parent", "new") if i % 2 == 0 else ("new", "parent")):
            js = child(trees[side], [os.path.join(trees[side], "tools", "eval_bench.py")], dict(NGM_EVAL_S="640"))
            for k in ev[side]:
                ev[side][k].append(js[k]["ms_per_image"])
    for k in ("S640", "S640_hash"):
        pv, nv = ev["parent"][k], ev["new"][k]
        img[k] = dict(parent=spread(pv), new=spread(nv), new_within_parent_spread=bool(max(nv) <= max(pv)))
    trn = dict(command="bench.py --gpus 1 --steps 200 --warmup 20 --variant V in a checkout of the parent commit and in this "
                       "tree, mirrored pairs of alternating processes in one call; ms per step", pairs=bench_pairs)
    for v in ("fourier", "hash"):
        vals = dict(parent=[], new=[])
        for i in range(bench_pairs):
            for side in (("new", "parent") if i % 2 == 0 else ("parent", "new")):
                js = child(trees[side], [os.path.join(trees[side], "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20", "--variant", v])
                vals[side].append(js["ms_per_step"])
        trn[v] = dict(parent=spread(vals["parent"]), new=spread(vals["new"]),
                      new_median_within_parent_spread=bool(statistics.median(vals["new"]) <= max(vals["parent"])))
    return img, trn


# ---- the compiler's per-kernel report of csrc/ngm_knn.hip, parent commit against this one (no GPU) -------------------------
RES_KEYS = ("VGPRs", "AGPRs", "ScratchSize", "Occupancy")
RES_CMD = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c"]


def _resources_of(tree):
    import re
    import shutil
    from neural_graph_mapping_amd import build as B
    obj = tempfile.mktemp(suffix=".o")
    p = subprocess.run([B._hipcc()] + RES_CMD + [os.path.join(tree, "neural_graph_mapping_amd", "csrc", "ngm_knn.hip"), "-o", obj],
                       capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError(f"hipcc failed in {tree}: {p.stderr[-600:]}")
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    names, out, cur = [], {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            names.append(cur)
            out[cur] = {}
            continue
        m = re.search(r"remark: .*?\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1).split(" ")[0]] = int(m.group(2))
    if filt:
        nice = subprocess.run([filt] + names, capture_output=True, text=True).stdout.splitlines()
        out = {re.sub(r"^void ", "", n).replace("(KnnArgs)", ""): out[k] for k, n in zip(names, nice)}
    return out


def kernel_resources(parent_tree, json_path, md_path):
    """Every kernel instance of ngm_knn.hip in both trees.  An instance of this tree whose last template argument is the point
    source 0 (points from memory / drawn on rays) is the parent's instance of the same name without that argument."""
    import concurrent.futures
    with concurrent.futures.ThreadPoolExecutor(2) as ex:
        fa, fb = ex.submit(_resources_of, os.path.abspath(parent_tree)), ex.submit(_resources_of, ROOT)
        a, b = fa.result(), fb.result()
    same = lambda k: k[:-4] + ">" if k.startswith(("k_knn_assign<", "k_knn_eval<")) and k.endswith(", 0>") else k
    b = {same(k): v for k, v in b.items()}
    changed = [k for k in a if k not in b or any(a[k].get(x) != b[k].get(x) for x in RES_KEYS)]
    res = dict(command="hipcc " + " ".join(RES_CMD) + " csrc/ngm_knn.hip, parent commit and this one",
               columns=list(RES_KEYS), parent_instances=len(a), changed=changed, new_instances=len([k for k in b if k not in a]),
               parent=a, new=b)
    _write(json_path, res)
    fmt = lambda v: " / ".join(str(v.get(x)) for x in RES_KEYS)
    md = ["# Lattice point source of the kNN evaluation: kernel resources, parent commit against this one\n",
          "`" + res["command"] + "` (written by `python tools/mesh_bench.py --kernel-resources PARENT_TREE`).",
          "Columns: VGPRs / AGPRs / scratch bytes per lane / occupancy in waves per SIMD.\n",
          f"{len(a)} kernels in the parent's object, {len(changed)} of them with a changed figure; {res['new_instances']} new instances.\n",
          "## The parent's instances\n", "| kernel | parent | this commit |", "|---|---|---|"]
    md += [f"| `{k}` | {fmt(a[k])} | {fmt(b.get(k, {}))} |" for k in a]
    md += ["\n## The new instances (point source 2: the lattice)\n", "| kernel | this commit | its point-source-0 twin |", "|---|---|---|"]
    for k in b:
        if k not in a:
            twin = k[:-4] + ">" if k.endswith(", 2>") else None
            md.append(f"| `{k}` | {fmt(b[k])} | {fmt(b[twin]) if twin in b else '-'} |")
    with open(md_path, "w") as fh:
        fh.write("\n".join(md) + "\n")
    print(json.dumps(dict(parent_instances=len(a), changed=changed, new_instances=res["new_instances"])))


def readme_row(out):
    """the row of profiles/README.md, from the result itself"""
    run = {(r["network"], r["resolution"]): r for r in out["runs"]}
    gb = lambda r, p: f"{r[p]['max_memory_allocated_bytes'] / 1e9:.2f}"
    t = lambda r, p: f"{r[p]['median_ms']:.1f} ({r[p]['min_ms']:.1f}-{r[p]['max_ms']:.1f})"
    parts = []
    for (net, res), r in run.items():
        parts.append(f"{net} at {res if res != 'default' else 'the default 0.0125'} m: fused {t(r, 'fused')} against staged {t(r, 'staged')} ms, "
                     f"volume stage {r['fused']['split_ms']['volume']:.1f} against {r['staged']['split_ms']['volume']:.1f} ms, marching cubes "
                     f"{r['fused']['split_ms']['marching_cubes']:.1f}, colours {r['fused']['split_ms']['colours']:.1f}, "
                     f"{r['fused']['stats']['blocks_skipped']} of {r['fused']['stats']['blocks_total']} blocks skipped, peak memory "
                     f"{gb(r, 'fused')} against {gb(r, 'staged')} GB (10^9 bytes), {r['vertices']} vertices, meshes "
                     f"{'torch.equal' if r['meshes_equal'] else 'DIFFER'}")
    notes = "; ".join(parts)
    notes += ("; every fused repeat below every staged one: `fused=True` is the default" if out["default_fused"]
              else "; NOT every fused repeat below every staged one: the default is `fused=False`")
    kt = out.get("kernel_trace", {}).get("fused")
    if isinstance(kt, list):
        notes += "; trace of one fused extraction: " + ", ".join(f"`{k['kernel']}` {k['avg_us']:.0f} us x {k['calls']}" for k in kt[:4])
    img, trn = out.get("image_path_parent_vs_new"), out.get("train_bench_parent_vs_new")
    if img:
        notes += "; image path " + ", ".join(f"{k}: {img[k]['new']['min']}-{img[k]['new']['max']} ms against the parent's {img[k]['parent']['min']}-{img[k]['parent']['max']}" for k in ("S640", "S640_hash"))
    if trn:
        notes += "; `bench.py` medians " + ", ".join(f"{v}: {trn[v]['new']['median']} against {trn[v]['parent']['median']} ms" for v in ("fourier", "hash"))
    kr = out.get("kernel_resources")
    if isinstance(kr, dict) and "parent_instances" in kr:
        notes += (f"; compiler report: {kr['parent_instances']} kernel instances of the parent's `ngm_knn.hip`, {len(kr['changed'])} with a changed "
                  f"register / scratch / occupancy figure, {kr['new_instances']} new")
    cmd = out["command"] + " on one MI355X in one call (" + out["procedure"] + ")"
    return f"| `r11_mesh_extract.json`, `r11_mesh_kernel_resources.md` | `{cmd}` | {out['map']}, {out['runs'][0]['block']}-cell blocks: {notes} |"


def upsert_readme(path, row):
    lines = open(path).read().rstrip("\n").split("\n")
    lines = [l for l in lines if not l.startswith("| `r11_mesh_extract.json`")] + [row]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--networks", default="hash,m1_fourier")
    ap.add_argument("--resolutions", default="0.02,default")
    ap.add_argument("--block", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built: image path and bench.py on both")
    ap.add_argument("--merge", nargs="*", default=[], metavar="KEY=FILE", help="JSON files copied into the result under KEY")
    ap.add_argument("--readme", default=None, help="profiles/README.md: its r11_mesh_extract row is written from the result")
    ap.add_argument("--kernel-resources", default=None, metavar="PARENT_TREE",
                    help="no GPU: compile csrc/ngm_knn.hip of both trees with the resource report, write --resources-json / --resources-md, exit")
    ap.add_argument("--resources-json", default=os.path.join(ROOT, "profiles", "r11_mesh_kernel_resources.json"))
    ap.add_argument("--resources-md", default=os.path.join(ROOT, "profiles", "r11_mesh_kernel_resources.md"))
    ap.add_argument("--from-result", default=None, metavar="JSON", help="no GPU: write the --readme row from an existing result, exit")
    ap.add_argument("--trace-child", nargs=4, default=None)
    a = ap.parse_args()
    if a.from_result:
        return upsert_readme(a.readme, readme_row(json.load(open(a.from_result))))
    if a.trace_child:
        return trace_child(a.trace_child[0], a.trace_child[1], int(a.trace_child[2]), a.trace_child[3])
    if a.kernel_resources:
        return kernel_resources(a.kernel_resources, a.resources_json, a.resources_md)
    assert torch.cuda.is_available(), "mesh_bench needs the MI355X: there is no CPU fallback to time"
    assert a.reps >= 5, "at least five repeats per path"
    # the command as a reader would repeat it (the result and the parent's checkout wherever they lie)
    cmd = (f"python tools/mesh_bench.py --out profiles/r11_mesh_extract.json --reps {a.reps} --networks {a.networks} --resolutions "
           f"{a.resolutions} --block {a.block}" + (" --trace" if a.trace else "") + (" --parent-tree PARENT_TREE" if a.parent_tree else "")
           + "".join(f" --merge {m.partition('=')[0]}=profiles/{os.path.basename(m.partition('=')[2])}" for m in a.merge)
           + " --readme profiles/README.md")
    out = dict(tool="tools/mesh_bench.py", command=cmd, device=torch.cuda.get_device_name(0),
               map=f"{NF} fields, radius {RADIUS} m, cover-grid nodes nearest to the walls and floor of an {ROOM[0]:g} x {ROOM[1]:g} x {ROOM[2]:g} m room",
               procedure=f"fused / staged alternated in one process, {a.reps} repeats each after one warm-up of each, host clock "
                         "around a final device synchronise; split: device events at the stage boundaries of one more extraction",
               runs=[])
    for net in a.networks.split(","):
        assert net in NETWORKS, net
        for res in a.resolutions.split(","):
            out["runs"].append(measure(net, res, a.block, a.reps))
            print(json.dumps({k: v for k, v in out["runs"][-1].items() if k not in ("fused", "staged")}), flush=True)
            _write(a.out, out)
    out["default_fused"] = bool(all(r["fused_faster_beyond_the_spread"] and r["meshes_equal"] for r in out["runs"]))
    stop = False
    if a.trace:
        net, res = a.networks.split(",")[0], a.resolutions.split(",")[0]
        out["kernel_trace"] = dict(command="rocprofv3 --kernel-trace --stats --output-format csv -- python tools/mesh_bench.py "
                                           "--trace-child NETWORK RESOLUTION BLOCK PATH (one extraction, set-up included)",
                                   network=net, resolution=res)
        for path in ("fused", "staged"):
            try:
                out["kernel_trace"][path] = kernel_rows(net, res, a.block, path)
            except Exception as e:      # a child failed or ran into its limit: record it and start nothing more on the card
                out["kernel_trace"][path] = dict(error=f"{type(e).__name__}: {e}")
                stop = True
                break
    if a.parent_tree and not stop:
        torch.cuda.empty_cache()
        try:
            out["image_path_parent_vs_new"], out["train_bench_parent_vs_new"] = parent_vs_new(a.parent_tree, 8, 6)
        except Exception as e:          # as above: nothing more is started
            out["parent_vs_new_error"] = f"{type(e).__name__}: {e}"
    for item in a.merge:
        key, _, f = item.partition("=")
        try:
            js = json.load(open(f))
            out[key] = {k: v for k, v in js.items() if k not in ("parent", "new")} if key == "kernel_resources" else js
        except Exception as e:
            out[key] = dict(error=f"{type(e).__name__}: {e}")
    _write(a.out, out)
    if a.readme:
        upsert_readme(a.readme, readme_row(out))
    print(json.dumps(dict(default_fused=out["default_fused"], runs=len(out["runs"]))))


if __name__ == "__main__":
    main()
