"""Mesh extraction: dense-grid field evaluation -> marching cubes -> vertex colours -> PLY.

Host-side mirror of ``NeuralGraphMap._extract_mesh`` (run_mapping.py:2186-2384).  The grid is filled by the
kNN-blended evaluation kernels (``ops.field_eval_knn``), the iso-surface is extracted by the HIP marching-cubes
kernels (``ngm_marching_cubes_*``; the reference calls the un-vendored ``pytorch3d.ops.marching_cubes``), the file
is the binary little-endian PLY layout ``pytorch3d.io.save_ply`` writes for (verts, faces, verts_colors).
No CPU fallback: device tensors in, device tensors out.
"""
import ctypes as C
import itertools
import os
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _capi as K
from . import ops


@torch.library.custom_op("ngm355::marching_cubes", mutates_args=(), device_types="cuda")
def _marching_cubes_op(volume: torch.Tensor, isolevel: float) -> List[torch.Tensor]:
    """[verts (V,3) fp32 grid-index coordinates, faces (T,3) int64]; data-dependent sizes (no fake kernel)"""
    nx, ny, nz = volume.shape
    L = K.lib()
    wsb = L.ngm_marching_cubes_workspace(nx, ny, nz)
    if wsb < 0:
        raise ValueError(f"marching_cubes: grid {nx}x{ny}x{nz} not supported (every side >= 2, 3*nx*ny*nz < 2^31)")
    dev = volume.device
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    st = ops._stream()
    K.check(L.ngm_marching_cubes_count(volume.data_ptr(), nx, ny, nz, float(isolevel), counts.data_ptr(), ws.data_ptr(), wsb,
                                       st), "ngm_marching_cubes_count")
    nv, nf = (int(v) for v in counts.tolist())                  # the only host sync: output sizes
    verts = torch.empty(nv, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(nf, 3, device=dev, dtype=torch.int64)
    if nv or nf:
        K.check(L.ngm_marching_cubes_emit(volume.data_ptr(), nx, ny, nz, float(isolevel), verts.data_ptr(), nv,
                                          faces.data_ptr(), nf, ws.data_ptr(), wsb, st), "ngm_marching_cubes_emit")
    return [verts, faces]


def marching_cubes(volume: torch.Tensor, isolevel: float):
    """volume (nx, ny, nz) fp32 on the GPU, inside = value > isolevel -> (verts (V,3) fp32 in grid-index
    coordinates (x, y, z), faces (T,3) int64).  Deterministic order, one vertex per crossed grid edge.
    Dispatches through torch.ops.ngm355.marching_cubes."""
    ops._require_gpu(volume)
    if volume.dim() != 3 or volume.dtype != torch.float32:
        raise ValueError("marching_cubes expects a (nx, ny, nz) float32 volume")
    verts, faces = torch.ops.ngm355.marching_cubes(volume.contiguous(), float(isolevel))
    return verts, faces


def save_ply(path_or_file, verts: torch.Tensor, faces: torch.Tensor, verts_colors: Optional[torch.Tensor] = None) -> None:
    """Binary little-endian PLY as pytorch3d.io.save_ply(f, verts, faces, verts_colors, ascii=False,
    colors_as_uint8=False) lays it out (the call of rm.py:2375-2384): float x y z [red green blue] per vertex,
    `list uchar int vertex_index` per face (pytorch3d's header spelling, as far as its public documentation shows; the
    reader below accepts either -- a file is data-identical whichever name the list carries)."""
    v = verts.detach().cpu().numpy().astype("<f4")
    f = faces.detach().cpu().numpy().astype("<i4")
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
              "property float z"]
    if verts_colors is not None:
        c = verts_colors.detach().cpu().numpy().astype("<f4")
        header += ["property float red", "property float green", "property float blue"]
        v = np.concatenate([v, c], 1)
    header += [f"element face {len(f)}", "property list uchar int vertex_index", "end_header"]
    rec = np.empty(len(f), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    own = isinstance(path_or_file, (str, os.PathLike))
    fp = open(path_or_file, "wb") if own else path_or_file
    try:
        fp.write(("\n".join(header) + "\n").encode("ascii"))
        fp.write(np.ascontiguousarray(v).tobytes())
        fp.write(rec.tobytes())
    finally:
        if own:
            fp.close()


def load_ply(path):
    """Reader for the files save_ply writes (tests / round trips): (verts (V,3), faces (T,3), colors (V,3) | None)."""
    with open(path, "rb") as fp:
        props, nv, nf = [], 0, 0
        while True:
            line = fp.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                nv = int(line.split()[-1])
            elif line.startswith("element face"):
                nf = int(line.split()[-1])
            elif line.startswith("property float"):
                props.append(line.split()[-1])
            elif line == "end_header":
                break
        v = np.frombuffer(fp.read(4 * len(props) * nv), dtype="<f4").reshape(nv, len(props))
        rec = np.frombuffer(fp.read(13 * nf), dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    cols = torch.from_numpy(v[:, 3:6].copy()) if len(props) >= 6 else None
    return torch.from_numpy(v[:, :3].copy()), torch.from_numpy(rec["idx"].astype(np.int64)), cols


def _matrix_to_quaternion(R: torch.Tensor) -> torch.Tensor:
    """real-first unit quaternion of a rotation matrix (the sign is irrelevant for rotating points)"""
    m = R.double()
    t = m.trace()
    if t > 0:
        s = torch.sqrt(t + 1.0) * 2
        q = torch.stack([0.25 * s, (m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s])
    else:
        i = int(torch.argmax(torch.diagonal(m)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = torch.sqrt(1.0 + m[i, i] - m[j, j] - m[k, k]) * 2
        q = torch.zeros(4, dtype=torch.float64)
        q[0] = (m[k, j] - m[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (m[j, i] + m[i, j]) / s
        q[1 + k] = (m[k, i] + m[i, k]) / s
    return (q / q.norm()).float()


def _quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def grid_axes(pos: torch.Tensor, field_radius: float, resolution: float):
    """rm.py:2222-2231: bounding box of the field centres +- 2 r, three torch.arange axes of spacing `resolution`"""
    lo = pos.min(0)[0] - 2 * field_radius
    hi = pos.max(0)[0] + 2 * field_radius
    return [torch.arange(float(lo[i]), float(hi[i]), step=resolution, device=pos.device) for i in range(3)]


def grid_to_world(v: torch.Tensor, bx: torch.Tensor, by: torch.Tensor, bz: torch.Tensor) -> torch.Tensor:
    """Marching-cubes vertices in grid-index coordinates (ix, iy, iz) of one block -> world.  The reference maps
    pytorch3d's local coordinates l = 2 i / (n - 1) - 1 back with (0.5 l + 0.5) (last - first) + first per axis
    (rm.py:2304-2317, then the zyx -> xyz swap of :2320-2322); the block's axes are uniform, so this is the same affine
    map without the detour through [-1, 1]."""
    org = torch.stack([bx[0], by[0], bz[0]])
    span = torch.stack([bx[-1] - bx[0], by[-1] - by[0], bz[-1] - bz[0]])
    n1 = torch.tensor([len(bx) - 1, len(by) - 1, len(bz) - 1], device=v.device, dtype=torch.float32)
    return v / n1 * span + org


def reachable_blocks(axes, block: int, pos: torch.Tensor, radius: float) -> torch.Tensor:
    """Which blocks of extract_mesh's grid can hold a point inside a field: (nbx, nby, nbz) bool, block (i, j, k) being the
    lattice axes[0][i*block : i*block + block + 1] x ... (the block loop's slices, range(0, len(axis) - 1, block) per axis:
    a one-point axis has no block and gives an empty dimension; ascending axes).  `radius` is the radius of the INSIDE TEST
    of the evaluation the result guards (the model's, or a call's mask_radius), not the map's.  A block is marked
    when some centre of `pos` (F, 3) lies within radius * (1 + 1e-3) of the block's axis-aligned box, by box distance --
    every lattice point of the block is inside the box, so an unmarked block has no point within `radius` of any centre;
    the margin covers the fp32 arithmetic of this test and of the kernels' inside test.  Conservative the other way: a
    marked block may hold no inside point (the box's corner region, or the lattice stepping over the cap).
    Pure torch on the tensors' device (CPU tensors work), no host synchronisation: one (blocks x fields) computation."""
    lo, hi = [], []
    for a in axes:
        n = a.shape[0]
        st = torch.arange(0, n - 1, block, device=a.device)
        lo.append(a[st])
        hi.append(a[torch.clamp(st + block, max=n - 1)])
    c = pos.to(torch.float32)
    d2 = 0
    for i, shape in enumerate(((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1))):
        l, h, ci = lo[i].view(shape), hi[i].view(shape), c[:, i].view(1, 1, 1, -1)
        d = torch.clamp(torch.maximum(l - ci, ci - h), min=0)              # distance of the centre to the slab [l, h]
        d2 = d2 + d * d
    reach = float(radius) * (1.0 + 1e-3)
    return (d2 <= reach * reach).any(-1)


@torch.no_grad()
def extract_mesh(renderer, mesh_file_path=None, resolution: Optional[float] = None, threshold: Optional[float] = None,
                 transform: Optional[torch.Tensor] = None, field_ids: Optional[torch.Tensor] = None, block: int = 200,
                 debug: Optional[dict] = None, fused: bool = True, stats: Optional[dict] = None):
    """NeuralGraphMap._extract_mesh (rm.py:2186-2384): bounding box of the field centres +- 2 r, grid of spacing
    `resolution` (default: the training sample spacing, rm.py:199-207), blocks of `block`^3 cells evaluated with the
    kNN-blended fields, marching cubes per block, vertex colours from a second evaluation with radius + 0.1
    (rm.py:2320-2340), one PLY + `<stem>_fields.txt`.  Returns (verts (V,3) world, faces (T,3), colours (V,3) in
    [0,255] as the reference stores them) or None when no block crosses the iso-surface.
    fused (default): a block's volume comes from ONE call (ops.grid_eval_knn: the lattice's points are formed inside the
    kernels, the geometry channel is blended -- and negated -- straight into the volume), and blocks no field can reach
    (reachable_blocks, one device computation and one transfer before the loop) launch nothing: their volume is constant,
    no grid edge is crossed.  fused=False: the staged path (cartesian_prod -> field_eval_knn in `block_size` chunks -> slice,
    reshape, negate) over every block.  The mesh is bit for bit the same either way.  With `debug` nothing is skipped.
    stats: filled with blocks_total / blocks_skipped / blocks_evaluated / blocks_with_surface.
    Vertex and face ORDER are this build's (oracle/mesh_oracle.py), not pytorch3d's: compare meshes as surfaces."""
    m = renderer._model
    dev = renderer._device
    gmd = renderer._global_map_dict
    num = gmd["num"]
    pos = gmd["positions"][:num]
    quat = gmd["orientations"][:num]
    if transform is not None:
        transform = transform.to(dev)
        pos = pos @ transform[:3, :3].T + transform[:3, 3]                     # utils.transform_points
        quat = _quat_mul(_matrix_to_quaternion(transform[:3, :3].cpu()).to(dev), quat)   # utils.transform_quaternions
    params = m.kernel_params()
    fidx = None
    if field_ids is not None:
        field_ids = field_ids[field_ids < num].to(dev)
        if len(field_ids) == 0:
            return None
        pos, quat, fidx = pos[field_ids].contiguous(), quat[field_ids].contiguous(), field_ids.contiguous()
    r = renderer._field_radius
    if resolution is None:
        cfg = renderer._config
        n_g = cfg.get("num_samples_depth_guided", 0)
        rho = cfg.get("range_depth_guided") or cfg.get("truncation_distance", 0.1)
        resolution = 2 * rho / n_g if n_g > 0 else 2 * r / cfg["num_samples_coarse"]
    axes = grid_axes(pos, r, resolution)
    mode = renderer._rc_train.geometry_mode
    isolevel, low_is_inside = {K.GEO["occupancy"]: (0.5, False), K.GEO["density"]: (30.0, False),
                               K.GEO["neus"]: (0.0, True), K.GEO["nrgbd"]: (0.0, True)}[mode]     # rm.py:2268-2289
    if threshold is not None:
        isolevel = threshold
    gfac, cfac = renderer._rc_train.geometry_factor, renderer._rc_train.color_factor
    color_radius = r + 0.1          # "avoid black colors on field boundaries" (rm.py:2332-2333): widens the inside test only,
                                    # the local coordinates keep the model's own scaling (models.py:278-285, 368-378)
    big = int(renderer._config.get("block_size", 3000000))

    def evaluate(pts, mask_radius=None):
        outs = [ops.field_eval_knn(renderer._fc, params, pts[s:s + big], pos, quat, m._num_knn, m._distance_factor,
                                   m._outside_value, fidx, mask_radius) for s in range(0, pts.shape[0], big)]
        return torch.cat(outs) if len(outs) > 1 else outs[0]

    def volume_fused(bx, by, bz):
        """the block's volume from one call, None where the block is too large for it (P K >= 2^31: the staged path takes it)"""
        try:
            vol = ops.grid_eval_knn(renderer._fc, params, bx, by, bz, pos, quat, m._num_knn, m._distance_factor,
                                    m._outside_value, fidx, None, 3, low_is_inside and mode != K.GEO["occupancy"])
        except K.NgmError as e:
            if e.code != K.NGM_E_UNSUPPORTED:
                raise
            return None
        if mode == K.GEO["occupancy"]:
            vol = torch.sigmoid(gfac * vol)
            if low_is_inside:
                vol = -vol
        return vol

    all_v, all_f, all_c, offset = [], [], [], 0
    starts = [range(0, len(a) - 1, block) for a in axes]               # blocks overlap by one grid plane (rm.py:2236-2240)
    count = dict(blocks_total=0, blocks_skipped=0, blocks_evaluated=0, blocks_with_surface=0)
    reach = None
    if fused and debug is None:
        # the radius the volume evaluation tests points against is the MODEL's (mask_radius is None there: the kernels take
        # fc.field_radius), which need not be the map's `r` that pads the box and spaces the grid
        reach = reachable_blocks(axes, block, pos, float(renderer._fc.field_radius)).cpu()   # the one transfer: (nbx, nby, nbz) bool
    for xs, ys, zs in itertools.product(*starts):
        count["blocks_total"] += 1
        if reach is not None and not bool(reach[xs // block, ys // block, zs // block]):
            count["blocks_skipped"] += 1                                # constant volume: marching cubes would return nothing
            continue
        count["blocks_evaluated"] += 1
        bx, by, bz = axes[0][xs:xs + block + 1], axes[1][ys:ys + block + 1], axes[2][zs:zs + block + 1]
        vol = volume_fused(bx, by, bz) if fused else None
        if vol is None:
            xyz = torch.cartesian_prod(bx, by, bz)
            vol = evaluate(xyz)[:, 3].reshape(len(bx), len(by), len(bz))
            if mode == K.GEO["occupancy"]:
                vol = torch.sigmoid(gfac * vol)
            if low_is_inside:
                vol = -vol
        v, f = marching_cubes(vol.contiguous(), isolevel)
        if debug is not None:      # tests: what was handed to marching cubes and what came back, per block (fixture G17)
            debug.setdefault("blocks", []).append(dict(axes=(bx, by, bz), volume=vol, isolevel=isolevel, verts_grid=v, faces=f))
            debug["color_fn"] = lambda pts: torch.clamp(cfac * evaluate(pts, color_radius)[:, :3], 0, 1) * 255
        if len(v) == 0:
            continue
        count["blocks_with_surface"] += 1
        vw = grid_to_world(v, bx, by, bz)
        col = torch.clamp(cfac * evaluate(vw, color_radius)[:, :3], 0, 1) * 255
        all_v.append(vw)
        all_f.append(f + offset)
        all_c.append(col)
        offset += len(vw)
    if stats is not None:
        stats.update(count)
    if not all_v:
        return None
    verts, faces, cols = torch.cat(all_v), torch.cat(all_f), torch.cat(all_c)
    if mesh_file_path is not None:
        stem, _ = os.path.splitext(str(mesh_file_path))
        np.savetxt(stem + "_fields.txt", pos.cpu().numpy())
        save_ply(mesh_file_path, verts, faces, cols)
    return verts, faces, cols


# ------------------------------------------------------------------------------------------------
# scoring a mesh (evaluation._evaluate_postprocessed_meshes, evaluation.py:163-208): surface samples of the estimated and
# the ground-truth mesh, two exact nearest-neighbour queries between the clouds, ten numbers.  The reference runs
# trimesh.sample.sample_surface and scipy.spatial.KDTree on the host; here both are device kernels (csrc/ngm_mesh_eval.hip)
# and the reductions are torch on the device.  Culling (mesh_culling.py) is further down: subdivide_to_size, render_mesh_depth,
# cull_mesh, evaluate_raw_mesh; ICP alignment (evaluation._align_mesh) is at the end: vertex_normals, icp_point_to_plane,
# align_mesh.  The per-frame render metrics (PSNR, SSIM, depth L1) are evaluation.py's.  OUT OF SCOPE: LPIPS.
# ------------------------------------------------------------------------------------------------
METRIC_KEYS = ("median_acc", "median_comp", "acc", "comp", "acc_ratio", "acc_ratio_1cm", "comp_ratio", "comp_ratio_1cm",
               "f1_5cm", "f1_1cm")


@ops._op("surface_sample")
def _surface_sample_op(verts: torch.Tensor, faces: torch.Tensor, num_samples: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[points (N,3) fp32, face ids (N) int64]"""
    L = K.lib()
    nf = faces.shape[0]
    wsb = L.ngm_surface_sample_workspace(nf)
    if wsb < 0:
        raise K.NgmError(f"surface_sample: {nf} faces not supported (1 <= faces < 2^31)", code=int(wsb))
    dev = verts.device
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    points = torch.empty(num_samples, 3, device=dev, dtype=torch.float32)
    face_ids = torch.empty(num_samples, device=dev, dtype=torch.int64)
    K.check(L.ngm_surface_sample(verts.data_ptr(), verts.shape[0], faces.data_ptr(), nf, num_samples, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                 points.data_ptr(), face_ids.data_ptr(), ws.data_ptr(), wsb, ops._stream()), "ngm_surface_sample")
    return points, face_ids


@_surface_sample_op.register_fake
def _(verts, faces, num_samples, seed):
    return verts.new_empty(num_samples, 3), faces.new_empty(num_samples)


@ops._op("nearest_point")
def _nearest_point_op(queries: torch.Tensor, refs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[dist (N) fp32, index (N) int64]"""
    L = K.lib()
    n, m = queries.shape[0], refs.shape[0]
    dev = queries.device
    dist = torch.empty(n, device=dev, dtype=torch.float32)
    index = torch.empty(n, device=dev, dtype=torch.int64)
    wsb = L.ngm_nearest_point_workspace(m, n)
    ws = torch.empty(max(wsb, 0), device=dev, dtype=torch.uint8)
    K.check(L.ngm_nearest_point(refs.data_ptr(), m, queries.data_ptr(), n, dist.data_ptr(), index.data_ptr(), ws.data_ptr(),
                                max(wsb, 0), ops._stream()), "ngm_nearest_point")
    return dist, index


@_nearest_point_op.register_fake
def _(queries, refs):
    return queries.new_empty(queries.shape[0]), queries.new_empty(queries.shape[0], dtype=torch.int64)


def sample_surface(verts: torch.Tensor, faces: torch.Tensor, num_points: int, seed: int = 0):
    """trimesh.sample.sample_surface (evaluation.py:190-191) on the device: verts (V, 3) fp32, faces (F, 3) int64 ->
    (points (num_points, 3) fp32, face_ids (num_points,) int64): a face with probability proportional to its area, a uniform
    point in it.  Seeded (Philox; a function of the mesh, the seed and the sample index alone), no host synchronisation.
    Faces with a non-finite vertex or an out-of-range index count as area 0 and are never drawn; a mesh whose total area
    is not > 0 gives NaN points and face ids -1.  A mesh without faces is refused.
    Dispatches through torch.ops.ngm355.surface_sample."""
    ops._require_gpu(verts, faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("sample_surface expects (V, 3) float32 vertices")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise ValueError("sample_surface expects (F, 3) int64 faces")
    num_points, seed = int(num_points), int(seed)
    if num_points < 0 or not 0 <= seed < 2 ** 63:
        raise ValueError("sample_surface: num_points >= 0 and 0 <= seed < 2^63")
    if faces.shape[0] == 0:
        raise K.NgmError("sample_surface: a mesh without faces has no surface to sample", code=K.NGM_E_INVALID)
    points, face_ids = torch.ops.ngm355.surface_sample(verts.contiguous(), faces.contiguous(), num_points, seed)
    return points, face_ids


def nearest_distances(queries: torch.Tensor, refs: torch.Tensor):
    """scipy.spatial.KDTree(refs).query(queries) (evaluation.py:75-130) on the device: queries (N, 3), refs (M, 3) fp32 ->
    (dist (N,) fp32, index (N,) int64), EXACT (a uniform grid over refs built per call, no size read back).  Ties may go to
    any of the tied indices.  Non-finite references are nobody's neighbour; a non-finite query gets (NaN, -1); with no finite
    reference every query gets (+inf, -1).  M == 0 is refused (NgmError, code NGM_E_INVALID).
    Dispatches through torch.ops.ngm355.nearest_point."""
    ops._require_gpu(queries, refs)
    for name, t in (("queries", queries), ("refs", refs)):
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError(f"nearest_distances expects (n, 3) float32 {name}")
    dist, index = torch.ops.ngm355.nearest_point(queries.contiguous(), refs.contiguous())
    return dist, index


def _np_median(d: torch.Tensor) -> torch.Tensor:
    """np.median: the mean of the two middle values for an even count (torch.median returns the lower one)"""
    s = torch.sort(d).values
    n = s.shape[0]
    return 0.5 * (s[(n - 1) // 2] + s[n // 2])


def mesh_metrics(gt_points: torch.Tensor, est_points: torch.Tensor) -> dict:
    """The ten numbers of evaluation._evaluate_postprocessed_meshes (evaluation.py:197-208) from two device clouds:
    accuracy = distance of every estimated point to its nearest ground-truth point, completion = the other way round;
    median (np.median's) and mean of each, the share below 5 cm and 1 cm (mean of `dist < th` as float32), and
    F1 = 2 / (1 / comp_ratio + 1 / acc_ratio).  Two nearest_distances calls, reductions in fp64 on the device, ONE transfer
    of ten numbers.  Differs from the reference in one place: where a ratio is 0 the reference raises ZeroDivisionError
    (evaluation.py:72); F1 is 0.0 here."""
    acc_d = nearest_distances(est_points, gt_points)[0].double()
    comp_d = nearest_distances(gt_points, est_points)[0].double()
    ratio = lambda d, th: (d < th).to(torch.float32).mean().double()
    ar5, ar1, cr5, cr1 = ratio(acc_d, 0.05), ratio(acc_d, 0.01), ratio(comp_d, 0.05), ratio(comp_d, 0.01)

    def f1(comp, acc):
        ok = (comp > 0) & (acc > 0)
        one = torch.ones_like(comp)
        return torch.where(ok, 2.0 / (1.0 / torch.where(ok, comp, one) + 1.0 / torch.where(ok, acc, one)), torch.zeros_like(comp))

    vals = torch.stack([_np_median(acc_d), _np_median(comp_d), acc_d.mean(), comp_d.mean(), ar5, ar1, cr5, cr1, f1(cr5, ar5),
                        f1(cr1, ar1)]).tolist()
    return dict(zip(METRIC_KEYS, vals))


def _as_mesh(m, device):
    if isinstance(m, (str, os.PathLike)):
        v, f, _ = load_ply(m)
        return v.to(device), f.to(device)
    return m[0], m[1]


def evaluate_mesh(est, gt, num_points: int = 200000, seed: int = 0) -> dict:
    """evaluation._evaluate_postprocessed_meshes (evaluation.py:163-208): `num_points` surface samples of each mesh
    (est with `seed`, gt with `seed + 1`), then mesh_metrics.  est / gt: a (verts, faces) pair of device tensors, or the path of
    a PLY file save_ply wrote.  The meshes are taken as they are: culling, the subdivision before it and ICP alignment are evaluate_raw_mesh's (below; align_mesh on its own)."""
    device = next((m[0].device for m in (est, gt) if not isinstance(m, (str, os.PathLike))), torch.device("cuda"))
    ev, ef = _as_mesh(est, device)
    gv, gf = _as_mesh(gt, device)
    est_points = sample_surface(ev, ef, num_points, seed)[0]
    gt_points = sample_surface(gv, gf, num_points, seed + 1)[0]
    return mesh_metrics(gt_points, est_points)


# ------------------------------------------------------------------------------------------------
# culling a mesh (mesh_culling._cull_mesh, mesh_culling.py:228-352): scene bounds, camera frusta and self-occlusion seen from
# the given poses.  The reference draws two pyrender depth maps per pose under EGL and runs about ten torch kernels per pose over
# all vertices; here the depth maps come from a HIP rasteriser and the per-vertex decisions of all poses of a chunk from one
# launch (csrc/ngm_mesh_cull.hip; the rule is written down in include/ngm_hip.h), selection and compaction are torch on the
# device.  The reference first subdivides the mesh to a maximum edge length (mesh.subdivide_to_size(max_edge),
# mesh_culling.py:260-261): subdivide_to_size below, two kernels of csrc/ngm_mesh_eval.hip, which cull_mesh runs when it is given
# max_edge.  ICP alignment is align_mesh (further down).  NOT BUILT: reading virtual-camera files (the caller appends those poses and says where they start), GL's
# top-left fill rule and depth-buffer quantisation (both far inside eps = 0.03).
# ------------------------------------------------------------------------------------------------
CULLING_METHODS = ("frustum", "occlusion", "virt_cams")


@ops._op("mesh_depth")
def _mesh_depth_op(verts: torch.Tensor, faces: torch.Tensor, c2ws: torch.Tensor, width: int, height: int, fx: float, fy: float,
                   cx: float, cy: float, near: float, far: float) -> torch.Tensor:
    """depth (P, H, W) fp32"""
    p = c2ws.shape[0]
    depth = torch.empty(p, height, width, device=verts.device, dtype=torch.float32)
    if verts.shape[0] == 0:
        return depth.zero_()                                    # the entry point launches nothing for a mesh without vertices
    K.check(K.lib().ngm_mesh_depth(verts.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0], c2ws.data_ptr(), p, width, height,
                                   fx, fy, cx, cy, near, far, depth.data_ptr(), ops._stream()), "ngm_mesh_depth")
    return depth


@_mesh_depth_op.register_fake
def _(verts, faces, c2ws, width, height, fx, fy, cx, cy, near, far):
    return verts.new_empty(c2ws.shape[0], height, width)


@ops._op("mesh_visibility")
def _mesh_visibility_op(verts: torch.Tensor, c2ws: torch.Tensor, depth: Optional[torch.Tensor], width: int, height: int, fx: float,
                        fy: float, cx: float, cy: float, eps: float, num_frustum_poses: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[in_frustum (V) int32, observed (V) int32]: the counts over the poses of this call"""
    v = verts.shape[0]
    in_frustum = torch.empty(v, device=verts.device, dtype=torch.int32).zero_()
    observed = torch.empty(v, device=verts.device, dtype=torch.int32).zero_()
    K.check(K.lib().ngm_mesh_visibility(verts.data_ptr(), v, c2ws.data_ptr(), c2ws.shape[0], width, height, fx, fy, cx, cy,
                                        ops._ptr(depth), eps, num_frustum_poses, in_frustum.data_ptr(), observed.data_ptr(),
                                        ops._stream()), "ngm_mesh_visibility")
    return in_frustum, observed


@_mesh_visibility_op.register_fake
def _(verts, c2ws, depth, width, height, fx, fy, cx, cy, eps, num_frustum_poses):
    return verts.new_empty(verts.shape[0], dtype=torch.int32), verts.new_empty(verts.shape[0], dtype=torch.int32)


SUBDIVIDE_MAX_ITER = 10                     # include/ngm_hip.h: the weights of a lattice point have at most 10 bits


@ops._op("mesh_subdivide_count")
def _mesh_subdivide_count_op(verts: torch.Tensor, faces: torch.Tensor, max_edge: float, max_iter: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """[totals (3) int64 = new vertices, output faces, largest level; the workspace (uint8) the emit call reads]"""
    L = K.lib()
    nf = faces.shape[0]
    wsb = L.ngm_mesh_subdivide_workspace(nf)
    if wsb < 0:
        raise K.NgmError(f"mesh_subdivide_count: {nf} faces not supported (faces < 2^31)", code=int(wsb))
    dev = verts.device
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    totals = torch.empty(3, device=dev, dtype=torch.int64)
    K.check(L.ngm_mesh_subdivide_count(verts.data_ptr(), verts.shape[0], faces.data_ptr(), nf, float(max_edge), int(max_iter), ws.data_ptr(),
                                       wsb, totals.data_ptr(), ops._stream()), "ngm_mesh_subdivide_count")
    return totals, ws


@_mesh_subdivide_count_op.register_fake
def _(verts, faces, max_edge, max_iter):
    nf = faces.shape[0]
    chunks = max((nf + 2047) // 2048, 1)                   # the layout of ngm_mesh_subdivide_workspace, restated for shape inference
    up = lambda b: (b + 255) // 256 * 256
    return faces.new_empty(3), verts.new_empty(256 + up(4 * nf) + 2 * up(8 * (nf + 1)) + up(8 * (chunks + 1)), dtype=torch.uint8)


@ops._op("mesh_subdivide_emit")
def _mesh_subdivide_emit_op(verts: torch.Tensor, faces: torch.Tensor, attrs: Optional[torch.Tensor], workspace: torch.Tensor,
                            new_vertices: int, out_faces: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """[verts (V + new_vertices, 3) fp32, faces (out_faces, 3) int64, attrs (V + new_vertices, C) fp32 -- C = 0 without attrs --,
    parent (out_faces) int64]"""
    nv, dev = verts.shape[0], verts.device
    if nv + new_vertices >= 2 ** 31 or out_faces >= 2 ** 31:                       # before anything is allocated
        raise K.NgmError(f"mesh_subdivide_emit: {nv + new_vertices} vertices, {out_faces} faces: the output must stay below 2^31 "
                         "vertices and 2^31 faces", code=K.NGM_E_UNSUPPORTED)
    c = 0 if attrs is None else attrs.shape[1]
    out_v = torch.empty(nv + new_vertices, 3, device=dev, dtype=torch.float32)
    out_f = torch.empty(out_faces, 3, device=dev, dtype=torch.int64)
    out_a = torch.empty(nv + new_vertices, c, device=dev, dtype=torch.float32)
    parent = torch.empty(out_faces, device=dev, dtype=torch.int64)
    K.check(K.lib().ngm_mesh_subdivide_emit(verts.data_ptr(), nv, faces.data_ptr(), faces.shape[0], ops._ptr(attrs), c, workspace.data_ptr(),
                                            new_vertices, out_faces, out_v.data_ptr(), out_f.data_ptr(), out_a.data_ptr() if c else None,
                                            parent.data_ptr(), ops._stream()), "ngm_mesh_subdivide_emit")
    return out_v, out_f, out_a, parent


@_mesh_subdivide_emit_op.register_fake
def _(verts, faces, attrs, workspace, new_vertices, out_faces):
    n = verts.shape[0] + new_vertices
    return (verts.new_empty(n, 3), faces.new_empty(out_faces, 3), verts.new_empty(n, 0 if attrs is None else attrs.shape[1]),
            faces.new_empty(out_faces))


@torch.no_grad()
def subdivide_to_size(verts: torch.Tensor, faces: torch.Tensor, max_edge: float, max_iter: int = 10, attrs: Optional[torch.Tensor] = None,
                      return_index: bool = False):
    """trimesh.Trimesh.subdivide_to_size (the first step of mesh_culling._cull_mesh, mesh_culling.py:260-261) on the device:
    verts (V, 3) fp32, faces (F, 3) int64 -> (verts, faces[, attrs][, parent]) in which no edge is longer than max_edge.
    trimesh splits every face with an edge above max_edge into four by its edge midpoints and repeats on the children; the
    children are similar to the parent, so the result per input face is the uniform split into 4^k, k the number of halvings of
    its longest edge until `L > max_edge` is false (an edge equal to max_edge is not split).  Two kernels -- count and scan,
    then emit -- with ONE read-back between them, of the three totals; the rule, the orders and why points on shared edges are
    bit-identical from both faces (no cracks for the rasteriser) are written down in include/ngm_hip.h.
    attrs (V, C) fp32: per-vertex attributes, interpolated with the same weights.  return_index: parent (F_out,) int64, the
    input face of every output face (trimesh's return_index).
    A face that needs more than max_iter halvings (a +inf edge always does) raises ValueError("max_iter exceeded") and nothing
    is returned; a face that needs EXACTLY max_iter is accepted (whether trimesh accepts it is not pinned by any
    fixture of this repository).  When nothing has to be split the INPUT tensors themselves are returned, uncopied.
    A face with a NaN edge or an index outside [0, V) is copied unchanged.  max_iter > 10 is refused: the exactness argument
    uses at most 10 weight bits.  A result of 2^31 vertices or faces or more is refused (NgmError, NGM_E_UNSUPPORTED) before
    it is allocated.
    Differences from trimesh: the outputs are fp32 (trimesh works on a float64 copy); the V input vertices stay in place and
    every split face appends its own new vertices, so a vertex on an edge shared by two split faces is stored once per face
    -- bit-identical positions, two indices.  trimesh duplicates vertices across its rounds too, and _cull_mesh loads with
    process=False: vertex counts and orders differ, the triangles do not.
    Dispatches through torch.ops.ngm355.mesh_subdivide_count / mesh_subdivide_emit."""
    ops._require_gpu(verts, faces, attrs)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("subdivide_to_size expects (V, 3) float32 vertices")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise ValueError("subdivide_to_size expects (F, 3) int64 faces")
    if attrs is not None and (attrs.dim() != 2 or attrs.shape[0] != verts.shape[0] or attrs.dtype != torch.float32):
        raise ValueError("subdivide_to_size expects (V, C) float32 attrs")
    if isinstance(max_edge, bool) or not isinstance(max_edge, (int, float)) or not (0 < max_edge < float("inf")):
        raise ValueError("subdivide_to_size: max_edge must be a finite number > 0")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or not 0 <= max_iter <= SUBDIVIDE_MAX_ITER:
        raise ValueError(f"subdivide_to_size: 0 <= max_iter <= {SUBDIVIDE_MAX_ITER}")

    def result(v, f, a, parent):
        return (v, f) + ((a,) if attrs is not None else ()) + ((parent(),) if return_index else ())

    nf = faces.shape[0]
    unsplit = lambda: torch.arange(nf, device=faces.device, dtype=torch.int64)
    if nf == 0:
        return result(verts, faces, attrs, unsplit)
    cv, cf = verts.contiguous(), faces.contiguous()
    totals, ws = torch.ops.ngm355.mesh_subdivide_count(cv, cf, float(max_edge), max_iter)
    new_vertices, out_faces, max_level = (int(t) for t in totals.tolist())        # the one read-back
    if max_level > max_iter:
        raise ValueError("max_iter exceeded")
    if new_vertices == 0:
        return result(verts, faces, attrs, unsplit)
    ca = None if attrs is None else attrs.contiguous()
    out_v, out_f, out_a, parent = torch.ops.ngm355.mesh_subdivide_emit(cv, cf, ca, ws, new_vertices, out_faces)
    return result(out_v, out_f, out_a, lambda: parent)


def _cull_inputs(fn, verts, faces, c2ws, camera):
    ops._require_gpu(verts, faces, c2ws)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError(f"{fn} expects (V, 3) float32 vertices")
    if faces is not None and (faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64):
        raise ValueError(f"{fn} expects (F, 3) int64 faces")
    if c2ws.dim() != 3 or tuple(c2ws.shape[1:]) != (4, 4) or c2ws.dtype != torch.float32:
        raise ValueError(f"{fn} expects (P, 4, 4) float32 camera-to-world poses")
    fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.5)
    return int(camera.width), int(camera.height), float(fx), float(fy), float(cx), float(cy)


def render_mesh_depth(verts: torch.Tensor, faces: torch.Tensor, c2ws: torch.Tensor, camera, near: float = 0.01, far: float = 10.0):
    """Depth maps of a mesh: verts (V, 3) fp32, faces (F, 3) int64, c2ws (P, 4, 4) fp32 camera-to-world in the OpenGL
    convention, `camera` a renderer.Camera -> (P, H, W) fp32, the camera-space z of the nearest surface at every pixel centre,
    0.0 where nothing is hit (mesh_culling._render_depth_maps_doublesided, mesh_culling.py:41-120: either winding counts).
    The rule is the contract of ngm_mesh_depth (include/ngm_hip.h).  Bitwise deterministic, no host synchronisation.
    Dispatches through torch.ops.ngm355.mesh_depth."""
    w, h, fx, fy, cx, cy = _cull_inputs("render_mesh_depth", verts, faces, c2ws, camera)
    return torch.ops.ngm355.mesh_depth(verts.contiguous(), faces.contiguous(), c2ws.contiguous(), w, h, fx, fy, cx, cy, float(near),
                                       float(far))


def mesh_visibility(verts: torch.Tensor, c2ws: torch.Tensor, camera, depth: Optional[torch.Tensor] = None, eps: float = 0.03,
                    num_frustum_poses: Optional[int] = None):
    """_cull_from_one_pose over all poses plus the sums of _apply_culling_strategy (mesh_culling.py:143-225): (in_frustum (V),
    observed (V)) int32, how many of the poses have the vertex inside the image and how many also see it, i.e. find it no
    further than `eps` behind depth (P, H, W) at its pixel.  depth None: observed = in_frustum.  Poses at or beyond
    num_frustum_poses (None: all count) add to observed only -- the virtual-camera rule.
    Dispatches through torch.ops.ngm355.mesh_visibility."""
    w, h, fx, fy, cx, cy = _cull_inputs("mesh_visibility", verts, None, c2ws, camera)
    p = c2ws.shape[0]
    if depth is not None:
        ops._require_gpu(depth)
        if tuple(depth.shape) != (p, h, w) or depth.dtype != torch.float32:
            raise ValueError(f"mesh_visibility expects ({p}, {h}, {w}) float32 depth maps")
        depth = depth.contiguous()
    nfp = p if num_frustum_poses is None else max(0, min(int(num_frustum_poses), p))
    return torch.ops.ngm355.mesh_visibility(verts.contiguous(), c2ws.contiguous(), depth, w, h, fx, fy, cx, cy, float(eps), nfp)


def _take(mask: torch.Tensor, n: int) -> torch.Tensor:
    """indices of the n set entries of `mask`, ascending, without a read-back of their number (n is known)"""
    return torch.argsort((~mask).to(torch.uint8), stable=True)[:n]


@torch.no_grad()
def cull_mesh(verts: torch.Tensor, faces: torch.Tensor, c2ws: torch.Tensor, camera, method: str, bounds=None,
              colors: Optional[torch.Tensor] = None, num_frustum_poses: Optional[int] = None, th_obs: float = 0, eps: float = 0.03,
              bounds_eps: float = 0.02, pose_chunk: int = 16, max_edge: Optional[float] = None, max_iter: int = 10):
    """mesh_culling._cull_mesh (mesh_culling.py:228-352) on the device, step by step:
      0. max_edge, when given: the mesh and its colours are subdivided first (subdivide_to_size(max_edge, max_iter)) and
         everything below runs on the result -- the reference's `subdivide=True, max_edge=0.1` (mesh_culling.py:260-261).  The
         decisions below are per vertex: they mean something only on faces that are small against the frusta.  Colours that
         are not fp32 are interpolated in fp32 and rounded back to their type.  None (default): the mesh is taken as it is;
      1. bounds (2, 3), when given: a face stays if ANY of its vertices is inside [lo - bounds_eps, hi + bounds_eps];
      2. method "occlusion" / "virt_cams": depth maps of the faces that are left, from every pose (render_mesh_depth);
      3. visibility of ALL original vertices (mesh_visibility), `pose_chunk` poses at a time so that depth memory is bounded;
      4. a face stays if any vertex has in_frustum > th_obs and -- occlusion methods -- any vertex has observed > th_obs;
      5. vertices no face refers to any more are dropped (order kept), then faces with a repeated index.
    Returns (verts, faces) or (verts, faces, colors) on the device.  One read-back (the two output sizes), at the end.
    The camera and the poses are taken AS GIVEN: _cull_mesh culls with dataset.camera.scaled_camera(0.5) and every second
    ground-truth pose (`[::2]`); the caller applies both.  "virt_cams": the caller appends the virtual poses (OpenGL convention) and
    passes the index of the first as num_frustum_poses -- they add to `observed` only.
    "frustum": the reference dies in torch.from_numpy(None) (mesh_culling.py:210-215); here it runs and does what
    remove_occlusion=False evidently means -- no depth maps, faces kept on in_frustum alone.
    A face with an index outside [0, V) is dropped (the reference would raise)."""
    if method not in CULLING_METHODS:
        raise ValueError(f"Unknown culling method {method}")                     # mesh_culling.py:373 wording
    _cull_inputs("cull_mesh", verts, faces, c2ws, camera)
    if colors is not None:
        ops._require_gpu(colors)
        if colors.shape[0] != verts.shape[0]:
            raise ValueError("cull_mesh expects one colour row per vertex")
    if int(pose_chunk) < 1:
        raise ValueError("cull_mesh: pose_chunk >= 1")
    if max_edge is not None:
        if colors is None:
            verts, faces = subdivide_to_size(verts, faces, max_edge, max_iter)
        else:
            attrs = colors.reshape(colors.shape[0], -1).to(torch.float32)
            verts, faces, attrs = subdivide_to_size(verts, faces, max_edge, max_iter, attrs=attrs)
            if not colors.dtype.is_floating_point:
                attrs = torch.round(attrs)
            colors = attrs.to(colors.dtype).reshape(attrs.shape[0], *colors.shape[1:])
    occlusion = method != "frustum"
    nv, p = verts.shape[0], c2ws.shape[0]
    verts, faces, c2ws = verts.contiguous(), faces.contiguous(), c2ws.contiguous()
    keep = ((faces >= 0) & (faces < nv)).all(1)
    idx = faces.clamp(0, max(nv - 1, 0))                                         # safe to gather with; `keep` carries validity
    if nv == 0:
        keep = torch.zeros_like(keep)
        idx = torch.zeros_like(faces)
        verts_g = verts.new_zeros(1, 3)
    else:
        verts_g = verts
    if bounds is not None:
        b = torch.as_tensor(bounds, dtype=torch.float32, device=verts.device).reshape(2, 3)
        inside = ((verts_g >= b[0] - bounds_eps) & (verts_g <= b[1] + bounds_eps)).all(1)
        keep = keep & inside[idx].any(1)
    in_frustum = torch.zeros(nv, device=verts.device, dtype=torch.int32)
    observed = torch.zeros(nv, device=verts.device, dtype=torch.int32)
    nfp = p if num_frustum_poses is None else max(0, min(int(num_frustum_poses), p))
    drawn = torch.where(keep[:, None], faces, torch.full_like(faces, -1)) if occlusion else None   # index -1: skipped by the kernel
    for s in range(0, p, int(pose_chunk)):
        chunk = c2ws[s:s + int(pose_chunk)]
        depth = render_mesh_depth(verts, drawn, chunk, camera) if occlusion else None
        inf, obs = mesh_visibility(verts, chunk, camera, depth, eps, nfp - s)
        in_frustum += inf
        observed += obs
    if nv:
        keep = keep & (in_frustum[idx] > th_obs).any(1)
        if occlusion:
            keep = keep & (observed[idx] > th_obs).any(1)
    referenced = torch.zeros(nv + 1, device=verts.device, dtype=torch.bool)
    referenced[torch.where(keep[:, None], idx, torch.full_like(idx, nv)).reshape(-1)] = True
    referenced = referenced[:nv]
    keep = keep & (idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 0] != idx[:, 2])
    n_v, n_f = torch.stack([referenced.sum(), keep.sum()]).tolist()              # the one read-back
    new_index = torch.cumsum(referenced, 0) - 1
    vsel, fsel = _take(referenced, n_v), _take(keep, n_f)
    out_faces = new_index[idx[fsel]]
    if colors is not None:
        return verts[vsel], out_faces, colors[vsel]
    return verts[vsel], out_faces


def evaluate_raw_mesh(est, gt, c2ws: torch.Tensor, camera, gt_culling_method: str, est_culling_method: str, num_points: int = 200000,
                      seed: int = 0, bounds=None, mesh_alignment: bool = False, align: Optional[str] = None, **cull_kwargs) -> dict:
    """evaluation.evaluate_raw_mesh (evaluation.py:211-251): both meshes culled (cull_mesh: the ground truth with
    gt_culling_method, the estimate with est_culling_method, the same poses, camera and bounds), then evaluate_mesh on what is
    left -- the reference's headline mesh numbers without leaving the device.  est / gt as evaluate_mesh takes them;
    cull_kwargs go to both cull_mesh calls (num_frustum_poses, th_obs, eps, bounds_eps, pose_chunk, max_edge, max_iter:
    max_edge=0.1 is the reference's default, both meshes subdivided before they are culled).
    align="icp": the reference's eval_mesh_alignment, in its order -- the ground truth is culled, the UNCULLED estimate is
    aligned to the culled ground truth (align_mesh: point-to-plane ICP, threshold 0.1, at most 100 iterations), the aligned
    estimate is culled, then scored.  None (default): no alignment; any other string is a ValueError.
    mesh_alignment=True is the reference's spelling and raises NotImplementedError: ask with align="icp"."""
    _check_align(align)
    if mesh_alignment:
        raise NotImplementedError('evaluate_raw_mesh: mesh_alignment is the reference\'s flag; here ICP alignment is asked for '
                                  'with align="icp"')
    device = next((m[0].device for m in (est, gt) if not isinstance(m, (str, os.PathLike))), c2ws.device)
    ev, ef = _as_mesh(est, device)
    gv, gf = _as_mesh(gt, device)
    gt_culled = cull_mesh(gv, gf, c2ws, camera, gt_culling_method, bounds=bounds, **cull_kwargs)
    if align == "icp":
        (ev, ef), _ = align_mesh((ev, ef), gt_culled)
    est_culled = cull_mesh(ev, ef, c2ws, camera, est_culling_method, bounds=bounds, **cull_kwargs)
    return evaluate_mesh(est_culled, gt_culled, num_points=num_points, seed=seed)


# ------------------------------------------------------------------------------------------------
# aligning a mesh to the ground truth (evaluation._align_mesh, evaluation.py:133-160): Open3D's compute_vertex_normals and
# registration_icp with TransformationEstimationPointToPlane, restated from their public definitions as device kernels
# (csrc/ngm_mesh_eval.hip; the rules are the contract of ngm_mesh_vertex_normals / ngm_icp_point_to_plane in
# include/ngm_hip.h).  PARITY UNPINNED against Open3D; tests/_mesh_align_host.py is the fp64 mirror.
# ------------------------------------------------------------------------------------------------
ICP_STATE_DOUBLES = 64                      # include/ngm_hip.h: the layout of `state`
ICP_MAX_ITERATION = 1000


def _check_align(align):
    if align is not None and align != "icp":
        raise ValueError(f'Unknown alignment {align!r}: None or "icp"')


@ops._op("mesh_vertex_normals")
def _mesh_vertex_normals_op(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """normals (V, 3) fp32"""
    L = K.lib()
    nv = verts.shape[0]
    wsb = L.ngm_mesh_vertex_normals_workspace(nv)
    if wsb < 0:
        raise K.NgmError(f"mesh_vertex_normals: {nv} vertices not supported (vertices < 2^31)", code=int(wsb))
    ws = torch.empty(wsb, device=verts.device, dtype=torch.uint8)
    normals = torch.empty(nv, 3, device=verts.device, dtype=torch.float32)
    K.check(L.ngm_mesh_vertex_normals(verts.data_ptr(), nv, faces.data_ptr(), faces.shape[0], normals.data_ptr(), ws.data_ptr(), wsb,
                                      ops._stream()), "ngm_mesh_vertex_normals")
    return normals


@_mesh_vertex_normals_op.register_fake
def _(verts, faces):
    return verts.new_empty(verts.shape[0], 3)


@ops._op("icp_point_to_plane")
def _icp_point_to_plane_op(source: torch.Tensor, target: torch.Tensor, target_normals: torch.Tensor, threshold: float,
                           max_iteration: int, relative_fitness: float, relative_rmse: float, init: List[float]) -> torch.Tensor:
    """state (64) fp64: the layout of include/ngm_hip.h"""
    L = K.lib()
    n, m = source.shape[0], target.shape[0]
    wsb = L.ngm_icp_point_to_plane_workspace(m, n)
    if wsb < 0:
        raise K.NgmError(f"icp_point_to_plane: {n} source and {m} target points not supported (1 <= target, both < 2^31)", code=int(wsb))
    ws = torch.empty(wsb, device=source.device, dtype=torch.uint8)
    state = torch.empty(ICP_STATE_DOUBLES, device=source.device, dtype=torch.float64)
    init_c = (C.c_double * 16)(*init)
    K.check(L.ngm_icp_point_to_plane(source.data_ptr(), n, target.data_ptr(), target_normals.data_ptr(), m, float(threshold),
                                     int(max_iteration), float(relative_fitness), float(relative_rmse), init_c, state.data_ptr(),
                                     ws.data_ptr(), wsb, ops._stream()), "ngm_icp_point_to_plane")
    return state


@_icp_point_to_plane_op.register_fake
def _(source, target, target_normals, threshold, max_iteration, relative_fitness, relative_rmse, init):
    return source.new_empty(ICP_STATE_DOUBLES, dtype=torch.float64)


def vertex_normals(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """Open3D's compute_vertex_normals on the device: verts (V, 3) fp32, faces (F, 3) int64 -> (V, 3) fp32 unit normals, every
    face's unnormalised normal (v1 - v0) x (v2 - v0) added to its three vertices (area weighting) and the sum normalised.
    (0, 0, 1) for a vertex whose sum has length 0 (no face, exact cancellation) or that is not finite; a face with an
    out-of-range index or a non-finite vertex adds nothing.  Exact integer sums: independent of the order of the faces, bitwise
    equal from call to call.  No host synchronisation.  Dispatches through torch.ops.ngm355.mesh_vertex_normals."""
    ops._require_gpu(verts, faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("vertex_normals expects (V, 3) float32 vertices")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int64:
        raise ValueError("vertex_normals expects (F, 3) int64 faces")
    return torch.ops.ngm355.mesh_vertex_normals(verts.contiguous(), faces.contiguous())


class IcpResult:
    """What icp_point_to_plane returns, every field a DEVICE tensor (nothing has been read back): transformation (4, 4) fp64,
    fitness and inlier_rmse (fp64 scalars), iterations (int64 scalar: updates applied), converged (bool scalar); `state`
    is the raw (64,) record of ngm_icp_point_to_plane (the last pass's sums are state[20:49])."""

    def __init__(self, state: torch.Tensor):
        self.state = state
        self.transformation = state[:16].view(4, 4)
        self.fitness = state[16]
        self.inlier_rmse = state[17]
        self.iterations = state[18].to(torch.int64)
        self.converged = state[19] != 0

    def __repr__(self):
        return "IcpResult(device tensors: transformation, fitness, inlier_rmse, iterations, converged)"


def icp_point_to_plane(source: torch.Tensor, target: torch.Tensor, target_normals: torch.Tensor, threshold: float = 0.1,
                       max_iteration: int = 100, init=None, relative_fitness: float = 1e-6, relative_rmse: float = 1e-6) -> IcpResult:
    """Open3D's registration_icp(source, target, threshold, init, TransformationEstimationPointToPlane(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) on the device: source (N, 3), target (M, 3),
    target_normals (M, 3) fp32 -> IcpResult.  init: None (identity) or a (4, 4) HOST array (numpy, nested lists, CPU tensor).
    The grid over the target is built once, every iteration is two launches, all of them enqueued at once: no host
    synchronisation, and the call can be captured in a graph.  Deterministic: equal distances go to the smallest target index,
    every sum has a fixed order.  A system that is singular by the rule of include/ngm_hip.h (a planar target) leaves the
    transformation unchanged.  M == 0 is refused (NgmError, NGM_E_INVALID).
    Dispatches through torch.ops.ngm355.icp_point_to_plane."""
    ops._require_gpu(source, target, target_normals)
    for name, t in (("source", source), ("target", target), ("target_normals", target_normals)):
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError(f"icp_point_to_plane expects (n, 3) float32 {name}")
    if target_normals.shape[0] != target.shape[0]:
        raise ValueError("icp_point_to_plane expects one normal per target point")
    threshold = float(threshold)
    if not (0 < threshold < float("inf")):
        raise ValueError("icp_point_to_plane: threshold must be a finite number > 0")
    if isinstance(max_iteration, bool) or not isinstance(max_iteration, int) or not 0 <= max_iteration <= ICP_MAX_ITERATION:
        raise ValueError(f"icp_point_to_plane: 0 <= max_iteration <= {ICP_MAX_ITERATION}")
    if init is None:
        init_l = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    else:
        if isinstance(init, torch.Tensor) and init.is_cuda:
            raise ValueError("icp_point_to_plane: init is a host array (a device tensor would have to be read back)")
        init_l = [float(x) for x in np.asarray(init, dtype=np.float64).reshape(-1)]
        if len(init_l) != 16:
            raise ValueError("icp_point_to_plane: init must be a (4, 4) transformation")
    state = torch.ops.ngm355.icp_point_to_plane(source.contiguous(), target.contiguous(), target_normals.contiguous(), threshold,
                                                max_iteration, float(relative_fitness), float(relative_rmse), init_l)
    return IcpResult(state)


def transform_vertices(verts: torch.Tensor, transformation: torch.Tensor) -> torch.Tensor:
    """R v + t in fp64, ((R0 x + R1 y) + R2 z) + t per row, rounded once to fp32: verts (V, 3) fp32, transformation (4, 4) fp64"""
    v = verts.double()
    T = transformation.to(device=verts.device, dtype=torch.float64)
    x, y, z = v[:, 0:1], v[:, 1:2], v[:, 2:3]
    return (((x * T[:3, 0] + y * T[:3, 1]) + z * T[:3, 2]) + T[:3, 3]).float()


@torch.no_grad()
def align_mesh(est, gt, threshold: float = 0.1, max_iteration: int = 100, init=None, relative_fitness: float = 1e-6,
               relative_rmse: float = 1e-6):
    """evaluation._align_mesh (evaluation.py:133-160) on the device: the vertex normals of `gt` (vertex_normals), point-to-plane
    ICP from est's vertices to gt's vertices (icp_point_to_plane with the reference's threshold 0.1, identity start and at most
    100 iterations by default), and est moved by the result.  est / gt as evaluate_mesh takes them; a third element of est
    (colours) is handed through.  Returns (est with its vertices at R v + t -- fp64, rounded to fp32; faces and colours are
    the SAME tensors --, IcpResult).  Nothing is read back."""
    device = next((m[0].device for m in (est, gt) if not isinstance(m, (str, os.PathLike))), torch.device("cuda"))
    rest = () if isinstance(est, (str, os.PathLike)) else tuple(est[2:])
    ev, ef = _as_mesh(est, device)
    gv, gf = _as_mesh(gt, device)
    result = icp_point_to_plane(ev, gv, vertex_normals(gv, gf), threshold=threshold, max_iteration=max_iteration, init=init,
                                relative_fitness=relative_fitness, relative_rmse=relative_rmse)
    return (transform_vertices(ev, result.transformation), ef) + rest, result
