"""Host mirror (numpy, fp64) of the mesh-scoring kernels (csrc/ngm_mesh_eval.hip; include/ngm_hip.h ngm_surface_sample /
ngm_nearest_point) and of mesh.mesh_metrics.  TEST INFRASTRUCTURE: the yardstick of tests/test_mesh_metrics_cpu.py and
tests/test_gpu_mesh_metrics.py.
  sample_surface   : the sampler's values drawn through tests/_philox_host.py: block = sample index of the sampler's stream,
                     words 0 and 1 the 53-bit face draw, words 2 and 3 the 24-bit (u, v); fp32 face areas as the kernel forms
                     them, their fp64 running sum, the first cum[k] > u * total; the point itself in fp64
  nearest          : brute force in chunks of explicit differences (no |a|^2 + |b|^2 - 2 a.b trick), fp64
  metrics          : the ten numbers of evaluation._evaluate_postprocessed_meshes from the two distance vectors
"""
import numpy as np

from _philox_host import philox4x32_10_words

MESH_STREAM_SURFACE = 0x54470006
METRIC_KEYS = ("median_acc", "median_comp", "acc", "comp", "acc_ratio", "acc_ratio_1cm", "comp_ratio", "comp_ratio_1cm",
               "f1_5cm", "f1_1cm")


def face_areas(verts, faces):
    """fp32 area per face, every product and sum rounded on its own, as k_face_area; 0 for a face with an index outside
    [0, V) or a non-finite vertex -> (F,) float64"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    ok = ((faces >= 0) & (faces < V)).all(1)
    f = np.where(ok[:, None], faces, 0) if V else np.zeros_like(faces)
    if V == 0:
        return np.zeros(len(faces))
    p = verts[f]                                                     # (F, 3 corners, 3)
    ok &= np.isfinite(p).all((1, 2))
    with np.errstate(all="ignore"):
        a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        cy = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        cz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        ar = np.float32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
    assert ar.dtype == np.float32
    ar = np.where(ok & np.isfinite(ar), ar, np.float32(0))
    return ar.astype(np.float64)


def sample_surface(verts, faces, num_points, seed=0):
    """-> dict(points (N, 3) float64, face_ids (N,) int64, uv (N, 2) float32 after the reflection, boundary_gap (N,) float64:
    distance of the face draw u * total to the nearest cumulative-area boundary, as a fraction of the total, area (F,), total,
    cum (F,) the running sum, target (N,) the face draws u * total)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    N, F = int(num_points), len(faces)
    area = face_areas(verts, faces)
    cum = np.cumsum(area)
    total = float(cum[-1]) if F else 0.0
    if not (total > 0 and np.isfinite(total)):
        return dict(points=np.full((N, 3), np.nan), face_ids=np.full(N, -1, np.int64), uv=np.zeros((N, 2), np.float32),
                    boundary_gap=np.zeros(N), area=area, total=total)
    i = np.arange(N, dtype=np.uint64)
    w = philox4x32_10_words(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.full_like(i, np.uint64(MESH_STREAM_SURFACE)),
                            np.zeros_like(i), int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    u53 = (((w[0] >> np.uint64(5)) << np.uint64(26)) | (w[1] >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)
    target = u53 * total
    k = np.minimum(np.searchsorted(cum, target, side="right"), F - 1)            # first cum[k] > target
    pos = np.flatnonzero(area > 0)
    for j in np.flatnonzero(area[k] == 0):                                     # (u * total rounded up to total)
        later = pos[pos > k[j]]
        k[j] = later[0] if len(later) else pos[pos < k[j]][-1]
    lower = np.where(k > 0, cum[np.maximum(k - 1, 0)], 0.0)
    gap = np.minimum(np.abs(target - lower), np.abs(cum[k] - target)) / total    # (0 and the total count as boundaries too)
    u = (w[2] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    v = (w[3] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    flip = (u + v) > np.float32(1.0)                                             # decided in fp32, as the kernel does
    u, v = np.where(flip, np.float32(1.0) - u, u), np.where(flip, np.float32(1.0) - v, v)
    p = verts[faces[k]].astype(np.float64)
    pts = p[:, 0] + u.astype(np.float64)[:, None] * (p[:, 1] - p[:, 0]) + v.astype(np.float64)[:, None] * (p[:, 2] - p[:, 0])
    return dict(points=pts, face_ids=k.astype(np.int64), uv=np.stack([u, v], 1), boundary_gap=gap, area=area, total=total,
                cum=cum, target=target)


def nearest(queries, refs, chunk=512):
    """-> (dist (N,) float64, index (N,) int64).  Non-finite references are left out; a non-finite query gets (NaN, -1); with
    no finite reference every query gets (+inf, -1)."""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    r = np.asarray(refs, np.float64).reshape(-1, 3)
    keep = np.flatnonzero(np.isfinite(r).all(1))
    r = r[keep]
    dist = np.full(len(q), np.inf)
    index = np.full(len(q), -1, np.int64)
    qok = np.isfinite(q).all(1)
    dist[~qok] = np.nan
    if len(r):
        ids = np.flatnonzero(qok)
        for s in range(0, len(ids), chunk):
            sel = ids[s:s + chunk]
            d2 = np.zeros((len(sel), len(r)))
            for a in range(3):
                d = q[sel, a][:, None] - r[None, :, a]
                d2 += d * d
            j = d2.argmin(1)
            dist[sel] = np.sqrt(d2[np.arange(len(sel)), j])
            index[sel] = keep[j]
    return dist, index


def distance_to(queries, refs, index):
    """fp64 distance of every query to refs[index] (index >= 0)"""
    q = np.asarray(queries, np.float64).reshape(-1, 3)
    r = np.asarray(refs, np.float64).reshape(-1, 3)
    return np.sqrt(((q - r[index]) ** 2).sum(1))


def metrics(acc_d, comp_d):
    """acc_d: distance of every estimated point to the ground truth, comp_d: of every ground-truth point to the estimate
    (evaluation.py:75-130, 197-208).  F1 is 0.0 where a ratio is 0 (the reference raises ZeroDivisionError there)."""
    acc_d, comp_d = np.asarray(acc_d, np.float64), np.asarray(comp_d, np.float64)
    ratio = lambda d, th: np.mean((d < th).astype(np.float32)).item()
    f1 = lambda comp, acc: 2.0 / (1.0 / comp + 1.0 / acc) if comp > 0 and acc > 0 else 0.0
    m = dict(median_acc=np.median(acc_d).item(), median_comp=np.median(comp_d).item(), acc=np.mean(acc_d).item(),
             comp=np.mean(comp_d).item(), acc_ratio=ratio(acc_d, 0.05), acc_ratio_1cm=ratio(acc_d, 0.01),
             comp_ratio=ratio(comp_d, 0.05), comp_ratio_1cm=ratio(comp_d, 0.01))
    m["f1_5cm"] = f1(m["comp_ratio"], m["acc_ratio"])
    m["f1_1cm"] = f1(m["comp_ratio_1cm"], m["acc_ratio_1cm"])
    return {k: m[k] for k in METRIC_KEYS}


def sampler_test_mesh(seed=27):
    """About 100 faces over a strip of triangles whose areas span 1 : 1000, with some faces of zero area (a repeated vertex,
    three collinear points), one face with an index outside the vertex array and one with a NaN vertex -> (verts (V, 3)
    float32, faces (F, 3) int64, dict of the special face ids)"""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    n = 96
    sizes = np.geomspace(0.03, 0.03 * np.sqrt(1000.0), n)              # edge lengths: areas 1 : 1000
    rng.shuffle(sizes)
    for s in sizes:
        o = rng.uniform(-2, 2, 3)
        e1 = rng.normal(size=3); e1 /= np.linalg.norm(e1)
        e2 = np.cross(e1, rng.normal(size=3)); e2 /= np.linalg.norm(e2)
        b = len(verts)
        verts += [o, o + s * e1, o + s * rng.uniform(0.2, 0.8) * e1 + s * e2]
        faces.append([b, b + 1, b + 2])
    special = {}
    faces.insert(10, [3, 3, 4]); special["repeated"] = 10              # zero area: a repeated vertex
    b = len(verts)
    verts += [np.array([0.0, 0, 0]), np.array([1.0, 1, 1]), np.array([2.0, 2, 2])]
    faces.insert(40, [b, b + 1, b + 2]); special["collinear"] = 40     # zero area: collinear
    faces.insert(60, [0, 1, 10 ** 6]); special["out_of_range"] = 60
    b = len(verts)
    verts += [np.array([np.nan, 0.0, 0.0])]
    faces.insert(80, [0, 1, b]); special["nan_vertex"] = 80
    faces.append([5, 5, 5]); special["last_degenerate"] = len(faces) - 1
    return np.asarray(verts, np.float32), np.asarray(faces, np.int64), special
