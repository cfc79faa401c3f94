"""Host mirror (numpy, fp64) of mesh culling (csrc/ngm_mesh_cull.hip; include/ngm_hip.h ngm_mesh_depth / ngm_mesh_visibility;
mesh.render_mesh_depth / mesh_visibility / cull_mesh).  TEST INFRASTRUCTURE: the yardstick of tests/test_mesh_cull_cpu.py and
tests/test_gpu_mesh_cull.py, itself held to the reference's own masks by fixture G29 (tests/golden/make_golden_mesh_cull.py).

Besides its results every function returns DOUBT flags: what a correct fp32 kernel may decide differently.
  a pixel is doubtful when
    - an edge of some (clipped) triangle passes within DELTA * max(1, m / 1024) px of its sample point, m that triangle's
      largest absolute screen coordinate: an fp32 screen coordinate below 2^10 px carries 2^-13 px per rounding, and there are
      a few tens of roundings from the vertex to the edge function, hence DELTA = 2^-9 px;
    - its two nearest candidate depths differ by less than DEPTH_DOUBT (relative), or a candidate is that close to `far`.
  a (vertex, pose) pair is doubtful when px or py is within DELTA of a bound; px or py is within DELTA of an integer and the
  neighbouring pixel would change the decision; |pz| < 1e-6; |pz - depth - eps| < 1e-5 max(1, pz); or its pixel is doubtful."""
import numpy as np

DELTA = 2.0 ** -9
DEPTH_DOUBT = 1e-4        # the largest depth bar the GPU test may come out with (its condition): doubt is judged at that
SMALL = 18                # boxes up to SMALL x SMALL pixels are rasterised for all triangles at once, offset by offset


def make_cam(width, height, fx, fy, cx, cy):
    """cx, cy in the 0.5-pixel-centre convention (Camera.get_pinhole_camera_parameters(0.5))"""
    return dict(W=int(width), H=int(height), fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy))


def world_to_camera(c2w):
    """(R (3,3), t (3,)) of the OpenCV world-to-camera of an OpenGL camera-to-world pose: columns 1 and 2 negated, the affine part
    inverted by adjugate.  None for a pose with a non-finite entry."""
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    if not np.isfinite(m).all():
        return None
    r = m[:3, :3].copy()
    r[:, 1] *= -1
    r[:, 2] *= -1
    c = np.array([[r[1, 1] * r[2, 2] - r[1, 2] * r[2, 1], r[0, 2] * r[2, 1] - r[0, 1] * r[2, 2], r[0, 1] * r[1, 2] - r[0, 2] * r[1, 1]],
                  [r[1, 2] * r[2, 0] - r[1, 0] * r[2, 2], r[0, 0] * r[2, 2] - r[0, 2] * r[2, 0], r[0, 2] * r[1, 0] - r[0, 0] * r[1, 2]],
                  [r[1, 0] * r[2, 1] - r[1, 1] * r[2, 0], r[0, 1] * r[2, 0] - r[0, 0] * r[2, 1], r[0, 0] * r[1, 1] - r[0, 1] * r[1, 0]]])
    det = r[0, 0] * c[0, 0] + r[0, 1] * c[1, 0] + r[0, 2] * c[2, 0]
    with np.errstate(all="ignore"):
        w = c / det
        t = -(w[:, 0] * m[0, 3] + w[:, 1] * m[1, 3] + w[:, 2] * m[2, 3])
    return w, t


# ------------------------------------------------------------------------------------------------ the rasterisation rule
def _clip(c, near):
    """one camera-space triangle (3, 3) against z >= near, the kernel's walk: corners in front are kept, a crossing is formed from
    the corner in front towards the one behind and has z = near -> list of (3, 3) triangles (0 1 2 and 0 2 3 of the polygon)"""
    q = []
    for i in range(3):
        j = (i + 1) % 3
        in_i, in_j = c[i, 2] >= near, c[j, 2] >= near
        if in_i:
            q.append(c[i])
        if in_i != in_j:
            a, b = (c[i], c[j]) if in_i else (c[j], c[i])
            s = (a[2] - near) / (a[2] - b[2])
            q.append(np.array([a[0] + s * (b[0] - a[0]), a[1] + s * (b[1] - a[1]), near]))
    if len(q) < 3:
        return []
    out = [np.stack([q[0], q[1], q[2]])]
    if len(q) == 4:
        out.append(np.stack([q[0], q[2], q[3]]))
    return out


def _segment_distance(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    l2 = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        s = np.where(l2 > 0, ((px - ax) * dx + (py - ay) * dy) / np.where(l2 > 0, l2, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)
    ex, ey = px - (ax + s * dx), py - (ay + s * dy)
    return np.sqrt(ex * ex + ey * ey)


def _samples(x, y, iz, tol, u, v, far):
    """triangles (n, 3) against one pixel each (u, v (n,)): covered (inside or on, either winding, 0 < z <= far), z, doubtful"""
    px, py = u + 0.5, v + 0.5
    w0 = (x[:, 2] - x[:, 1]) * (py - y[:, 1]) - (y[:, 2] - y[:, 1]) * (px - x[:, 1])
    w1 = (x[:, 0] - x[:, 2]) * (py - y[:, 2]) - (y[:, 0] - y[:, 2]) * (px - x[:, 2])
    w2 = (x[:, 1] - x[:, 0]) * (py - y[:, 0]) - (y[:, 1] - y[:, 0]) * (px - x[:, 0])
    inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
    with np.errstate(all="ignore"):
        z = (w0 + w1 + w2) / (w0 * iz[:, 0] + w1 * iz[:, 1] + w2 * iz[:, 2])
    ok = inside & (z > 0) & (z <= far)
    d = np.minimum(np.minimum(_segment_distance(px, py, x[:, 0], y[:, 0], x[:, 1], y[:, 1]),
                              _segment_distance(px, py, x[:, 1], y[:, 1], x[:, 2], y[:, 2])),
                   _segment_distance(px, py, x[:, 2], y[:, 2], x[:, 0], y[:, 0]))
    doubt = (d < tol) | (inside & (np.abs(z - far) < DEPTH_DOUBT * far))
    return ok, z, doubt


def render_depth(verts, faces, c2ws, cam, near=0.01, far=10.0, stats=None):
    """-> depth (P, H, W) fp64 (0 where nothing is hit), doubt (P, H, W) bool.  stats: filled with `covered` (pixels hit)."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    c2ws = np.asarray(c2ws).reshape(-1, 4, 4)
    W, H = cam["W"], cam["H"]
    nv = len(verts)
    fok = ((faces >= 0) & (faces < nv)).all(1) if len(faces) else np.zeros(0, bool)
    corners = verts[np.where(fok[:, None], faces, 0)] if nv else np.zeros((len(faces), 3, 3))
    fok = fok & np.isfinite(corners).all((1, 2))
    corners = corners[fok]
    depth = np.zeros((len(c2ws), H, W))
    doubt = np.zeros((len(c2ws), H, W), bool)
    for p, c2w in enumerate(c2ws):
        wt = world_to_camera(c2w)
        if wt is None or len(corners) == 0:
            continue
        with np.errstate(all="ignore"):
            cs = corners @ wt[0].T + wt[1]
        cs = cs[np.isfinite(cs).all((1, 2))]
        front = (cs[:, :, 2] >= near).sum(1)
        tris = [cs[front == 3]] + [np.stack(t) for c in cs[(front > 0) & (front < 3)] for t in [_clip(c, near)] if t]
        tris = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        if not len(tris):
            continue
        x = cam["fx"] * tris[:, :, 0] / tris[:, :, 2] + cam["cx"]
        y = cam["fy"] * tris[:, :, 1] / tris[:, :, 2] + cam["cy"]
        iz = 1.0 / tris[:, :, 2]
        area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        keep = area2 != 0
        x, y, iz = x[keep], y[keep], iz[keep]
        tol = DELTA * np.maximum(1.0, np.maximum(np.abs(x).max(1), np.abs(y).max(1)) / 1024.0)
        # the pixels whose samples the box holds, widened by one pixel for the doubt flags
        u0 = np.clip(np.ceil(x.min(1) - 0.5) - 1, 0, W).astype(np.int64)
        u1 = np.clip(np.floor(x.max(1) - 0.5) + 1, -1, W - 1).astype(np.int64)
        v0 = np.clip(np.ceil(y.min(1) - 0.5) - 1, 0, H).astype(np.int64)
        v1 = np.clip(np.floor(y.max(1) - 0.5) + 1, -1, H - 1).astype(np.int64)
        bw, bh = u1 - u0 + 1, v1 - v0 + 1
        live = (bw > 0) & (bh > 0)
        small = live & (bw <= SMALL) & (bh <= SMALL)
        cand_pix, cand_z, doubt_pix = [], [], []

        def run(sel, u, v):
            ok, z, db = _samples(x[sel], y[sel], iz[sel], tol[sel], u, v, far)
            pix = v * W + u
            cand_pix.append(pix[ok]); cand_z.append(z[ok]); doubt_pix.append(pix[db])

        for dv in range(int(bh[small].max()) if small.any() else 0):
            for du in range(int(bw[small].max()) if small.any() else 0):
                sel = np.nonzero(small & (du < bw) & (dv < bh))[0]
                if len(sel):
                    run(sel, u0[sel] + du, v0[sel] + dv)
        for k in np.nonzero(live & ~small)[0]:
            vv, uu = np.meshgrid(np.arange(v0[k], v1[k] + 1), np.arange(u0[k], u1[k] + 1), indexing="ij")
            run(np.full(uu.size, k), uu.reshape(-1), vv.reshape(-1))
        if not cand_pix:
            continue
        pix, z = np.concatenate(cand_pix), np.concatenate(cand_z)
        order = np.lexsort((z, pix))
        pix, z = pix[order], z[order]
        first = np.ones(len(pix), bool)
        first[1:] = pix[1:] != pix[:-1]
        i1 = np.nonzero(first)[0]
        d, db = depth[p].reshape(-1), doubt[p].reshape(-1)
        d[pix[i1]] = z[i1]
        has2 = (i1 + 1 < len(pix)) & ~np.append(first[1:], True)[i1]
        close = np.zeros(len(i1), bool)
        close[has2] = (z[i1[has2] + 1] - z[i1[has2]]) < DEPTH_DOUBT * z[i1[has2]]
        db[pix[i1[close]]] = True
        db[np.concatenate(doubt_pix)] = True
    if stats is not None:
        stats["covered"] = int((depth > 0).sum())
    return depth, doubt


# ------------------------------------------------------------------------------------------------ the visibility decisions
def visibility(verts, c2ws, cam, depth=None, eps=0.03, pixel_doubt=None):
    """_cull_from_one_pose per pose (mesh_culling.py:143-190) in fp64 -> inside (P, V), seen (P, V), doubt (P, V) bool.
    depth (P, H, W) or None (seen = inside); pixel_doubt (P, H, W): render_depth's flags for those maps."""
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    c2ws = np.asarray(c2ws).reshape(-1, 4, 4)
    W, H = cam["W"], cam["H"]
    P, V = len(c2ws), len(verts)
    inside, seen, doubt = np.zeros((P, V), bool), np.zeros((P, V), bool), np.zeros((P, V), bool)
    for p, c2w in enumerate(c2ws):
        wt = world_to_camera(c2w)
        if wt is None:
            continue
        with np.errstate(all="ignore"):
            c = verts @ wt[0].T + wt[1]
            pz = c[:, 2] + 1e-8
            px = (cam["fx"] * c[:, 0] + cam["cx"] * c[:, 2]) / pz
            py = (cam["fy"] * c[:, 1] + cam["cy"] * c[:, 2]) / pz
            ins = (0 <= px) & (px <= W - 1) & (0 <= py) & (py <= H - 1) & (pz > 0)
            db = (np.abs(px) < DELTA) | (np.abs(px - (W - 1)) < DELTA) | (np.abs(py) < DELTA) | (np.abs(py - (H - 1)) < DELTA)
            db |= np.abs(pz) < 1e-6
        u = np.clip(np.where(ins, px, 0), 0, W - 1).astype(np.int64)
        v = np.clip(np.where(ins, py, 0), 0, H - 1).astype(np.int64)
        s = ins.copy()
        if depth is not None:
            dm = np.asarray(depth[p], np.float64)
            s = ins & (pz < dm[v, u] + eps)
            db |= ins & (np.abs(pz - dm[v, u] - eps) < 1e-5 * np.maximum(1.0, pz))
            # the pixel on the other side of an integer that px / py nearly is
            ru, rv = np.rint(np.where(ins, px, 0)), np.rint(np.where(ins, py, 0))
            for near_int, uu, vv in ((np.abs(px - ru) < DELTA, np.clip(np.stack([ru - 1, ru]), 0, W - 1).astype(np.int64), None),
                                     (np.abs(py - rv) < DELTA, None, np.clip(np.stack([rv - 1, rv]), 0, H - 1).astype(np.int64))):
                for k in range(2):
                    alt = pz < dm[v if vv is None else vv[k], u if uu is None else uu[k]] + eps
                    db |= ins & near_int & (alt != s)
            if pixel_doubt is not None:
                db |= ins & np.asarray(pixel_doubt[p], bool)[v, u]
        inside[p], seen[p], doubt[p] = ins, s, db
    return inside, seen, doubt


# ------------------------------------------------------------------------------------------------ bounds, faces, compaction
def cull_by_bounds(verts, bounds, eps=0.02):
    """_cull_by_bounds (mesh_culling.py:123-140) per vertex; the thresholds are float32 (bounds) -/+ eps rounded to float32, as
    numpy forms them from the dataset's float32 bounds"""
    b = np.asarray(bounds, np.float32).reshape(2, 3)
    lo, hi = (b[0] - np.float32(eps)).astype(np.float64), (b[1] + np.float32(eps)).astype(np.float64)
    verts = np.asarray(verts, np.float64).reshape(-1, 3)
    return (verts >= lo).all(1) & (verts <= hi).all(1)


def select_faces(faces, in_frustum, observed=None, th_obs=0, start=None):
    """mesh_culling.py:334-346: a face stays if any vertex has in_frustum > th_obs and (observed given) any has observed > th_obs;
    start (F,) bool: the faces still there (the bounds rule)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.ones(len(faces), bool) if start is None else np.asarray(start, bool).copy()
    keep &= (np.asarray(in_frustum)[faces] > th_obs).any(1)
    if observed is not None:
        keep &= (np.asarray(observed)[faces] > th_obs).any(1)
    return keep


def compact(verts, faces, keep, colors=None):
    """trimesh's remove_unreferenced_vertices, then remove_degenerate_faces as the issue states it (mesh_culling.py:349-351):
    vertices no kept face refers to are dropped, order kept; then faces with a repeated index are dropped"""
    verts, faces = np.asarray(verts), np.asarray(faces, np.int64).reshape(-1, 3)
    f = faces[np.asarray(keep, bool)]
    ref = np.zeros(len(verts), bool)
    ref[f.reshape(-1)] = True
    new = np.cumsum(ref) - 1
    f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]
    out = (verts[ref], new[f])
    return out + (np.asarray(colors)[ref],) if colors is not None else out


def cull(verts, faces, c2ws, cam, method, bounds=None, num_frustum_poses=None, th_obs=0, eps=0.03, bounds_eps=0.02, near=0.01, far=10.0):
    """mesh.cull_mesh, step by step -> dict: verts, faces (the culled mesh), keep (F,) bool before the repeated-index rule,
    start (F,) bool (faces the bounds rule leaves), face_doubt (F,) bool: faces whose fate a doubtful (vertex, pose) pair decides."""
    verts64 = np.asarray(verts, np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    c2ws = np.asarray(c2ws).reshape(-1, 4, 4)
    P = len(c2ws)
    nfp = P if num_frustum_poses is None else max(0, min(int(num_frustum_poses), P))
    start = ((faces >= 0) & (faces < len(verts64))).all(1)
    safe = np.where(start[:, None], faces, 0)
    if bounds is not None:
        start &= cull_by_bounds(verts64, bounds, bounds_eps)[safe].any(1)
    depth = pdoubt = None
    if method != "frustum":
        depth, pdoubt = render_depth(verts64, faces[start], c2ws, cam, near, far)
        depth = depth.astype(np.float32)                                    # what the visibility kernel is handed
    ins, seen, db = visibility(verts64, c2ws, cam, depth, eps, pdoubt)
    keeps = []
    for sign in (0, -1, 1):                                                 # as decided; every doubtful pair against; every one for
        i = ins if sign == 0 else (ins & ~db if sign < 0 else ins | db)
        s = seen if sign == 0 else (seen & ~db if sign < 0 else seen | db)
        keeps.append(select_faces(safe, i[:nfp].sum(0), s.sum(0) if method != "frustum" else None, th_obs, start))
    out_v, out_f = compact(np.asarray(verts), safe, keeps[0])
    return dict(verts=out_v, faces=out_f, keep=keeps[0], start=start, face_doubt=keeps[1] != keeps[2], depth=depth,
                pixel_doubt=pdoubt, pair_doubt=db)


# ------------------------------------------------------------------------------------------------ fixture G29
def load_g29(path):
    """tests/golden/g29_mesh_cull.npz (make_golden_mesh_cull.py) -> dict; depth (P, H, W) float32 = counts * step, exact"""
    g = np.load(path)
    w, h, fx, fy, cx, cy = g["intrinsics"]
    verts = g["verts"]
    nv, npose = len(verts), len(g["c2ws"])
    unpack = lambda a: np.unpackbits(a, axis=1, count=nv).astype(bool)
    return dict(verts=verts, faces=g["faces"].astype(np.int64), c2ws=g["c2ws"], cam=make_cam(w, h, fx, fy, cx, cy), bounds=g["bounds"],
                depth=(g["depth_counts"].astype(np.float64) * float(g["depth_step"])).astype(np.float32), depth_counts=g["depth_counts"],
                depth_step=float(g["depth_step"]), eps=float(g["eps"]), num_frustum_poses=int(g["num_frustum_poses"]),
                ref_in_frustum=unpack(g["ref_in_frustum"]), ref_observed=unpack(g["ref_observed"]),
                ref_bounds=np.unpackbits(g["ref_bounds"], count=nv).astype(bool), num_poses=npose)
