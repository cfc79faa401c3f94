"""fp64 host mirror of mesh alignment (include/ngm_hip.h ngm_mesh_vertex_normals / ngm_icp_point_to_plane; mesh.vertex_normals /
icp_point_to_plane / align_mesh).  TEST INFRASTRUCTURE: the yardstick of tests/test_mesh_align_cpu.py and
tests/test_gpu_mesh_align.py, written to the rules of the header (Open3D is not installed: PARITY UNPINNED against it):
  - vertex normals: fp64 sums of the fp64 face normals of the fp32 vertices, normalised; (0, 0, 1) for a zero sum;
  - ICP: p = R s + t in fp64 with the device's order of operations, the search from the fp32-rounded p (scipy cKDTree in
    fp64; brute force with the smallest index on ties where the target holds exact duplicates), the threshold test in fp64
    from the fp64 p, the 29 sums, Cholesky with the singular rule, U = Rz Ry Rx, T <- U T.
Every per-point term is formed with the device's operations in the device's order (numpy neither fuses nor reorders them), so
a term is bitwise the device's and only the ORDER of the summation differs."""
import numpy as np
from scipy.spatial import cKDTree

STATE_SUMS = slice(20, 49)


# ---- vertex normals ------------------------------------------------------------------------------------------------------
def vertex_normals(verts, faces, return_weight=False):
    """verts (V, 3) float32, faces (F, 3) int64 -> (V, 3) float32 [, (V,) |sum| / sum |terms|: 1 = no cancellation, nan = no term]"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    finite_v = np.isfinite(v).all(1)
    ok = ((f >= 0) & (f < nv)).all(1)
    fi = np.where(ok[:, None], f, 0)
    ok &= finite_v[fi].all(1) if nv else ok
    fi = fi[ok]
    acc = np.zeros((nv, 3))
    length = np.zeros(nv)
    if len(fi):
        a, b = v[fi[:, 1]] - v[fi[:, 0]], v[fi[:, 2]] - v[fi[:, 0]]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        ln = np.sqrt((n * n).sum(1))
        for k in range(3):
            np.add.at(acc, fi[:, k], n)
            np.add.at(length, fi[:, k], ln)
    norm = np.sqrt((acc * acc).sum(1))
    out = np.zeros((nv, 3))
    out[:, 2] = 1.0
    good = (norm > 0) & finite_v
    out[good] = acc[good] / norm[good, None]
    out = out.astype(np.float32)
    if return_weight:
        with np.errstate(invalid="ignore", divide="ignore"):
            return out, norm / length
    return out


# ---- the test scene ------------------------------------------------------------------------------------------------------
def height(x, y):
    return 0.15 * np.sin(3 * x) * np.cos(2 * y) + 0.1 * np.cos(1.7 * x + 0.5) + 0.08 * np.sin(2.3 * y)


def lattice(nx, ny, x0, x1, y0, y1):
    """(nx * ny, 3) float64 vertices of the height field, x fastest, and the (2 (nx - 1)(ny - 1), 3) faces a-b-c / a-c-d"""
    xs, ys = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    v = np.stack([xs.ravel(), ys.ravel(), height(xs, ys).ravel()], 1)
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    a = (j * nx + i).ravel()
    b, c, d = a + 1, a + nx + 1, a + nx
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)
    return v, faces.astype(np.int64)


def rot_zyx(ax, ay, az):
    """Rz(az) Ry(ay) Rx(ax)"""
    ca, sa, cb, sb, cg, sg = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                     [-sb, cb * sa, cb * ca]])


def scene_motion():
    m = np.eye(4)
    m[:3, :3] = rot_zyx(np.deg2rad(1.5), np.deg2rad(-1.0), np.deg2rad(2.0))
    m[:3, 3] = (0.03, -0.02, 0.025)
    return m


def scene(seed):
    """(target verts (1271, 3) f32, target faces (2400, 3) i64, source (2160, 3) f32, the motion (4, 4) f64 the source was moved by)"""
    tv, tf = lattice(41, 31, 0.0, 2.0, 0.0, 1.5)
    sv, _ = lattice(54, 40, 0.3, 2.4, -0.2, 1.3)
    sv = (sv + np.random.default_rng(seed).normal(0, 0.004, sv.shape)).astype(np.float32)
    m = scene_motion()
    moved = (sv.astype(np.float64) @ m[:3, :3].T + m[:3, 3]).astype(np.float32)
    return tv.astype(np.float32), tf, moved, m


def plane_target(n=9):
    """n x n lattice at z = 0 over [0, 1]^2 with normals (0, 0, 1)"""
    xs, ys = np.meshgrid(np.linspace(0, 1, n), np.linspace(0, 1, n))
    t = np.stack([xs.ravel(), ys.ravel(), np.zeros(n * n)], 1).astype(np.float32)
    nrm = np.zeros_like(t)
    nrm[:, 2] = 1
    return t, nrm


# ---- ICP -----------------------------------------------------------------------------------------------------------------
def _nearest(q32, target64, finite_t, has_dup):
    """index into the ORIGINAL target of the nearest finite target of every query (fp64 distances from the fp32-rounded search
    point; smallest index on ties), -1 without a finite target; and the relative gap to the second nearest (inf without one)"""
    ids = np.nonzero(finite_t)[0]
    n = q32.shape[0]
    if len(ids) == 0:
        return np.full(n, -1, np.int64), np.full(n, np.inf)
    q = q32.astype(np.float64)
    t = target64[ids]
    if has_dup or len(ids) < 2:
        best = np.empty(n, np.int64)
        gap = np.full(n, np.inf)
        for s in range(0, n, 4096):
            d = np.sqrt(((q[s:s + 4096, None, :] - t[None]) ** 2).sum(2))
            best[s:s + 4096] = d.argmin(1)                                # the first minimum: the smallest index
        return ids[best], gap
    d, i = cKDTree(t).query(q, k=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(d[:, 1] > 0, (d[:, 1] - d[:, 0]) / d[:, 1], 0.0)
    return ids[i[:, 0]], gap


def icp_pass(source, target, normals, T, threshold, reverse=False):
    """One pass at T: dict(sums (29,), abs (29,) the sums of the terms' magnitudes, count, tie_gap, thr_margin, index (N,) -1 = no
    correspondence).  sums: J^T J upper row by row (21), J^T r (6), sum d^2, count."""
    s = np.asarray(source, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t32 = np.asarray(target, dtype=np.float32).reshape(-1, 3)
    t = t32.astype(np.float64)
    nr = np.asarray(normals, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    n = s.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.stack([((T[r, 0] * s[:, 0] + T[r, 1] * s[:, 1]) + T[r, 2] * s[:, 2]) + T[r, 3] for r in range(3)], 1)
        p32 = p.astype(np.float32)
    live = np.isfinite(s).all(1) & np.isfinite(p32).all(1)
    finite_t = np.isfinite(t).all(1)
    has_dup = len(np.unique(t32[finite_t], axis=0)) < int(finite_t.sum())
    index = np.full(n, -1, np.int64)
    gap = np.full(n, np.inf)
    if live.any():
        index[live], gap[live] = _nearest(p32[live], t, finite_t, has_dup)
    found = index >= 0
    qi = np.where(found, index, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[:, 0] - t[qi, 0], p[:, 1] - t[qi, 1], p[:, 2] - t[qi, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d = np.sqrt(d2)
    near = found & (d < threshold)
    corr = near & np.isfinite(nr[qi]).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        thr_margin = np.min(np.abs(d[found] - threshold) / threshold) if found.any() else np.inf
    tie_gap = np.min(gap[near]) if near.any() else np.inf
    k = np.nonzero(corr)[0]
    if reverse:
        k = k[::-1]
    px, py, pz = p[k, 0], p[k, 1], p[k, 2]
    nx, ny, nz = nr[index[k], 0], nr[index[k], 1], nr[index[k], 2]
    r = (dx[k] * nx + dy[k] * ny) + dz[k] * nz
    J = [py * nz - pz * ny, pz * nx - px * nz, px * ny - py * nx, nx, ny, nz]
    terms = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [d2[k], np.ones(len(k))]
    sums = np.array([np.sum(x) for x in terms])
    mags = np.array([np.sum(np.abs(x)) for x in terms])
    with np.errstate(invalid="ignore"):
        point_margin = np.where(found, np.abs(d - threshold) / threshold, np.inf)        # per source point, for tests that choose points
    point_gap = np.where(near, gap, np.inf)
    index = np.where(corr, index, -1)
    return dict(sums=sums, abs=mags, count=len(k), tie_gap=float(tie_gap), thr_margin=float(thr_margin), index=index,
                point_gap=point_gap, point_margin=point_margin)


def cholesky_solve(up, b):
    """x of A x = b, A given by its 21 upper entries row by row; None where a pivot is not above 1e-12 x the largest diagonal entry
    or the solution is not finite (the singular rule of include/ngm_hip.h)"""
    A = np.zeros((6, 6))
    k = 0
    for r in range(6):
        for c in range(r, 6):
            A[r, c] = A[c, r] = up[k]
            k += 1
    dmax = max(0.0, max(A[r, r] for r in range(6)))
    L = np.zeros((6, 6))
    for j in range(6):
        piv = A[j, j]
        for m in range(j):
            piv -= L[j, m] * L[j, m]
        if not piv > 1e-12 * dmax:
            return None
        l = np.sqrt(piv)
        L[j, j] = l
        for i in range(j + 1, 6):
            s = A[i, j]
            for m in range(j):
                s -= L[i, m] * L[j, m]
            L[i, j] = s / l
    y = np.zeros(6)
    x = np.zeros(6)
    for i in range(6):
        s = b[i]
        for m in range(i):
            s -= L[i, m] * y[m]
        y[i] = s / L[i, i]
    for i in range(5, -1, -1):
        s = y[i]
        for m in range(i + 1, 6):
            s -= L[m, i] * x[m]
        x[i] = s / L[i, i]
    return x if np.isfinite(x).all() else None


def update_matrix(x):
    u = np.eye(4)
    u[:3, :3] = rot_zyx(x[0], x[1], x[2])
    u[:3, 3] = x[3:6]
    return u


def icp(source, target, normals, threshold=0.1, max_iteration=100, init=None, relative_fitness=1e-6, relative_rmse=1e-6, reverse=False):
    """dict(T (4, 4), fitness, rmse, iterations, converged, count, sums, abs, tie_gap, thr_margin -- the two margins the smallest over all
    passes --, passes: the list of every pass's icp_pass record)"""
    T = np.eye(4) if init is None else np.array(init, dtype=np.float64).reshape(4, 4)
    n = np.asarray(source).reshape(-1, 3).shape[0]
    out = dict(T=T, fitness=0.0, rmse=0.0, iterations=0, converged=0, count=0, sums=np.zeros(29), abs=np.zeros(29), tie_gap=np.inf,
               thr_margin=np.inf, passes=[])
    if n == 0:
        return out
    fitness0 = rmse0 = 0.0
    for k in range(max_iteration + 1):
        ps = icp_pass(source, target, normals, T, threshold, reverse=reverse)
        out["passes"].append(ps)
        count = ps["count"]
        fitness = count / n
        rmse = float(np.sqrt(ps["sums"][27] / count)) if count > 0 else 0.0
        out.update(fitness=fitness, rmse=rmse, iterations=k, count=count, sums=ps["sums"], abs=ps["abs"], tie_gap=min(out["tie_gap"], ps["tie_gap"]),
                   thr_margin=min(out["thr_margin"], ps["thr_margin"]))
        if k >= 1 and abs(fitness - fitness0) < relative_fitness and abs(rmse - rmse0) < relative_rmse:
            out["converged"] = 1
            break
        if k == max_iteration:
            break
        fitness0, rmse0 = fitness, rmse
        x = cholesky_solve(ps["sums"][:21], -ps["sums"][21:27]) if count > 0 else None
        if x is not None:
            Tn = T.copy()
            Tn[:3] = update_matrix(x)[:3] @ T
            T = Tn
    out["T"] = T
    return out


def transform(verts, T):
    """mesh.transform_vertices: R v + t in fp64, rounded to fp32"""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    T = np.asarray(T, dtype=np.float64)
    return (((v[:, 0:1] * T[:3, 0] + v[:, 1:2] * T[:3, 1]) + v[:, 2:3] * T[:3, 2]) + T[:3, 3]).astype(np.float32)


def residual_motion(T, motion):
    """(Frobenius norm of R - I, |t|) of T . motion"""
    m = np.asarray(T) @ np.asarray(motion)
    return float(np.linalg.norm(m[:3, :3] - np.eye(3))), float(np.linalg.norm(m[:3, 3]))
