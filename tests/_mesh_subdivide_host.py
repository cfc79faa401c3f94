"""Host mirrors of mesh subdivision to a maximum edge length (include/ngm_hip.h ngm_mesh_subdivide_count / _emit;
mesh.subdivide_to_size), numpy fp64.

iterative    trimesh.Trimesh.subdivide_to_size restated from its public definition: every face with an edge longer than max_edge
             is split into four by its (unique) edge midpoints, the faces that are short enough are set aside, and the loop goes
             on with the children.
closed_form  the rule the kernels implement: per input face the level k (halvings of the longest edge until `L > max_edge` is
             false) and the uniform split into 4^k children -- in the kernels' documented vertex and face order, so that an
             indexed mesh comes out that can be compared index by index as well as a triangle soup.

Both take float32 vertices (what the device gets) and work on their float64 copy."""
import numpy as np


def edge_lengths(verts64, faces):
    """(F, 3) fp64: |v1 - v0|, |v2 - v1|, |v0 - v2| as numpy forms them: sqrt((dx*dx + dy*dy) + dz*dz)"""
    d = np.diff(verts64[faces[:, [0, 1, 2, 0]]], axis=1)
    return ((d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]) ** 0.5


def random_mesh(num_faces, seed, lo=0.02, hi=1.5, shuffle=True):
    """faces of very different sizes (log-uniform in [lo, hi]): every even face has three vertices of its own, every odd face
    shares an edge -- two vertices, traversed the other way -- with the face before it and adds an apex at up to four times
    the distance; the vertices are stored in a random order so that no index pattern follows the faces"""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for k in range(num_faces):
        size = np.exp(rng.uniform(np.log(lo), np.log(hi)))
        if k % 2 == 0:
            centre = rng.uniform(-2, 2, 3)
            base = len(verts)
            verts += list(centre + size * rng.normal(size=(3, 3)) / 2)
            faces.append((base, base + 1, base + 2))
        else:
            a, b, c = faces[-1]
            apex = (np.asarray(verts[b]) + np.asarray(verts[c])) / 2 + size * rng.uniform(0.5, 4) * rng.normal(size=3) / 2
            verts.append(apex)
            faces.append((c, b, len(verts) - 1))
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    if shuffle:
        perm = rng.permutation(len(verts))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        verts, faces = verts[perm], inv[faces]
    return verts, faces


def special_faces(max_edge):
    """three faces: a degenerate one (two equal corners); one whose longest edge is EXACTLY max_edge (not split); one whose
    longest edge is exactly 2 max_edge (split once).  max_edge must be a float32 value with a few bits, so that the corners and
    the lengths are exact: the long edge lies along x, the apex is close enough for the other two edges to be shorter."""
    e = float(max_edge)
    assert float(np.float32(e)) == e and float(np.float32(1 + e)) == 1 + e and float(np.float32(2 + 2 * e)) == 2 + 2 * e
    v = np.array([(0, 0, 0), (0, 0, 0), (0.3 * e, 0.2 * e, 0),
                  (1, 1, 1), (1 + e, 1, 1), (1 + 0.5 * e, 1 + 0.3 * e, 1),
                  (2, 2, 2), (2 + 2 * e, 2, 2), (2 + e, 2 + 0.5 * e, 2)], np.float32)
    return v, np.array([(0, 1, 2), (3, 4, 5), (6, 7, 8)], np.int64)


# ------------------------------------------------------------------------------------------------ trimesh's loop
def _subdivide_once(verts, faces):
    """trimesh.remesh.subdivide: one midpoint per UNIQUE edge, four children per face, parent's winding"""
    edges = np.sort(faces[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2), axis=1)
    unique, inverse = np.unique(edges, axis=0, return_inverse=True)
    mid = verts[unique].mean(axis=1)
    m = inverse.reshape(-1, 3) + len(verts)
    f = np.column_stack([faces[:, 0], m[:, 0], m[:, 2], m[:, 0], faces[:, 1], m[:, 1], m[:, 2], m[:, 1], faces[:, 2],
                         m[:, 0], m[:, 1], m[:, 2]]).reshape(-1, 3)
    return np.vstack([verts, mid]), f


def iterative(verts, faces, max_edge, max_iter=10):
    """-> soup (T, 3, 3) fp64, parent (T,) int64.  Raises ValueError("max_iter exceeded") when faces are left that are too long
    after max_iter rounds (a face that needs exactly max_iter rounds is accepted, as the kernels accept it)."""
    cur_v = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    cur_f = np.asarray(faces, np.int64).reshape(-1, 3).copy()
    cur_i = np.arange(len(cur_f))
    done_soup, done_index = [], []
    for it in range(max_iter + 1):
        with np.errstate(all="ignore"):
            too_long = (edge_lengths(cur_v, cur_f) > max_edge).any(axis=1)
        done_soup.append(cur_v[cur_f[~too_long]])
        done_index.append(cur_i[~too_long])
        if not too_long.any():
            break
        if it == max_iter:
            raise ValueError("max_iter exceeded")
        cur_v, cur_f = _subdivide_once(cur_v, cur_f[too_long])
        cur_i = np.repeat(cur_i[too_long], 4)
    return np.concatenate(done_soup), np.concatenate(done_index)


# ------------------------------------------------------------------------------------------------ the closed form
def levels(verts, faces, max_edge, max_iter=10):
    """(F,) int64: the level of every face, max_iter + 1 where more than max_iter halvings are needed (+inf: always).  A NaN
    length makes the longest NaN, which compares false: 0.  A face with an index outside [0, V): 0."""
    v64 = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < len(v64))).all(1) if len(faces) else np.zeros(0, bool)
    k = np.zeros(len(faces), np.int64)
    if not ok.any():
        return k
    with np.errstate(all="ignore"):
        L = edge_lengths(v64, faces[ok]).max(axis=1)                   # np.max: NaN wins
        kk = np.zeros(len(L), np.int64)
        for _ in range(max_iter + 1):
            m = L > max_edge
            kk += m
            L = np.where(m, L * 0.5, L)                                # exact
    k[ok] = kk
    return k


def lattice(n):
    """the lattice of a face split into n segments per edge, in the kernels' order -> (ij (P, 2) of ALL points row by row
    (j = 0 .. n, i = 0 .. n - j), tri (n * n, 3) indices into them: row j, u = 0 .. 2 (n - j) - 2, even u upright, odd u inverted)"""
    jj = np.repeat(np.arange(n + 1), n + 1 - np.arange(n + 1))
    start = np.arange(n + 1) * (2 * n + 3 - np.arange(n + 1)) // 2
    ii = np.arange(len(jj)) - start[jj]
    lin = lambda i, j: j * (2 * n + 3 - j) // 2 + i
    tj = np.repeat(np.arange(n), 2 * (n - np.arange(n)) - 1)
    before = np.arange(n) * (2 * n - np.arange(n))
    u = np.arange(n * n) - before[tj]
    i = u // 2
    up = np.stack([lin(i, tj), lin(i + 1, tj), lin(i, tj + 1)], -1)
    down = np.stack([lin(i + 1, tj), lin(i + 1, tj + 1), lin(i, tj + 1)], -1)
    return np.stack([ii, jj], -1), np.where((u % 2 == 0)[:, None], up, down)


def mix(corner_values, ij, n):
    """(..., 3, C) corner values, lattice coordinates -> (..., P, C) fp64: x0 w0 + x1 w1 + x2 w2, w = ((n - i - j), i, j) / n,
    summed as the kernel sums it ((t0 + t1) + t2; a term of weight 0 is exactly 0 here and changes nothing but a zero's sign)"""
    w = np.stack([n - ij[:, 0] - ij[:, 1], ij[:, 0], ij[:, 1]], -1).astype(np.float64) / n          # (P, 3)
    c = np.asarray(corner_values, np.float64)
    with np.errstate(all="ignore"):
        t = c[..., None, :, :] * w[:, :, None]                                                      # (..., P, 3, C)
        t = np.where(w[:, :, None] == 0, 0.0, t)                                                    # 0 * inf: the term is left out
        return (t[..., 0, :] + t[..., 1, :]) + t[..., 2, :]


def closed_form(verts, faces, max_edge, max_iter=10, attrs=None):
    """-> dict: levels (F,); verts (V + N, 3) fp64 (the V inputs, then every split face's non-corner lattice points, in face
    order), faces (T, 3) int64, parent (T,), soup (T, 3, 3) fp64; vert_parent (N,), vert_ij (N, 2), vert_n (N,): where every new
    vertex comes from; attrs (V + N, C) fp64 when attrs are given.  Raises ValueError("max_iter exceeded") like the device path."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    v64 = v32.astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    a64 = None if attrs is None else np.asarray(attrs, np.float32).astype(np.float64).reshape(len(v32), -1)
    lv = levels(v32, faces, max_edge, max_iter)
    if len(lv) and lv.max() > max_iter:
        raise ValueError("max_iter exceeded")
    n_of = 2 ** lv
    new_count = (n_of + 1) * (n_of + 2) // 2 - 3
    child_count = n_of * n_of
    voff = len(v64) + np.concatenate([[0], np.cumsum(new_count)])
    foff = np.concatenate([[0], np.cumsum(child_count)])
    out_v = np.zeros((voff[-1], 3))
    out_v[:len(v64)] = v64
    out_a = None
    if a64 is not None:
        out_a = np.zeros((voff[-1], a64.shape[1]))
        out_a[:len(a64)] = a64
    out_f = np.zeros((foff[-1], 3), np.int64)
    parent = np.repeat(np.arange(len(faces)), child_count)
    vert_parent = np.repeat(np.arange(len(faces)), new_count)
    vert_ij = np.zeros((voff[-1] - len(v64), 2), np.int64)
    flat = lv == 0
    out_f[foff[:-1][flat]] = faces[flat]
    for k in np.unique(lv[~flat]):
        n = 2 ** int(k)
        ij, tri = lattice(n)
        npts = len(ij)
        inner = np.ones(npts, bool)
        inner[[0, n, npts - 1]] = False
        sel = np.nonzero(lv == k)[0]
        for s0 in range(0, len(sel), 4096):
            fs = sel[s0:s0 + 4096]
            c = faces[fs]
            pts = mix(v64[c], ij[inner], n)                                             # (f, N_k, 3)
            dst = voff[fs][:, None] + np.arange(inner.sum())[None]
            out_v[dst] = pts
            vert_ij[dst - len(v64)] = ij[inner]
            if a64 is not None:
                out_a[dst] = mix(a64[c], ij[inner], n)
            index = np.zeros((len(fs), npts), np.int64)                                 # lattice number -> output vertex index
            index[:, inner] = dst
            index[:, 0], index[:, n], index[:, npts - 1] = c[:, 0], c[:, 1], c[:, 2]
            out_f[foff[fs][:, None] + np.arange(n * n)[None]] = index[:, tri]
    safe = np.where(((out_f >= 0) & (out_f < len(out_v))).all(1)[:, None], out_f, 0)
    res = dict(levels=lv, verts=out_v, faces=out_f, parent=parent, soup=out_v[safe] if len(out_v) else np.zeros((len(out_f), 3, 3)),
               vert_parent=vert_parent, vert_ij=vert_ij, vert_n=n_of[vert_parent])
    if a64 is not None:
        res["attrs"] = out_a
    return res


def canonical(soup, decimals=None, f32_keys=False):
    """a triangle soup (T, 3, 3) in canonical order: the corners of a triangle sorted, then the triangles -> (sorted soup, order:
    the permutation of the triangles).  The sort keys are the coordinates, rounded to `decimals` or to float32 when asked (the
    values themselves are not changed): two soups that agree to rounding then come out in the same order."""
    soup = np.asarray(soup, np.float64).reshape(-1, 3, 3)
    key = soup if decimals is None else np.round(soup, decimals)
    if f32_keys:
        key = soup.astype(np.float32).astype(np.float64)
    key = key + 0.0                                                                     # -0 -> +0
    o = np.lexsort((key[:, :, 2], key[:, :, 1], key[:, :, 0]), axis=1)
    soup = np.take_along_axis(soup, o[:, :, None], 1)
    key = np.take_along_axis(key, o[:, :, None], 1).reshape(len(soup), 9)
    order = np.lexsort(key.T[::-1])
    return soup[order], order
