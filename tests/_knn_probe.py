"""Host side of the exact nearest-neighbour tests (test_knn_probe_cpu.py, test_gpu_knn_exact.py): probe fields, layouts, a
brute-force reference and the near-tie screen.  torch on the CPU and numpy only -- nothing here touches the GPU or the library.

Probe fields.  The last layer of a field is linear with a bias and no activation (oracle.field_mlp).  A field whose weights
and hidden biases are zero and whose last bias is a 4-vector code[f] outputs code[f] at every point, so the public
ops.field_eval_knn returns sum_k w_k code[f_k]: the neighbour SET of every point is visible through the public entry, without a
debug interface.

Set mode.  distance_factor = 0 makes every weight 1 / K.  With integer codes in [0, 4096) per channel, round(K out) is the exact
per-channel sum of the K codes (the fp32 fmaf chain of k_knn_blend stays within 0.012 of it, `emulate_set_blend`), compared with
torch.equal on int64.  Two different sets with the same four sums need a 4096^-4 coincidence.

Reference.  `brute_force`: every centre, fp64 from the fp32 inputs, in chunks; the neighbours of a point are the smallest by
(squared distance, field index) -- numpy.lexsort, no reliance on the tie order of torch.topk.  Written without a look at
oracle.field_set_forward_knn; test_knn_probe_cpu.py holds the two to each other on tie-free inputs.

Near-tie screen.  A point is UNDECIDED when two correct fp32 implementations may disagree on it: the K-th and (K+1)-th exact
squared distances differ by no more than 2^-21 D_{K+1}, or |sqrt(D_1) - radius| <= 2^-21 radius (2^-21: twice the fp32 error
bound of a squared distance, the margin of DESIGN section 4 "Exact nearest point").  Undecided points are left out of the
comparison and their number is bounded (1 % of a case; 0 where the arithmetic is exact).  Where the fp32 arithmetic is exact by
construction (dyadic coordinates) or the tied centres are the same floats, an exact tie is decided by the index rule."""
import numpy as np
import torch

from oracle import ngm_oracle as O

NERF16 = dict(encoding="nerf", num_octaves=2, num_layers=1, dim_hidden=16)     # the smallest compiled network: 276 floats per field
EPS = 2.0 ** -21
CODE_RANGE = 4096
KMAX = 16
OUTSIDE = -1.0            # no sum of codes is negative: an outside point cannot pass for an inside one
COVER = 2.0 / 3 ** 0.5    # spacing of the cover grid in radii (rm.py:299)
RECORDS = []              # one dict per checked case (points, inside share, undecided, ...): written out by the GPU module


# ------------------------------------------------------------------------------------------------ probe fields
def probe_params(fs, NF, codes):
    """all-zero fields whose last bias is `codes` (NF, 4): field f outputs codes[f] everywhere"""
    shapes = fs.param_shapes()
    assert all(n.startswith("_linears.") for n in shapes), "probe fields need an encoding without parameters"
    params = {n: torch.zeros(NF, *s, dtype=torch.float32) for n, s in shapes.items()}
    params[f"_linears.{fs.num_layers}.bias"] = codes.to(torch.float32).reshape(NF, 4).clone()
    return params


def int_codes(NF, seed=0):
    return torch.randint(0, CODE_RANGE, (NF, 4), generator=torch.Generator().manual_seed(1000 + seed))


def real_codes(NF, seed=0):
    return torch.rand(NF, 4, generator=torch.Generator().manual_seed(2000 + seed)) * 2 - 1


def fma32(a, b, c):
    """fp32 fmaf(a, b, c) on numpy arrays: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to
    fp32 (for the set-mode operands -- multiples of 2^-28 below 2^17 -- the fp64 sum is exact, so this IS fmaf)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_blend(w, v):
    """k_knn_blend's chain o = fmaf(w_k, v_k, o), k = 0 .. K-1, from o = 0: w (P, K) fp32, v (P, K, C) fp32 -> (P, C) fp32"""
    w, v = np.asarray(w, np.float32), np.asarray(v, np.float32)
    o = np.zeros((v.shape[0], v.shape[2]), np.float32)
    for k in range(v.shape[1]):
        o = fma32(w[:, k:k + 1], v[:, k], o)
    return o


def emulate_set_blend(K, code_sets):
    """set mode on the host: the weights the assignment computes at distance_factor = 0 (expf(0) / sum of K ones, in fp32) and
    the blend's fmaf chain.  code_sets (P, K, 4) integers -> (P, 4) fp32"""
    w = np.float32(1.0) / np.float32(K)
    return emulate_blend(np.full((code_sets.shape[0], K), w, np.float32), code_sets.astype(np.float32))


def decode_sums(out, K):
    """round(K out) as int64: the per-channel sums of the K codes"""
    return torch.round(float(K) * out.double()).to(torch.int64)


# ------------------------------------------------------------------------------------------------ layouts (all from seeds)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def cover_lattice(NF, seed=0, radius=1.0, noise=0.0, dims=None):
    """NF nodes of the cover grid (spacing 2 r / sqrt 3, fp32 as the map computes it) drawn without replacement from the
    smallest cube (or the box `dims`) that holds them, in shuffled row order; `noise`: sigma of an added normal perturbation"""
    g = _gen(seed)
    if dims is None:
        n = 1
        while n ** 3 < NF:
            n += 1
        dims = (n, n, n)
    ax = [torch.arange(n, dtype=torch.float32) * (radius * COVER) for n in dims]
    nodes = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    pos = nodes[torch.randperm(nodes.shape[0], generator=g)[:NF]].clone()
    if noise:
        pos = pos + noise * torch.randn(NF, 3, generator=g)
    return pos.contiguous()


def points_in_box(pos, P, seed=0, reach=2.0):
    """uniform points in the centres' bounding box grown by `reach` on every side"""
    lo, hi = pos.min(0).values - reach, pos.max(0).values + reach
    return (lo + (hi - lo) * torch.rand(P, 3, generator=_gen(500 + seed))).contiguous()


def points_near(pos, P, seed=0, spread=1.5):
    """points uniform in the cube of half-edge `spread` around randomly chosen centres"""
    g = _gen(600 + seed)
    c = pos[torch.randint(0, pos.shape[0], (P,), generator=g)]
    return (c + (torch.rand(P, 3, generator=g) * 2 - 1) * spread).contiguous()


def two_clusters(seed=0):
    """20 centres in two clusters 500 apart: the grid over them is coarsened to fit its cell budget"""
    g = _gen(seed)
    return torch.cat([torch.rand(10, 3, generator=g) * 3, torch.rand(10, 3, generator=g) * 3 + torch.tensor([500.0, 0.0, 0.0])]).contiguous()


def sparse_box(seed=0):
    """50 centres uniform in a 60^3 box: the K-th neighbour of a point is several rings of (coarsened) cells away"""
    return (torch.rand(50, 3, generator=_gen(seed)) * 60).contiguous()


def dyadic_lattice(spacing, n=4, seed=0):
    """n^3 centres at multiples of `spacing` (a multiple of 1/8), shuffled rows -> (pos, geometric id of every row)"""
    ax = torch.arange(n, dtype=torch.float32) * spacing
    nodes = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    perm = torch.randperm(n ** 3, generator=_gen(seed))
    return nodes[perm].contiguous(), perm


def dyadic_points(spacing, n=4):
    """the half-spacing lattice from one cell outside the centres to one cell outside (vertices, edge midpoints, face and body
    centres of every cell) and a 1/8-step lattice over one interior cell; every coordinate a multiple of 1/8"""
    half = torch.arange(-2, 2 * n + 1, dtype=torch.float32) * (spacing / 2)
    fine = spacing + torch.arange(int(round(spacing * 8)) + 1, dtype=torch.float32) / 8
    pts = torch.cat([torch.cartesian_prod(half, half, half), torch.cartesian_prod(fine, fine, fine)])
    assert bool((pts * 8 == torch.round(pts * 8)).all())
    return pts.contiguous()


def boundary_case(radius):
    """eight centres 8 apart and, per centre and axis direction, a point at exactly `radius` (outside: the test is strict) and one
    at radius - 2^-10 (inside).  Every operation on them is exact in fp32.  -> pos, points, owner (P), expected inside (P)"""
    ax = torch.tensor([0.0, 8.0])
    pos = torch.cartesian_prod(ax, ax, ax)[torch.randperm(8, generator=_gen(8))].contiguous()
    dirs = torch.cat([torch.eye(3), -torch.eye(3)])
    pts, own, ins = [], [], []
    for f in range(8):
        for d in dirs:
            pts += [pos[f] + d * radius, pos[f] + d * (radius - 2.0 ** -10)]
            own += [f, f]
            ins += [False, True]
    pts = torch.stack(pts)
    perm = torch.randperm(pts.shape[0], generator=_gen(9))
    return pos, pts[perm].contiguous(), torch.tensor(own)[perm], torch.tensor(ins)[perm]


def grid_in_lds_bytes(NF):
    """LDS the assignment asks for with the grid resident: histogram (rounded to four entries), centres, cell offsets"""
    max_cells = min(max(8 * NF, 512), 1 << 18)
    return ((NF + 3) & ~3) * 4 + NF * 16 + (max_cells + 1) * 4


def grid_cells(pos, cell=1.1547005):
    """cells of the uniform grid k_knn_grid lays over the centres (its header arithmetic in fp32; `cell`: 1.1547005 field radii,
    the requested edge when no mask radius is given): the length of its first exclusive scan"""
    NF, c = pos.shape[0], np.float32(cell)
    max_cells = min(max(8 * NF, 512), 1 << 18)
    lo, hi = pos.numpy().astype(np.float32).min(0), pos.numpy().astype(np.float32).max(0)
    for _ in range(200):
        n = [int(np.float32(np.float32(hi[d] - lo[d]) / c)) + 1 for d in range(3)]
        if n[0] * n[1] * n[2] <= max_cells and (n[0] + 2) * (n[1] + 2) * (n[2] + 2) <= 4 * max_cells:
            break
        c = np.float32(c * np.float32(1.26))
    return n[0] * n[1] * n[2]


def smallest_nf_beyond(fits):
    nf = 1
    while fits(nf):
        nf += 1
    return nf


# ------------------------------------------------------------------------------------------------ reference
def brute_force(points, pos, kmax=KMAX, chunk=256):
    """-> (idx (P, M) int64, d2 (P, M) fp64), M = min(NF, kmax + 1): every point's M nearest centres ordered by (exact squared
    distance, field index).  fp64 from the fp32 inputs, all centres, `chunk` points at a time"""
    P, NF = points.shape[0], pos.shape[0]
    M = min(NF, kmax + 1)
    p, c = points.double(), pos.double()
    idx = torch.empty(P, M, dtype=torch.int64)
    d2o = torch.empty(P, M, dtype=torch.float64)
    for s in range(0, P, chunk):
        q = p[s:s + chunk]
        n = q.shape[0]
        d2 = (q[:, None, 0] - c[None, :, 0]) ** 2
        d2 += (q[:, None, 1] - c[None, :, 1]) ** 2
        d2 += (q[:, None, 2] - c[None, :, 2]) ** 2
        if M < NF:                                          # only the VALUE of the M-th smallest is taken from kthvalue
            mask = d2 <= torch.kthvalue(d2, M, dim=1).values[:, None]
        else:
            mask = torch.ones_like(d2, dtype=torch.bool)
        rows, cols = mask.nonzero(as_tuple=True)
        d = d2[rows, cols]
        order = torch.from_numpy(np.lexsort((cols.numpy(), d.numpy(), rows.numpy())))       # by row, distance, then index
        rows, cols, d = rows[order], cols[order], d[order]
        cnt = torch.bincount(rows, minlength=n)
        assert int(cnt.min()) >= M
        rank = torch.arange(rows.shape[0]) - (torch.cumsum(cnt, 0) - cnt)[rows]
        keep = rank < M
        idx[s:s + n] = cols[keep].view(n, M)
        d2o[s:s + n] = d[keep].view(n, M)
    return idx, d2o


class Expected:
    """what a correct assignment gives for K neighbours: the set, which points are inside, which are undecided"""

    def __init__(self, ref, K, radius, exact_ties=False, exact_radius=False):
        idx, d2 = ref
        M = idx.shape[1]
        self.K = Ke = min(K, M) if M <= KMAX else K           # (the entry points cap K at the number of fields)
        assert 1 <= Ke <= KMAX and (Ke < M or M <= KMAX)
        self.idx, self.d2 = idx[:, :Ke], d2[:, :Ke]
        d1 = torch.sqrt(d2[:, 0])
        self.inside = d1 < radius
        near_r = torch.zeros_like(self.inside) if exact_radius else (d1 - radius).abs() <= EPS * radius
        dk = d2[:, Ke - 1]
        dk1 = d2[:, Ke] if Ke < M else torch.full_like(dk, float("inf"))
        gap = dk1 - dk
        near_t = torch.isfinite(dk1) & (gap <= EPS * dk1)
        if exact_ties:
            near_t &= gap > 0
        self.tied = self.inside & (gap == 0)                # the index rule decides (or the point is undecided)
        self.undecided = near_r | (self.inside & near_t)
        self.P = idx.shape[0]

    def share(self):
        return float(self.inside.double().mean())


def expect(ref, K, radius=1.0, **kw):
    return Expected(ref, K, radius, **kw)


def softmax_blend64(exp, codes, distance_factor):
    """sum_k softmax(-distance_factor dist)_k codes[idx_k] in fp64 -> (P, 4)"""
    w = torch.softmax(-distance_factor * torch.sqrt(exp.d2), dim=-1)
    return (w[..., None] * codes.double()[exp.idx]).sum(1)


def softmax_blend32(exp, points, pos, codes, distance_factor):
    """the same in fp32 as a plain restatement: torch's fp32 squared distance, sqrt and softmax, the fmaf-order sum"""
    d2 = ((points[:, None, :] - pos[exp.idx]) ** 2).sum(-1)
    w = torch.softmax(-torch.tensor(distance_factor, dtype=torch.float32) * torch.sqrt(d2), dim=-1)
    return torch.from_numpy(emulate_blend(w.numpy(), codes.float()[exp.idx].numpy()))


# ------------------------------------------------------------------------------------------------ checks
def _record(case, exp, **extra):
    rec = dict(case=case, K=exp.K, points=exp.P, inside_share=round(exp.share(), 4), undecided=int(exp.undecided.sum()),
               index_rule_points=int((exp.tied & ~exp.undecided).sum()), **extra)
    RECORDS.append(rec)
    return rec


def check_screen(case, exp, cap=0.01):
    """the condition every case is held to: at most `cap` of its points are undecided"""
    n = int(exp.undecided.sum())
    assert n <= cap * exp.P, f"{case}: {n} of {exp.P} points undecided (cap {cap})"
    return n


def check_set(case, out, exp, codes, points=None, cap=0.01, outside_value=OUTSIDE, NF=None):
    """set mode: `out` (P, 4) of ops.field_eval_knn with integer probe codes, distance_factor 0 -> decided inside points carry
    exactly the sums of their K codes, decided outside points exactly outside_value.  Reports the first mismatch."""
    out = out.detach().cpu()
    check_screen(case, exp, cap)
    dec = ~exp.undecided
    want = codes.to(torch.int64)[exp.idx].sum(1)
    got = decode_sums(out, exp.K)
    is_out = (out == outside_value).all(-1)
    bad_in = dec & exp.inside & ((got != want).any(-1) | is_out)
    bad_out = dec & ~exp.inside & ~is_out
    rec = _record(case, exp, NF=NF if NF is not None else codes.shape[0], wrong_sets=int(bad_in.sum()), wrong_outside=int(bad_out.sum()))
    for bad, what in ((bad_in, "neighbour set"), (bad_out, "outside point")):
        if bool(bad.any()):
            i = int(bad.nonzero()[0])
            raise AssertionError(
                f"{case}: {what} wrong at {int(bad.sum())} of {int(dec.sum())} decided points; first: NF={rec['NF']} K={exp.K} point {i}"
                f"{'' if points is None else ' at ' + str(points[i].tolist())}, expected fields {exp.idx[i].tolist()} "
                f"(squared distances {exp.d2[i].tolist()}) with sums {want[i].tolist()}, returned {out[i].tolist()} "
                f"= sums {got[i].tolist()}, reference inside={bool(exp.inside[i])}")
    return rec


def set_mode_accepts(out, exp, codes, outside_value=OUTSIDE):
    """per point: does the set-mode check accept `out`?  (the host-side mutation test asks this of a swapped neighbour)"""
    want = codes.to(torch.int64)[exp.idx].sum(1)
    ok_in = (decode_sums(out, exp.K) == want).all(-1) & ~(out == outside_value).all(-1)
    return torch.where(exp.inside, ok_in, (out == outside_value).all(-1))


def check_weights(case, out, exp, codes, distance_factor, tol, restated_err, outside_value=OUTSIDE):
    """weights mode: real codes, `out` against the fp64 softmax over the reference's own set; `tol` = 4 x the error of the
    fp32 restatement (`restated_err`).  Decided points only."""
    out = out.detach().cpu()
    check_screen(case, exp)
    dec = ~exp.undecided
    ref = softmax_blend64(exp, codes, distance_factor)
    m = dec & exp.inside
    err = float((out.double() - ref)[m].abs().max())
    _record(case, exp, distance_factor=distance_factor, restated_err=restated_err, kernel_err=err, tol=tol)
    print(f"{case}: fp32 restatement max |err| {restated_err:.3e}, kernel {err:.3e}, allowed {tol:.3e}")
    assert bool((out[dec & ~exp.inside] == outside_value).all())
    assert err <= tol, (case, err, tol)
    return err


def format_records(records=None):
    lines = ["# exact kNN assignment, probe fields (tests/test_gpu_knn_exact.py): per case the number of points, the share inside a field,",
             "# the points the near-tie screen left out, the decided points whose set an exact tie settles by the index rule,",
             "# and for the weights cases the error of the fp32 restatement and of the kernels against the fp64 softmax"]
    for r in (RECORDS if records is None else records):
        head = f"{r['case']:<44} K={r['K']:<2} points={r['points']:<5} inside={r['inside_share']:.4f} undecided={r['undecided']} index_rule={r['index_rule_points']}"
        rest = " ".join(f"{k}={v:.3e}" if isinstance(v, float) else f"{k}={v}" for k, v in r.items()
                        if k not in ("case", "K", "points", "inside_share", "undecided", "index_rule_points"))
        lines.append(head + " " + rest)
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------------------------------------ the oracle's blend on given sets
def oracle_blend_on_sets(points, pos, quat, params, fs, idx, d2, inside, distance_factor=10.0, outside_value=1.0, radius=1.0):
    """oracle.field_set_forward_knn's loop (its own functions, models.py:369-401) on neighbour sets handed in, so that a set
    can be altered: idx / d2 (P, K)"""
    out = torch.full((points.shape[0], fs.dim_out), outside_value, dtype=points.dtype)
    pi, ii = points[inside], idx[inside]
    w = torch.softmax(-distance_factor * torch.sqrt(d2[inside]).to(points.dtype), dim=-1)
    acc = torch.zeros(pi.shape[0], fs.dim_out, dtype=points.dtype)
    for k in range(idx.shape[1]):
        fk = ii[:, k]
        loc = O.scale_local(O.orientation_apply_inverse(quat[fk], pi - pos[fk]), radius, "unit_cube")
        o = O.field_forward_local(loc.unsqueeze(1), {n: v[fk] for n, v in params.items()}, fs).squeeze(1)
        acc = acc + w[:, k:k + 1] * o
    out[inside] = acc
    return out


def unit_quats(NF, seed=0):
    return torch.nn.functional.normalize(torch.randn(NF, 4, generator=_gen(700 + seed)), dim=-1).contiguous()


# the layouts of the GPU file's random cases, by name: (centres, points); the CPU file runs the screen on every one of them
def nf_grid_not_in_lds():
    return smallest_nf_beyond(lambda nf: grid_in_lds_bytes(nf) <= 64 * 1024)


def nf_global_histograms():
    return smallest_nf_beyond(lambda nf: 4 * nf <= 150 * 1024)


def _collinear():
    pos = torch.zeros(40, 3)
    pos[:, 0] = torch.arange(40, dtype=torch.float32) * COVER
    pos[:, 1], pos[:, 2] = 0.37, -1.21
    return pos[torch.randperm(40, generator=_gen(41))].contiguous()


def _coplanar():
    pos = cover_lattice(40, seed=42, dims=(8, 5, 1))
    pos[:, 2] = 2.5
    return pos


def _layout(pos, P, seed, near=None, reach=2.0):
    return pos, (points_near(pos, P, seed, spread=near) if near else points_in_box(pos, P, seed, reach=reach))


_ONE = torch.tensor([[0.3, -0.2, 1.7]])
LAYOUTS = {
    "cover300": lambda: _layout(cover_lattice(300, seed=1), 4096, 1),
    "lds_edge_below": lambda: _layout(cover_lattice(nf_grid_not_in_lds() - 1, seed=2), 2048, 2),
    "grid_not_in_lds": lambda: _layout(cover_lattice(nf_grid_not_in_lds(), seed=3), 4096, 3),
    "near_inline_2048": lambda: _layout(cover_lattice(2048, seed=4), 2048, 4),
    "near_kernels_2049": lambda: _layout(cover_lattice(2049, seed=5), 4096, 5),
    "global_histograms_38401": lambda: _layout(cover_lattice(nf_global_histograms(), seed=6), 4096, 6),
    "scan_round_1025": lambda: _layout(cover_lattice(1025, seed=13, dims=(5, 5, 41)), 2048, 13),
    "clusters20": lambda: _layout(two_clusters(7), 2048, 7, near=1.5),
    "sparse50": lambda: _layout(sparse_box(8), 2048, 8, near=1.0),
    "single_field": lambda: _layout(_ONE.clone(), 512, 9, near=1.5),
    "identical5": lambda: _layout(_ONE.repeat(5, 1).contiguous(), 512, 10, near=1.5),
    "collinear40": lambda: _layout(_collinear(), 2048, 11, reach=1.5),
    "coplanar40": lambda: _layout(_coplanar(), 2048, 12, reach=1.5),
}
# cases whose tied centres are the same floats: an exact tie is settled by the index rule whatever the rounding
EXACT_TIES = {"identical5"}
_CASES = {}


def layout_case(name):
    """(pos, points, brute-force reference to KMAX + 1 neighbours) of a named layout, computed once per process"""
    if name not in _CASES:
        pos, pts = LAYOUTS[name]()
        _CASES[name] = (pos, pts, brute_force(pts, pos))
    return _CASES[name]
