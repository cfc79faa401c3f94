"""Host yardstick of ngm_cover_depth (include/ngm_hip.h; NeuralGraphMap._extend_global_map_dict, rm.py:265-345).

Three parts, numpy only:

* ``classify``: the rules in float64 on the float32 inputs, with every decision's MARGIN.  The kernel works in float32, so a
  point next to a cell face or next to a field's sphere may legitimately fall on either side.  Rounding budget of the
  float32 path, each rounding at most half an ulp of the largest magnitude M involved (2^-24 M):
      x = ((j - cx) d) / fx                      3 roundings   (y alike, z none)
      p = ((R0 x + R1 y) + R2 z) + t             3 products (the three of a row are not nested: they count once per
                                                 magnitude) + 3 additions, on top of x's 3            -> 9
      u = (p + shift) / cell                     2 roundings                                          -> 11
      |p - c|^2 < r^2                            1 subtraction, then squares and sums relative to r^2 -> 10 + a few 2^-24 r
  Eleven half-ulps are 5.5 * 2^-23 M; the band is 32 * 2^-23 * max(max|p| + cell, r), about sixfold slack (the camera-frame
  intermediates are bounded by |p| + |t|, at most twice max|p| in the scenes used; the slack covers it).  A pixel or centre
  is AMBIGUOUS when a margin is below the band.
* from the classification three sets of cells: REQUIRED (an unambiguous uncovered pixel lies in it and no centre, sure or
  possible, occupies it), OPTIONAL (possible but not required), everything else FORBIDDEN; ``check`` holds a result to them,
  to the ascending (i, j, k) order, to the float32 emit formula bit for bit and to the pixel counts.
* ``cover_fp32``: a float32 restatement of the kernel's arithmetic, with optional single FAULTS -- what the checker is shown to
  reject (tests/test_cover_depth_cpu.py) -- and ``box_scene``, the scenes of the sweep.
"""
import itertools
import math

import numpy as np

F32 = np.float32
BAND_FACTOR = 32.0 * 2.0 ** -23
INDEX_LIMIT = 1 << 20


def cell_of(radius) -> float:
    """(float)(2 r / sqrt 3): formed in double, rounded once"""
    return float(F32(2.0 * float(radius) / math.sqrt(3.0)))


def intrinsics32(K):
    return tuple(float(F32(v)) for v in K)


def world_points(depth, c2w, K, dtype=np.float64, keep_zero=False):
    """valid pixels (finite, != 0, finite world point) -> (pixel indices, world points) in the kernel's order of operations"""
    fx, fy, cx, cy = (dtype(v) for v in intrinsics32(K))
    d = np.asarray(depth, F32)
    H, W = d.shape
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ok = np.isfinite(d) & ((d != 0) | keep_zero)
    i, j, dv = ii[ok].astype(dtype), jj[ok].astype(dtype), d[ok].astype(dtype)
    T = np.asarray(c2w, F32).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (j - cx) * dv / fx
        y = -(i - cy) * dv / fy
        z = -dv
        p = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], -1)
    fin = np.isfinite(p).all(-1)
    return np.flatnonzero(ok.reshape(-1))[fin], p[fin]


def active_rows(positions, field_ids=None, num_active=None):
    if positions is None:
        return np.zeros((0, 3), F32)
    positions = np.asarray(positions, F32).reshape(-1, 3)
    if field_ids is None:
        return positions[:len(positions) if num_active is None else num_active]
    ids = np.asarray(field_ids, np.int64)
    return positions[ids[(ids >= 0) & (ids < len(positions))]]


def _candidates(u, band_u):
    """for every point the cells it may fall into: per axis floor(u), and the neighbour across a face closer than the band"""
    f = np.floor(u)
    lo, hi = (u - f) < band_u, (f + 1 - u) < band_u
    out = []
    for n in range(len(u)):
        axes = [[int(f[n, a])] + ([int(f[n, a]) - 1] if lo[n, a] else []) + ([int(f[n, a]) + 1] if hi[n, a] else []) for a in range(3)]
        out.append(list(itertools.product(*axes)))
    return out


def classify(depth, c2w, K, shift, radius, positions=None, field_ids=None, num_active=None, cell=None):
    """-> dict(required, optional: sets of (i, j, k); valid, uncovered_min, uncovered_max; ambiguous_pixels, ambiguous_centres;
    band, cell, shift).  A cell not in required | optional is forbidden."""
    cell = cell_of(radius) if cell is None else float(cell)
    r = float(F32(radius))
    sh = np.asarray(shift, F32).astype(np.float64)
    _, p = world_points(depth, c2w, K)
    act = active_rows(positions, field_ids, num_active).astype(np.float64)
    act = act[np.isfinite(act).all(-1)]
    mag = max([float(np.abs(p).max()) if len(p) else 0.0, float(np.abs(act).max()) if len(act) else 0.0])
    band = BAND_FACTOR * max(mag + cell, r)
    # coverage
    if len(act) and len(p):
        dist = np.empty((len(p), 2))
        for s in range(0, len(p), 4096):
            dd = np.sqrt(((p[s:s + 4096, None, :] - act[None]) ** 2).sum(-1))
            dist[s:s + 4096, 0] = dd.min(-1)
            dist[s:s + 4096, 1] = np.abs(dd - r).min(-1)
        uncovered, sphere_amb = ~(dist[:, 0] < r), dist[:, 1] < band
    else:
        uncovered, sphere_amb = np.ones(len(p), bool), np.zeros(len(p), bool)
    u = (p + sh) / cell
    f = np.floor(u)
    face = np.minimum(u - f, f + 1 - u).min(-1) * cell if len(p) else np.zeros(0)
    face_amb = face < band
    sure = uncovered & ~sphere_amb & ~face_amb
    maybe = (uncovered | sphere_amb) & ~sure
    wanted_sure = {tuple(int(v) for v in c) for c in f[sure]}
    wanted_maybe = set()
    if maybe.any():
        for cands in _candidates(u[maybe], band / cell):
            wanted_maybe.update(cands)
    # occupancy
    uc = (act + sh) / cell
    fc = np.floor(uc)
    c_amb = (np.minimum(uc - fc, fc + 1 - uc).min(-1) * cell < band) if len(act) else np.zeros(0, bool)
    occ_sure = {tuple(int(v) for v in c) for c in fc[~c_amb]}
    occ_maybe = set()
    if c_amb.any():
        for cands in _candidates(uc[c_amb], band / cell):
            occ_maybe.update(cands)
    occ_maybe -= occ_sure
    required = wanted_sure - occ_sure - occ_maybe
    optional = ((wanted_sure | wanted_maybe) - occ_sure) - required
    return dict(required=required, optional=optional, valid=int(len(p)), uncovered_min=int((uncovered & ~sphere_amb).sum()),
                uncovered_max=int((uncovered | sphere_amb).sum()), ambiguous_pixels=int((sphere_amb | face_amb).sum()),
                ambiguous_centres=int(c_amb.sum()), band=band, cell=cell, shift=np.asarray(shift, F32))


def emit(cells, shift, cell):
    """((ijk - shift) + 0.5) * cell in float32, in that order (rm.py:325)"""
    ijk = np.asarray(cells, np.int64).reshape(-1, 3).astype(F32)
    return ((ijk - np.asarray(shift, F32)) + F32(0.5)) * F32(cell)


def cells_of_positions(pos, shift, cell):
    """the integer cells a result's positions stand for (to the nearest integer; `check` then re-emits them bit for bit)"""
    pos = np.asarray(pos, F32).reshape(-1, 3).astype(np.float64)
    return np.rint(pos / float(cell) - 0.5 + np.asarray(shift, F32).astype(np.float64)).astype(np.int64)


def check(cls, positions, counts):
    """Hold a result (the first num_new rows of new_positions, counts) to the classification.  Raises AssertionError."""
    counts = [int(v) for v in counts]
    positions = np.asarray(positions, F32).reshape(-1, 3)
    assert counts[1] == 0, f"status {counts[1]}"
    assert counts[0] == len(positions), (counts[0], len(positions))
    assert counts[3] == cls["valid"], f"valid pixels {counts[3]} != {cls['valid']}"
    assert cls["uncovered_min"] <= counts[2] <= cls["uncovered_max"], (counts[2], cls["uncovered_min"], cls["uncovered_max"])
    cells = cells_of_positions(positions, cls["shift"], cls["cell"])
    got = [tuple(int(v) for v in c) for c in cells]
    assert len(set(got)) == len(got), "a cell was emitted twice"
    assert got == sorted(got), "cells are not in ascending (i, j, k) order"
    missing = cls["required"] - set(got)
    assert not missing, f"{len(missing)} required cells missing, e.g. {sorted(missing)[:3]}"
    extra = set(got) - cls["required"] - cls["optional"]
    assert not extra, f"{len(extra)} forbidden cells emitted, e.g. {sorted(extra)[:3]}"
    want = emit(cells, cls["shift"], cls["cell"])
    assert positions.tobytes() == want.tobytes(), "positions differ from ((ijk - shift) + 0.5) * cell in float32"


FAULTS = ("truncate", "shift_subtracted", "no_occupied_filter", "all_fields", "unsorted", "cell_rounding", "zero_depth_kept")


def cover_fp32(depth, c2w, K, shift, radius, positions=None, field_ids=None, num_active=None, fault=None):
    """The kernel's arithmetic in float32 (numpy rounds every operation, no fused multiply-add) -> (new_positions, counts).
    fault: None, or one of FAULTS -- a single deliberate mistake."""
    assert fault is None or fault in FAULTS
    cell = F32(cell_of(radius))
    if fault == "cell_rounding":
        cell = F32(2.0) * F32(radius) / F32(math.sqrt(3.0))
        if cell == F32(cell_of(radius)):                    # that form happens to round alike at this radius: one ulp off instead
            cell = np.nextafter(cell, F32(np.inf))
    r2 = F32(radius) * F32(radius)
    sh = np.asarray(shift, F32)
    d = np.asarray(depth, F32)
    _, p = world_points(d, c2w, K, F32, keep_zero=fault == "zero_depth_kept")
    p = p.astype(F32)
    act_all = active_rows(positions, None, None if field_ids is not None else num_active)
    act = act_all if fault == "all_fields" else active_rows(positions, field_ids, num_active)
    if len(act) and len(p):
        unc = np.ones(len(p), bool)
        for s in range(0, len(p), 4096):
            q = p[s:s + 4096, None, :] - act[None]
            d2 = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
            unc[s:s + 4096] = ~(d2 < r2).any(-1)
    else:
        unc = np.ones(len(p), bool)
    snap = np.trunc if fault == "truncate" else np.floor
    cells = lambda v: snap(((v - sh) if fault == "shift_subtracted" else (v + sh)) / cell).astype(np.int64)
    wanted = {tuple(c) for c in cells(p[unc]).tolist()}
    occupied = set() if fault == "no_occupied_filter" or not len(act) else {tuple(c) for c in cells(act[np.isfinite(act).all(-1)]).tolist()}
    new = sorted(wanted - occupied)
    if fault == "unsorted" and len(new) > 1:
        new = new[::-1]
    pos = emit(np.asarray(new, np.int64).reshape(-1, 3), sh, cell)
    status = 2 if any(abs(v) >= INDEX_LIMIT for c in wanted for v in c) else 0
    return pos, [0 if status else len(new), status, int(unc.sum()), int(len(p))]


ROOM = np.array([8.0, 6.0, 3.0])


def box_scene(seed, H=48, W=64, zero_share=0.1, nudge=0):
    """A random camera inside an 8 x 6 x 3 m box room centred on the origin (world points on both sides of it on every axis):
    -> depth (H, W) float32 with a share of pixels zeroed, c2w (4, 4) float32, (fx, fy, cx, cy).  nudge != 0: the camera of
    `seed` moved by up to 0.3 m per axis and turned a little -- a next keyframe that sees much of the same walls."""
    g = np.random.default_rng(seed)
    fx = fy = 55.4 * W / 64
    cx, cy = (W - 1) / 2, (H - 1) / 2
    lo, hi = -ROOM / 2, ROOM / 2
    eye = lo + ROOM * (0.3 + 0.4 * g.random(3))
    q = g.normal(size=4)
    q /= np.linalg.norm(q)
    if nudge:
        g2 = np.random.default_rng(7919 * seed + nudge)
        eye = eye + 0.6 * (g2.random(3) - 0.5)
        q = q + 0.15 * g2.normal(size=4)
        q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    d_cam = np.stack(((jj - cx) / fx, -(ii - cy) / fy, -np.ones((H, W))), -1)        # rays at z-depth 1
    d_w = d_cam @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d_w > 0, (hi - eye) / d_w, (lo - eye) / d_w).min(-1)            # z-depth at the wall
    depth = t.astype(F32)
    depth[g.random((H, W)) < zero_share] = 0.0
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = R, eye
    return depth, c2w.astype(F32), (fx, fy, cx, cy)


def sweep_case(seed, radius, H=48, W=64):
    """A sweep scene: the box scene of `seed`, a field table = the cover of the same view under another shift, every second
    of its fields active.  -> dict(depth, c2w, K, shift, radius, positions, field_ids)"""
    depth, c2w, K = box_scene(seed, H, W)
    cell = cell_of(radius)
    g = np.random.default_rng(1000 + seed)
    shift0, shift = (g.random(3) * cell).astype(F32), (g.random(3) * cell).astype(F32)
    table, _ = cover_fp32(depth, c2w, K, shift0, radius)
    ids = np.arange(0, len(table), 2, dtype=np.int64)
    return dict(depth=depth, c2w=c2w, K=K, shift=shift, radius=radius, positions=table, field_ids=ids)
