"""Host restatement (numpy) of the single-view training-target sampler on the device (csrc/ngm_target.hip k_tssv_*,
include/ngm_hip.h ngm_target_sample_sv = NeuralGraphMap._sample_target_sv, rm.py:1461-1583): the Philox keys of the three
draws, the k smallest by the kernels' radix select, back-projection, box and segment-sphere tests, the per-ray targets -- in
float32 in the kernels' operation order, and in float64 with the margins the GPU scenes are chosen by.  `compare` is the
comparison the GPU test makes; `fault` plants one-line mistakes that the CPU test shows it catches.  No GPU."""
import numpy as np

from _target_device_host import philox_words
from _target_live_host import _world_to_cam, back_project, k_smallest_radix

STREAM_PIXELS, STREAM_FIELDS, STREAM_RAYS = 0x54470007, 0x54470008, 0x54470009
f32 = np.float32
_LOW = np.uint64(0xFFFFFFFF)
FAULTS = ("hits_gt", "sorted_when_few", "ray_key_no_field", "ray_order_by_pixel", "gt_le_far", "padding_zero")
EXACT = ("pixels", "num_used", "hits", "num_candidates", "subset_fields", "field_ids", "count", "segments", "ijs", "rgb_mask",
         "depth_mask", "term_mask")
FLOATS = ("near", "far", "gt", "rgbds", "term_probs", "c2ws")


def draw_pixels(depth, num_points, seed, iteration):
    """the chosen linear pixel indices, ascending (the device's order is unspecified)"""
    pix = np.nonzero(np.asarray(depth).reshape(-1) != 0)[0].astype(np.uint64)
    keys = (philox_words(seed, iteration, pix, STREAM_PIXELS)[0] << np.uint64(32)) | pix
    return np.sort((k_smallest_radix(keys, num_points) & _LOW).astype(np.int64))


def field_keys(ids, seed, iteration):
    g = np.asarray(ids, dtype=np.uint64)
    return (philox_words(seed, iteration, g, STREAM_FIELDS)[0] << np.uint64(32)) | g


def ray_keys(g, pixels, seed, iteration, with_field=True):
    p = np.asarray(pixels, dtype=np.uint64)
    ctr = (np.uint64(g) << np.uint64(32)) | p if with_field else p
    return (philox_words(seed, iteration, ctr, STREAM_RAYS)[0] << np.uint64(32)) | p


def sample(rgbd, c2w, positions, active, radius, intrinsics, num_points, T, R, seed, iteration, world_size=1, rank=0,
           num_fields=None, capacity=None, dt=f32, draws=None, fault=None):
    """The whole sampler.  rgbd (H, W, 4), c2w (4, 4), positions (NF, 3), active (A,) int; intrinsics (fx, fy, cx, cy) at pixel
    centre 0.  draws: dict with any of pixels / subset_fields / segments (the conventions of ngm_target_sample_sv).  Returns a
    dict keyed like ops.TARGET_SAMPLE_SV_OUT (pixels ascending unless replayed); with dt = float64 also `margins` = (box,
    hit, gt): the smallest relative distance of a box comparison from its bound, of r^2 - d^2 from 0 over the fields in the
    box, of gt - far from 0."""
    assert fault is None or fault in FAULTS
    rgbd = np.asarray(rgbd, dtype=f32)
    H, W = rgbd.shape[:2]
    c2w = np.asarray(c2w, dtype=f32)
    positions = np.asarray(positions, dtype=f32)
    active = np.asarray(active, dtype=np.int64)
    A = len(active)
    nf = len(positions) if num_fields is None else int(num_fields)
    fx, fy, cx, cy = (dt(f32(v)) for v in intrinsics)
    r = dt(f32(radius))
    d = draws or {}
    owned = (nf - rank + world_size - 1) // world_size if nf > rank else 0
    cap = min(T, A, owned) if capacity is None else capacity
    # 1. points
    if d.get("pixels") is not None:
        pixels = np.asarray(d["pixels"], dtype=np.int64)
        pixels = np.where((pixels >= 0) & (pixels < H * W), pixels, -1)
    else:
        pixels = draw_pixels(rgbd[..., 3], num_points, seed, iteration)
        pixels = np.concatenate([pixels, np.full(num_points - len(pixels), -1, np.int64)])
    ok = pixels >= 0
    pix = pixels[ok]
    out = dict(pixels=pixels, num_used=int(ok.sum()), hits=np.zeros(A, np.int32))
    margins = [np.inf, np.inf, np.inf]
    # 2. candidates
    valid = (active >= 0) & (active < nf)
    hit = np.zeros((A, len(pix)), bool)
    c_all = np.zeros((A, 3), dt)
    if len(pix) and valid.any():
        pts = back_project(rgbd, pix, fx, fy, cx, cy, dt)
        lo, hi = pts.min(0), pts.max(0)
        c = _world_to_cam(c2w, positions[active[valid]], dt)
        c_all[valid] = c
        in_box = ((c - r) <= hi[None]).all(-1) & ((c + r) >= lo[None]).all(-1)
        margins[0] = float(np.abs(np.concatenate([hi[None] - (c - r), (c + r) - lo[None]], -1)).min() / r)
        cb = c[in_box]
        sq = (pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]
        sq = np.where(sq == 0, dt(1.0), sq)
        dot = (cb[:, None, 0] * pts[None, :, 0] + cb[:, None, 1] * pts[None, :, 1]) + cb[:, None, 2] * pts[None, :, 2]
        t = np.minimum(np.maximum(dot / sq[None], dt(0.0)), dt(1.0))
        ex, ey, ez = (cb[:, None, k] - pts[None, :, k] * t for k in range(3))
        d2 = (ex * ex + ey * ey) + ez * ez
        if d2.size:
            margins[1] = float(np.abs(r * r - d2).min() / (r * r))
        rows = np.nonzero(valid)[0][in_box]
        hit[rows] = d2 <= r * r
        out["hits"][rows] = hit[rows].sum(-1)
    is_c = (out["hits"] > R) if fault == "hits_gt" else (out["hits"] >= R)
    cand = np.nonzero(is_c)[0]                                    # positions in `active`, its order
    nc = len(cand)
    out["num_candidates"] = nc
    # 3. fields
    sub = np.full(T, -1, np.int64)
    if nc <= T:
        order = np.arange(nc)
        if fault == "sorted_when_few":
            order = np.argsort(field_keys(active[cand], seed, iteration), kind="stable")
        sub[:nc] = order
    elif d.get("subset_fields") is not None:
        s = np.asarray(d["subset_fields"], dtype=np.int64)[:T]
        sub[:len(s)] = np.where((s >= 0) & (s < nc), s, -1)
    else:
        sub[:] = np.argsort(field_keys(active[cand], seed, iteration), kind="stable")[:T]
    out["subset_fields"] = sub
    drawn = active[cand[sub[sub >= 0]]]
    mine = [int(g) for g in drawn if g % world_size == rank][:cap]
    n = len(mine)
    pad_id = 0 if fault == "padding_zero" else -1
    out["count"] = n
    out["field_ids"] = np.array(mine + [pad_id] * (cap - n), dtype=np.int64)
    # 4. rays, 5. targets
    o = dict(segments=np.full((cap, R), -1, np.int64), ijs=np.zeros((cap, R, 2), np.int64), near=np.zeros((cap, R), dt),
             far=np.zeros((cap, R), dt), gt=np.zeros((cap, R), dt), rgbds=np.zeros((cap, R, 4), f32),
             rgb_mask=np.zeros((cap, R), bool), depth_mask=np.zeros((cap, R), bool), term_probs=np.zeros((cap, R), f32),
             term_mask=np.zeros((cap, R), bool), c2ws=np.zeros((cap, R, 4, 4), f32))
    where = {int(g): k for k, g in enumerate(active) if valid[k]}
    flat = rgbd.reshape(-1, 4)
    for row, g in enumerate(mine):
        k = where[g]
        if d.get("segments") is not None:
            p = pixels[np.asarray(d["segments"], dtype=np.int64)[row]]
        else:
            hp = pix[hit[k]]
            keys = ray_keys(g, hp, seed, iteration, with_field=fault != "ray_key_no_field")
            p = (np.sort(k_smallest_radix(keys, R)) & _LOW).astype(np.int64)
            if fault == "ray_order_by_pixel":
                p = np.sort(p)
        i, j = p // W, p % W
        dx, dy = (j.astype(dt) - cx) / fx, (i.astype(dt) - cy) / fy
        nrm = np.maximum(np.sqrt((dx * dx + dy * dy) + dt(1.0)), dt(1e-12))
        gx, gy, gz = dx / nrm, (-dy) / nrm, dt(-1.0) / nrm
        center = (c_all[k, 0] * gx + c_all[k, 1] * gy) + c_all[k, 2] * gz
        near, far = center - r, center + r
        px = flat[p]
        gt = px[:, 3].astype(dt) / (dt(1.0) / nrm)
        dm = (gt <= far) if fault == "gt_le_far" else (gt < far)
        margins[2] = min(margins[2], float((np.abs(gt - far) / np.abs(far)).min()))
        o["segments"][row], o["ijs"][row] = p, np.stack([i, j], -1)
        o["near"][row], o["far"][row], o["gt"][row], o["rgbds"][row] = near, far, gt, px
        o["rgb_mask"][row] = o["depth_mask"][row] = dm
        o["term_probs"][row], o["term_mask"][row], o["c2ws"][row] = dm.astype(f32), True, c2w
    out.update(o)
    if dt is not f32:
        out["margins"] = tuple(margins)
    return out


def compare(got, exp, float_tol=0.0, ordered_pixels=False):
    """What tests/test_gpu_target_sv_device.py asserts of the device's outputs `got` against the mirror's `exp` (dicts of
    numpy arrays / ints): every decision exactly -- `pixels` as a set unless ordered_pixels -- and the floats bit for bit
    (float_tol = 0) or within float_tol.  Each assertion is named by its first word."""
    g = {k: np.asarray(v) for k, v in got.items()}
    e = {k: np.asarray(v) for k, v in exp.items()}
    n = int(e["count"])
    assert int(g["count"]) == n, f"count: {int(g['count'])} != {n}"
    assert np.array_equal(g["field_ids"][n:], np.full(len(g["field_ids"]) - n, -1)), f"padding: field_ids {g['field_ids'][n:]}"
    for k in ("rgb_mask", "depth_mask", "term_mask", "near", "far", "gt", "rgbds", "term_probs", "ijs", "c2ws"):
        assert not g[k][n:].any(), f"padding: {k} not zero past count"
    assert (g["segments"][n:] == -1).all(), "padding: segments not -1 past count"
    for k in EXACT:
        a, b = g[k].reshape(-1) if k in ("count", "num_used", "num_candidates") else g[k], e[k]
        if k == "pixels" and not ordered_pixels:
            a, b = np.sort(a), np.sort(b)
        if k in ("field_ids", "segments", "ijs", "rgb_mask", "depth_mask", "term_mask"):
            a, b = a[:n], b[:n]
        assert np.array_equal(np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)), f"{k}: device and mirror differ"
    for k in FLOATS:
        a, b = g[k][:n].astype(np.float64), e[k][:n].astype(np.float64)
        if float_tol == 0.0:
            assert np.array_equal(a, b), f"{k}: not bit for bit, max |diff| {np.abs(a - b).max() if a.size else 0.0}"
        else:
            assert np.allclose(a, b, rtol=float_tol, atol=float_tol), f"{k}: max |diff| {np.abs(a - b).max()}"


# ---------------------------------------------------------------------------------------------- scenes
# (num_points, active_field_ids, T, R) on the frame and fields of fixture G16; the draw seed -- and for the case that uses every
# valid pixel, where no draw seed moves the points, a seeded jitter of +-5 cm on the field centres -- was searched on the CPU
# for float64 margins above MARGIN (tests/test_target_sv_host_cpu.py asserts them).
MARGIN = 1e-5
_ACT12 = (0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 13)                        # G16's active_field_ids
CASES = {
    "p2000": dict(num_points=2000, active=_ACT12, T=4, R=24, seed=1),
    "p50000_padded": dict(num_points=50000, active=(-1, 99) + _ACT12[2:], T=4, R=24, seed=6),
    "all_pixels": dict(num_points=65536, active=tuple(range(14)), T=16, R=64, seed=1, jitter=1011),
    # field 8 is crossed by exactly R = 56 segments and is a candidate, field 4 by R - 1 = 55 and is none
    "boundary": dict(num_points=2000, active=_ACT12, T=12, R=56, seed=6),
}
BOUNDARY_IN, BOUNDARY_OUT = 8, 4


def g16_scene(jitter=None, frame_seed=None):
    """dict(img (H, W, 4), c2w, positions, radius, intrinsics, g = the fixture) as numpy float32"""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, "golden"))
    import scene
    z = np.load(os.path.join(here, "golden", "g16_target_sampler_sv.npz"))
    pos = z["positions"].astype(f32)
    if jitter is not None:
        pos = (pos + np.random.default_rng(jitter).uniform(-0.05, 0.05, pos.shape)).astype(f32)
    return dict(img=scene.sv_frame(int(z["frame_seed"]) if frame_seed is None else frame_seed).numpy(), c2w=z["c2w"].astype(f32),
                positions=pos, radius=float(z["field_radius"]), intrinsics=(scene.SV_FX, scene.SV_FY, scene.SV_CX, scene.SV_CY),
                g={k: z[k] for k in z.files})


def run_case(name, dt=f32, iteration=0, **kw):
    c = CASES[name]
    s = g16_scene(c.get("jitter"))
    args = dict(world_size=1, rank=0)
    args.update(kw)
    return s, sample(s["img"], s["c2w"], s["positions"], np.array(c["active"]), s["radius"], s["intrinsics"], c["num_points"], c["T"],
                     c["R"], c["seed"], iteration, dt=dt, **args)


def oracle_draws(res, depth):
    """the mirror's draws in the conventions of oracle.ngm_oracle.sample_target_sv(draws=...) (single process)"""
    pixels = np.asarray(res["pixels"])
    pixels = pixels[pixels >= 0]
    valid = np.nonzero(np.asarray(depth).reshape(-1) != 0)[0]
    where = np.full(np.asarray(depth).size, -1, np.int64)
    where[pixels] = np.arange(len(pixels))
    n = int(res["count"])
    sub = np.asarray(res["subset_fields"])
    return dict(subset_points=np.searchsorted(valid, pixels), segments=where[np.asarray(res["segments"])[:n]],
                subset_fields=sub[sub >= 0])
