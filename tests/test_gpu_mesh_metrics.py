"""-m gpu: scoring a mesh on the device (include/ngm_hip.h ngm_surface_sample / ngm_nearest_point; mesh.sample_surface /
nearest_distances / mesh_metrics / evaluate_mesh; NeuralGraphRenderer.evaluate_mesh) against the fp64 host mirror
tests/_mesh_metrics_host.py and the reference's own numbers (fixture G27).

Nearest point: |d - d64| <= 2^-21 d64 -- three products, two sums and a correctly rounded root of rounded fp32 differences stay
within about 4 units of 2^-24 relative, the bar is twice that --, the fp64 distance to the returned index <= (1 + 2^-21) times
the true minimum, d64 == 0 exactly 0.  Sampler: face ids equal to the mirror's except draws within 1e-5 of the total area of
a cumulative-area boundary (at most 1 % of them; tests/test_mesh_metrics_cpu.py holds the mirror to that cap), points within
4 * 2^-24 * the mesh's extent of the mirror's fp64 points."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_metrics_host as MH  # noqa: E402
from gpu_common import DEV, make_renderer, make_target  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2.0 ** -21
GPU_TEST_SEED = 5            # tests/test_mesh_metrics_cpu.py checks the mirror's boundary share for this seed


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ nearest point
def check_nearest(q, r):
    q, r = np.asarray(q, np.float32).reshape(-1, 3), np.asarray(r, np.float32).reshape(-1, 3)
    d_t, i_t = Mh.nearest_distances(dev(q), dev(r))
    assert d_t.dtype == torch.float32 and i_t.dtype == torch.int64 and d_t.shape == (len(q),) and i_t.shape == (len(q),)
    d, i = d_t.cpu().numpy(), i_t.cpu().numpy()
    d64, i64 = MH.nearest(q, r)
    assert np.array_equal(np.isnan(d), np.isnan(d64)) and np.array_equal(np.isposinf(d), np.isposinf(d64))
    ok = np.isfinite(d64)
    assert (i[~ok] == -1).all() and ((i[ok] >= 0) & (i[ok] < len(r))).all()
    err = np.abs(d[ok].astype(np.float64) - d64[ok])
    worst = float((err / np.maximum(d64[ok], 1e-300)).max()) if ok.any() else 0.0
    print(f"nearest point M={len(r)} N={len(q)}: worst |d - d64| / d64 = {worst:.3e} (bar {BAR:.3e})")
    assert (err <= BAR * d64[ok]).all()
    assert (d[ok][d64[ok] == 0] == 0).all()
    assert (MH.distance_to(q[ok], r, i[ok]) <= (1 + BAR) * d64[ok]).all()
    return d, i


def _sizes(M, N):
    rng = np.random.default_rng(1000 * M + N)
    return rng.uniform(-0.2, 1.2, (N, 3)), rng.uniform(0, 1, (M, 3)) * (1.0, 0.7, 0.4)


def _coincident():
    rng = np.random.default_rng(1)
    r = np.tile(np.float32([0.3, -1.0, 2.0]), (200, 1))
    return np.concatenate([rng.uniform(-1, 3, (300, 3)), r[:1]]), r


def _plane():
    rng = np.random.default_rng(2)
    r = rng.uniform(-1, 1, (700, 3)); r[:, 2] = 0.5
    return rng.uniform(-1.5, 1.5, (900, 3)), r


def _line():
    rng = np.random.default_rng(3)
    r = np.zeros((4099, 3)); r[:, 0] = rng.uniform(-3, 3, 4099); r[:, 1] = 0.25; r[:, 2] = -7.0
    q = rng.uniform(-4, 4, (1000, 3)); q[:, 2] -= 7.0
    return q, r


def _ties():
    g = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    r = np.concatenate([g, g, g[::7]])                                     # duplicates
    q = np.concatenate([g[:-1] + 0.5, g + (0.5, 0, 0), g, g + (0, 0.5, 0.5)])   # cell centres (8-way ties), edge / face midpoints, on a point
    return q, r


def _outside():
    rng = np.random.default_rng(4)
    r = rng.uniform(0, 1, (1500, 3))
    base = rng.uniform(0, 1, (40, 3))
    qs = []
    for axes in ((0,), (1,), (2,), (0, 1), (1, 2), (0, 2), (0, 1, 2)):
        for sign in (-1.0, 1.0):
            q = base.copy()
            for a in axes:
                q[:, a] = 0.5 + sign * rng.uniform(3, 100, 40)
            qs.append(q)
    return np.concatenate(qs), r


def _outlier():
    rng = np.random.default_rng(5)
    r = np.concatenate([rng.uniform(0, 0.1, (500, 3)), [[1000.0, 0.05, 0.05]]])
    q = rng.uniform(0, 0.1, (600, 3)); q[:, 0] = rng.uniform(50, 950, 600)          # the empty middle
    return np.concatenate([q, rng.uniform(0, 0.1, (50, 3)), [[999.0, 0, 0]]]), r


def _offset_cloud():
    rng = np.random.default_rng(6)
    g = np.stack(np.meshgrid(*[np.arange(12) * 0.01] * 3, indexing="ij"), -1).reshape(-1, 3)
    c = np.array([1000.0, -2000.0, 500.0])
    return c + rng.uniform(-0.02, 0.14, (2000, 3)), c + g + rng.uniform(-0.002, 0.002, g.shape)


def _nonfinite_refs():
    rng = np.random.default_rng(7)
    r = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    r[5, 0] = np.nan; r[17, 2] = np.inf; r[40] = -np.inf; r[299, 1] = np.nan
    return rng.uniform(-0.5, 1.5, (400, 3)), r


def _nonfinite_queries():
    rng = np.random.default_rng(8)
    q = rng.uniform(-0.5, 1.5, (333, 3)).astype(np.float32)
    q[0, 0] = np.nan; q[64, 1] = np.inf; q[200] = np.nan; q[332, 2] = -np.inf
    return q, rng.uniform(0, 1, (257, 3))


def _no_finite_ref():
    rng = np.random.default_rng(9)
    r = rng.uniform(0, 1, (70, 3)).astype(np.float32)
    r[:, rng.integers(0, 3, 70)[0]] = np.nan
    r[::2, 1] = np.inf
    q = rng.uniform(0, 1, (90, 3)).astype(np.float32); q[3, 0] = np.nan
    return q, r


CASES = {"1x1": lambda: _sizes(1, 1), "1x1000": lambda: _sizes(1, 1000), "63x65": lambda: _sizes(63, 65), "64x64": lambda: _sizes(64, 64),
         "1000x1": lambda: _sizes(1000, 1), "4099x70001": lambda: _sizes(4099, 70001), "coincident": _coincident, "plane": _plane,
         "line": _line, "ties": _ties, "outside": _outside, "outlier": _outlier, "offset_cloud": _offset_cloud,
         "nonfinite_refs": _nonfinite_refs, "nonfinite_queries": _nonfinite_queries, "no_finite_ref": _no_finite_ref}


@pytest.mark.parametrize("name", list(CASES))
def test_nearest_point_against_the_mirror(name):
    q, r = CASES[name]()
    d, i = check_nearest(q, r)
    if name == "no_finite_ref":
        fin = np.isfinite(np.asarray(q, np.float32)).all(1)
        assert np.isposinf(d[fin]).all() and np.isnan(d[~fin]).all() and (i == -1).all()
    if name == "nonfinite_refs":
        assert not np.isin(i, [5, 17, 40, 299]).any()
    if name == "nonfinite_queries":
        assert np.isnan(d[[0, 64, 200, 332]]).all() and (i[[0, 64, 200, 332]] == -1).all() and np.isfinite(np.delete(d, [0, 64, 200, 332])).all()


def test_nearest_point_without_references_is_refused_and_writes_nothing():
    q = torch.rand(8, 3, device=DEV)
    with pytest.raises(K.NgmError) as e:
        Mh.nearest_distances(q, torch.empty(0, 3, device=DEV))
    assert e.value.code == K.NGM_E_INVALID == -1
    dist, index = torch.full((8,), 7.0, device=DEV), torch.full((8,), 7, device=DEV, dtype=torch.int64)
    ws = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    rc = K.lib().ngm_nearest_point(None, 0, q.data_ptr(), 8, dist.data_ptr(), index.data_ptr(), ws.data_ptr(), 4096,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and bool((dist == 7.0).all()) and bool((index == 7).all()) and bool((ws == 0).all())
    d, i = Mh.nearest_distances(torch.empty(0, 3, device=DEV), q)                    # no query: empty outputs, nothing launched
    assert d.shape == (0,) and i.shape == (0,)


@pytest.fixture(scope="module")
def g27():
    return np.load(os.path.join(ROOT, "tests", "golden", "g27_mesh_metrics.npz"))


@pytest.mark.parametrize("pair", [0, 1])
def test_g27_kdtree_distances_and_the_ten_numbers(g27, pair):
    gt, est = g27[f"p{pair}_gt"], g27[f"p{pair}_est"]
    for q, r, key in ((est, gt, "acc_dist"), (gt, est, "comp_dist")):
        d = Mh.nearest_distances(dev(q), dev(r))[0].cpu().numpy().astype(np.float64)
        want = g27[f"p{pair}_{key}"]
        assert (np.abs(d - want) <= BAR * want).all()
    m = Mh.mesh_metrics(dev(gt), dev(est))
    assert tuple(m) == MH.METRIC_KEYS and all(isinstance(v, float) for v in m.values())
    for k, want in zip(MH.METRIC_KEYS, g27[f"p{pair}_metrics"]):
        print(f"G27 pair {pair} {k}: {m[k]:.9f} (reference {float(want):.9f})")
        assert abs(m[k] - float(want)) <= 1e-6, (k, m[k], float(want))


def test_mesh_metrics_median_of_an_even_count_and_zero_ratios():
    """np.median's mean of the two middle values; F1 = 0.0 where a ratio is 0 (the reference divides by zero there)"""
    gt = torch.tensor([[0.0, 0, 0], [10.0, 0, 0]], device=DEV)
    est = torch.tensor([[0.02, 0, 0], [0.03, 0, 0], [10.04, 0, 0], [10.0, 0.06, 0]], device=DEV)
    m = Mh.mesh_metrics(gt, est)
    assert m["median_acc"] == pytest.approx(0.035, abs=2e-6) and m["acc"] == pytest.approx(0.0375, abs=2e-6)      # (fp32 inputs near 10)
    assert m["median_comp"] == pytest.approx(0.03, abs=2e-6)
    assert m["acc_ratio"] == 0.75 and m["acc_ratio_1cm"] == 0.0 and m["comp_ratio"] == 1.0 and m["comp_ratio_1cm"] == 0.0
    assert m["f1_1cm"] == 0.0 and m["f1_5cm"] == pytest.approx(2 / (1 / 1.0 + 1 / 0.75), abs=1e-7)


# ------------------------------------------------------------------------------------------------ sampler
@pytest.fixture(scope="module")
def test_mesh():
    verts, faces, special = MH.sampler_test_mesh()
    fin = verts[np.isfinite(verts).all(1)]
    return verts, faces, special, float((fin.max(0) - fin.min(0)).max())


@pytest.fixture(scope="module")
def mirror_draws(test_mesh):
    verts, faces, _, _ = test_mesh
    return MH.sample_surface(verts, faces, 2 ** 18, GPU_TEST_SEED)           # sample i is a function of (seed, i): prefixes serve every N


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2 ** 18])
def test_sampler_against_the_mirror(test_mesh, mirror_draws, n):
    verts, faces, special, extent = test_mesh
    p_t, f_t = Mh.sample_surface(dev(verts), dev(faces), n, GPU_TEST_SEED)
    assert p_t.shape == (n, 3) and p_t.dtype == torch.float32 and f_t.shape == (n,) and f_t.dtype == torch.int64
    p, f = p_t.cpu().numpy(), f_t.cpu().numpy()
    want_f, want_p, gap = mirror_draws["face_ids"][:n], mirror_draws["points"][:n], mirror_draws["boundary_gap"][:n]
    assert (mirror_draws["area"][f] > 0).all() and not np.isin(f, list(special.values())).any()      # never a face without area
    near = gap <= 1e-5
    share = float(near.mean()) if n else 0.0
    print(f"sampler N={n}: {share:.5f} of the draws within 1e-5 of a cumulative-area boundary (left out of the face comparison)")
    assert share <= 0.01
    assert np.array_equal(f[~near], want_f[~near])
    same = f == want_f
    assert np.abs(p[same].astype(np.float64) - want_p[same]).max(initial=0.0) <= 4 * 2.0 ** -24 * extent
    assert np.isfinite(p).all()


def test_sampler_scan_carries_across_more_than_1024_chunks():
    """2.2 M faces: the scan's middle pass (one workgroup, 1024 chunk sums per round) has to carry into a second round.  With
    that many faces nearly every draw is within 1e-5 of the total of SOME boundary, so the face is checked against the fp64
    running sum itself: the draw u * total must fall into the returned face's interval of it, to 1e-9 of the total (the
    rounding of two differently ordered fp64 sums of 2 M terms is below 1e-10 of it)."""
    n = 1050
    rng = np.random.default_rng(3)
    ax = np.cumsum(rng.uniform(0.01, 1.0, n))                                # spacings 1 : 100, areas 1 : 10^4
    ay = np.cumsum(rng.uniform(0.01, 1.0, n))
    verts = np.stack(np.broadcast_arrays(ax[:, None], ay[None, :], 0.1 * np.sin(ax)[:, None]), -1).reshape(-1, 3).astype(np.float32)
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None]).reshape(-1)
    faces = np.concatenate([np.stack([i, i + n, i + 1], 1), np.stack([i + 1, i + n, i + n + 1], 1)]).astype(np.int64)
    faces = faces[rng.permutation(len(faces))]
    faces[::97, 2] = faces[::97, 1]                                          # faces without area among them
    assert len(faces) > 1024 * 2048
    N = 4096
    p_t, f_t = Mh.sample_surface(dev(verts), dev(faces), N, 9)
    p, f = p_t.cpu().numpy().astype(np.float64), f_t.cpu().numpy()
    m = MH.sample_surface(verts, faces, N, 9)
    cum, tot = m["cum"], m["total"]
    assert (f >= 0).all() and (m["area"][f] > 0).all()
    lower = np.where(f > 0, cum[np.maximum(f - 1, 0)], 0.0)
    assert (m["target"] >= lower - 1e-9 * tot).all() and (m["target"] <= cum[f] + 1e-9 * tot).all()
    print(f"sampler, {len(faces)} faces: {float((f == m['face_ids']).mean()):.4f} of the face ids equal to the mirror's")
    c = verts[faces[f]].astype(np.float64)
    u, v = m["uv"][:, 0].astype(np.float64)[:, None], m["uv"][:, 1].astype(np.float64)[:, None]
    want = c[:, 0] + u * (c[:, 1] - c[:, 0]) + v * (c[:, 2] - c[:, 0])
    assert np.abs(p - want).max() <= 4 * 2.0 ** -24 * float((verts.max(0) - verts.min(0)).max())


def test_sampler_is_repeatable_seeded_and_stream_independent(test_mesh):
    verts, faces, _, _ = test_mesh
    v, f = dev(verts), dev(faces)
    a = Mh.sample_surface(v, f, 5000, 11)
    b = Mh.sample_surface(v, f, 5000, 11)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = Mh.sample_surface(v, f, 5000, 11)
    side.synchronize()
    for o in (b, c):
        assert torch.equal(a[0].view(torch.int32), o[0].view(torch.int32)) and torch.equal(a[1], o[1])
    d = Mh.sample_surface(v, f, 5000, 12)
    assert not torch.equal(a[0], d[0]) and not torch.equal(a[1], d[1])
    assert torch.equal(a[0][:100], Mh.sample_surface(v, f, 100, 11)[0])


def test_sampler_single_face_degenerate_meshes_and_no_faces(test_mesh):
    verts, faces, special, extent = test_mesh
    tri = np.float32([[0, 0, 0], [2, 0, 0], [0, 3, 0]])
    p, f = Mh.sample_surface(dev(tri), dev(np.int64([[0, 1, 2]])), 4096, 3)
    p = p.cpu().numpy().astype(np.float64)
    assert bool((f == 0).all()) and (p[:, 2] == 0).all() and p.min() >= 0 and (p[:, 0] / 2 + p[:, 1] / 3).max() <= 1 + 1e-6
    assert abs(p[:, 0].mean() - 2 / 3) < 0.03 and abs(p[:, 1].mean() - 1.0) < 0.04           # the centroid: uniform in the face
    m = MH.sample_surface(tri, np.int64([[0, 1, 2]]), 4096, 3)
    assert np.abs(p - m["points"]).max() <= 4 * 2.0 ** -24 * 3
    p, f = Mh.sample_surface(dev(verts), dev(faces[list(special.values())]), 70, 3)        # nothing but faces without area
    assert bool(torch.isnan(p).all()) and bool((f == -1).all())
    with pytest.raises(K.NgmError) as e:
        Mh.sample_surface(dev(verts), torch.empty(0, 3, device=DEV, dtype=torch.int64), 10)
    assert e.value.code == K.NGM_E_INVALID
    pts, ids = torch.full((10, 3), 7.0, device=DEV), torch.full((10,), 7, device=DEV, dtype=torch.int64)
    ws = torch.zeros(4096, device=DEV, dtype=torch.uint8)
    rc = K.lib().ngm_surface_sample(dev(verts).data_ptr(), len(verts), None, 0, 10, 0, pts.data_ptr(), ids.data_ptr(), ws.data_ptr(),
                                    4096, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == K.NGM_E_INVALID and bool((pts == 7.0).all()) and bool((ids == 7).all())


# ------------------------------------------------------------------------------------------------ end to end
def uv_sphere(radius, centre=(0.0, 0.0, 0.0), n_lat=48, n_lon=96):
    """Triangulated sphere: n_lat bands x n_lon sectors, vertices ON the sphere.  48 x 96: an edge spans pi / 48 of a great
    circle at most, its sagitta is r (1 - cos(pi / 96)) = 0.32 mm at r = 0.6; a triangle's interior is at most about twice
    that inside the sphere."""
    th = torch.linspace(0, np.pi, n_lat + 1, dtype=torch.float64)
    ph = torch.arange(n_lon, dtype=torch.float64) * (2 * np.pi / n_lon)
    v = torch.stack([torch.sin(th)[:, None] * torch.cos(ph)[None], torch.sin(th)[:, None] * torch.sin(ph)[None],
                     torch.cos(th)[:, None].expand(-1, n_lon)], -1).reshape(-1, 3)
    i = torch.arange(n_lat)[:, None] * n_lon
    j = torch.arange(n_lon)[None]
    a, b = i + j, i + (j + 1) % n_lon
    f = torch.cat([torch.stack([a, a + n_lon, b], -1).reshape(-1, 3), torch.stack([b, a + n_lon, b + n_lon], -1).reshape(-1, 3)])
    verts = (radius * v + torch.tensor(centre, dtype=torch.float64)).float()
    return verts.to(DEV), f.to(torch.int64).to(DEV)                    # (the pole bands hold faces of zero area: never drawn)


def test_evaluate_mesh_two_concentric_spheres(tmp_path):
    """radius 0.6 against 0.62: every distance is the radial offset of 2 cm, plus the lateral distance to the nearest of 20 000
    samples over 4.5 m^2 (a few millimetres) and the tessellation's sagitta (0.3 - 0.7 mm)"""
    est, gt = uv_sphere(0.62), uv_sphere(0.6)
    m = Mh.evaluate_mesh(est, gt, num_points=20000, seed=0)
    print("concentric spheres:", {k: round(v, 5) for k, v in m.items()})
    assert tuple(m) == MH.METRIC_KEYS
    assert abs(m["acc"] - 0.02) <= 0.003 and abs(m["comp"] - 0.02) <= 0.003
    assert m["acc_ratio"] == 1.0 and m["comp_ratio"] == 1.0
    assert m["acc_ratio_1cm"] == 0.0 and m["comp_ratio_1cm"] == 0.0 and m["f1_1cm"] == 0.0 and m["f1_5cm"] == 1.0
    # PLY paths (files save_ply wrote) give the same numbers as the tensors; est is drawn with seed, gt with seed + 1
    Mh.save_ply(tmp_path / "est.ply", *est)
    Mh.save_ply(tmp_path / "gt.ply", *gt)
    assert Mh.evaluate_mesh(str(tmp_path / "est.ply"), tmp_path / "gt.ply", num_points=20000, seed=0) == m
    ep, gp = Mh.sample_surface(*est, 20000, 0)[0], Mh.sample_surface(*gt, 20000, 1)[0]
    assert Mh.mesh_metrics(gp, ep) == m


# ------------------------------------------------------------------------------------------------ memory safety
GUARD, PATTERN = 4096, 0xA5


@contextmanager
def guard_bands():
    """tests/test_gpu_safety.py's guard bands, restated for the allocations of the two ops (torch.empty with dtype and device):
    4 KiB of pattern on either side of every output and workspace, checked after a device synchronisation"""
    real = torch.empty
    raws = []

    def empty(*shape, dtype=None, device=None, **kw):
        if device is None or torch.device(device).type != "cuda" or kw:
            return real(*shape, dtype=dtype, device=device, **kw)
        shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)) else shape
        dtype = dtype or torch.get_default_dtype()
        nbytes = int(np.prod(shape, dtype=np.int64)) * real((), dtype=dtype).element_size()
        raw = real(GUARD + nbytes + (-nbytes) % 256 + GUARD, dtype=torch.uint8, device=device)
        raw.fill_(PATTERN)
        raws.append((raw, nbytes))
        return raw[GUARD:GUARD + nbytes].view(dtype).view(*shape)

    torch.empty = empty
    try:
        yield raws
    finally:
        torch.empty = real
    torch.cuda.synchronize()
    assert raws
    for raw, nbytes in raws:
        assert bool((raw[:GUARD] == PATTERN).all()) and bool((raw[GUARD + nbytes:] == PATTERN).all()), nbytes


def test_guard_bands_around_outputs_and_workspaces(test_mesh):
    verts, faces, _, _ = test_mesh
    v, f = dev(verts), dev(faces)
    with guard_bands() as raws:
        for n in (1, 63, 257, 5000):
            Mh.sample_surface(v, f, n, 1)
        Mh.sample_surface(*uv_sphere(1.0, n_lat=33, n_lon=63), 1000, 2)         # 4158 faces: three chunks of the scan
        Mh.sample_surface(*uv_sphere(1.0, n_lat=32, n_lon=32), 1000, 3)         # 2048 faces: exactly one chunk, stored as vectors
        for name in ("1x1", "63x65", "64x64", "1000x1", "line", "outlier", "nonfinite_refs", "no_finite_ref", "coincident"):
            q, r = CASES[name]()
            Mh.nearest_distances(dev(np.asarray(q, np.float32)), dev(np.asarray(r, np.float32)))
    assert len(raws) >= 3 * 6 + 3 * 9


# ------------------------------------------------------------------------------------------------ dispatcher and renderer
def test_ops_fake_shapes_and_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        v, f = torch.empty(50, 3, device=DEV), torch.empty(20, 3, dtype=torch.int64, device=DEV)
        p, ids = torch.ops.ngm355.surface_sample(v, f, 77, 3)
        assert p.shape == (77, 3) and p.dtype == torch.float32 and ids.shape == (77,) and ids.dtype == torch.int64
        d, i = torch.ops.ngm355.nearest_point(torch.empty(31, 3, device=DEV), v)
        assert d.shape == (31,) and d.dtype == torch.float32 and i.shape == (31,) and i.dtype == torch.int64
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        Mh.sample_surface(v, f, 4)
    with pytest.raises(RuntimeError):
        Mh.nearest_distances(v, v)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.ngm355.nearest_point(v, v)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.ngm355.surface_sample(v, f, 4, 0)


def test_renderer_evaluate_mesh_of_a_trained_field():
    """the trained sphere scene of tests/test_gpu_mesh.py (one field, resolution 0.04) scored against the analytic sphere"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from scene import sphere_scene_batch
    F, R = 1, 512
    r = make_renderer(dict(encoding="fourier", dim_enc=64, num_layers=2),
                      dict(num_samples_coarse=16, num_samples_depth_guided=16, termination_weight=0.5), F)
    pos = torch.tensor([[0.3, -0.2, 0.1]])
    r.set_field_poses(pos.to(DEV), torch.tensor([[1.0, 0, 0, 0]], device=DEV))
    for it in range(400):
        t = sphere_scene_batch(F, R, pos, 1000 + it)
        r.optimization_iteration(make_target(t, torch.arange(F)), seed=it, update=True)
    gt = uv_sphere(0.6, centre=tuple(pos[0].tolist()))
    m = r.evaluate_mesh(gt, num_points=20000, seed=0, resolution=0.04)
    print("trained sphere:", {k: round(v, 5) for k, v in m.items()})
    assert tuple(m) == MH.METRIC_KEYS and all(np.isfinite(v) for v in m.values())
    assert m["acc"] < 0.02
    assert r.evaluate_mesh(gt, num_points=1000, resolution=0.2, threshold=1e9) is None      # where extract_mesh returns None
