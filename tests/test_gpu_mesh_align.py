"""-m gpu: aligning a mesh on the device (include/ngm_hip.h ngm_mesh_vertex_normals / ngm_icp_point_to_plane; mesh.vertex_normals /
icp_point_to_plane / align_mesh / evaluate_raw_mesh(align="icp")) against the fp64 host mirror tests/_mesh_align_host.py.  The
conditions under which the device must pick the mirror's correspondences (tie and threshold margins) are asserted for the seeds
used here by tests/test_mesh_align_cpu.py; cases built here assert them before they compare."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_align_host as AH  # noqa: E402
import _mesh_cull_host as CH  # noqa: E402
from gpu_common import DEV  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd.renderer import Camera  # noqa: E402
from test_mesh_align_cpu import SEEDS, THRESHOLD_BAR, TIE_BAR  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD, PATTERN = 4096, 0xA5
NORMAL_BAR = 4 * 2.0 ** -24              # the sum is exact to 2^-40, the normalisation is fp64: one rounding to fp32 and a little
T_BAR = 1e-12                            # >= 100 x the summation floor the CPU test asserts (1e-14)
ICP_GRID = 1024 * 256                    # threads of the FIXED accumulate grid (1024 workgroups of 256): 300 000 points take two trips
INIT = AH.update_matrix([-0.02, 0.015, -0.03, -0.02, 0.02, -0.02])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ raw calls inside guard bands
class Banded:
    """`nbytes` of device memory between two bands of 4096 pattern bytes; fill: the byte the payload starts with"""

    def __init__(self, nbytes, fill=0):
        self.nbytes = int(nbytes)
        self.raw = torch.full((GUARD + self.nbytes + (-self.nbytes) % 256 + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.raw[GUARD:GUARD + self.nbytes] = fill
        self.ptr = self.raw.data_ptr() + GUARD

    def payload(self, dtype):
        return self.raw[GUARD:GUARD + self.nbytes].view(dtype)

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[GUARD + self.nbytes:] == PATTERN).all()), self.nbytes


def c_normals(verts, faces):
    """ngm_mesh_vertex_normals through the C ABI, output and workspace inside guard bands -> (V, 3) float32"""
    v, f = dev(np.asarray(verts, np.float32).reshape(-1, 3)), dev(np.asarray(faces, np.int64).reshape(-1, 3))
    L = K.lib()
    wsb = L.ngm_mesh_vertex_normals_workspace(len(v))
    out, ws = Banded(12 * len(v), PATTERN), Banded(wsb, PATTERN)
    K.check(L.ngm_mesh_vertex_normals(v.data_ptr(), len(v), f.data_ptr(), len(f), out.ptr, ws.ptr, wsb, ops._stream()), "normals")
    out.check()
    ws.check()
    return out.payload(torch.float32).view(-1, 3).cpu().numpy()


def c_icp(source, target, normals, threshold=0.1, max_iteration=100, init=None, rf=1e-6, rr=1e-6, calls=1):
    """ngm_icp_point_to_plane through the C ABI, state and a workspace PRE-FILLED with 0xA5 inside guard bands -> the states (64,) of
    `calls` calls on the same workspace"""
    s, t, n = (dev(np.asarray(a, np.float32).reshape(-1, 3)) for a in (source, target, normals))
    L = K.lib()
    wsb = L.ngm_icp_point_to_plane_workspace(len(t), len(s))
    ws = Banded(wsb, PATTERN)
    init_c = None if init is None else (C.c_double * 16)(*np.asarray(init, np.float64).ravel())
    states = []
    for _ in range(calls):
        state = Banded(64 * 8, PATTERN)
        K.check(L.ngm_icp_point_to_plane(s.data_ptr(), len(s), t.data_ptr(), n.data_ptr(), len(t), threshold, max_iteration, rf, rr, init_c,
                                         state.ptr, ws.ptr, wsb, ops._stream()), "icp")
        state.check()
        ws.check()
        states.append(state.payload(torch.float64).cpu().numpy())
    return states[0] if calls == 1 else states


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for seed in SEEDS:
        tv, tf, src, motion = AH.scene(seed)
        out[seed] = dict(tv=tv, tf=tf, src=src, motion=motion, nrm=AH.vertex_normals(tv, tf))
    return out


# ------------------------------------------------------------------------------------------------ 1. vertex normals
def fan(n):
    """n faces round vertex 0, the rim at varying heights and radii"""
    a = np.arange(n) * (2 * np.pi / n)
    rim = np.stack([(1 + 0.3 * np.sin(5 * a)) * np.cos(a), (1 + 0.3 * np.sin(5 * a)) * np.sin(a), 0.4 * np.cos(3 * a)], 1)
    v = np.concatenate([[(0.0, 0.0, 0.2)], rim]).astype(np.float32)
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int64)


def normal_meshes(scenes):
    big_v, big_f = AH.lattice(200, 166, 0.0, 3.0, 0.0, 2.5)
    s = scenes[SEEDS[0]]
    return {"scene": (s["tv"], s["tf"]), "triangle": (np.float32([(0, 0, 0), (1, 0, 0.5), (0.2, 1, 0)]), np.int64([(0, 1, 2)])),
            "fan4096": fan(4096), "faces65537": (big_v.astype(np.float32), big_f[:65537])}


@pytest.mark.parametrize("name", ["scene", "triangle", "fan4096", "faces65537"])
def test_normals_against_the_mirror(scenes, name):
    v, f = normal_meshes(scenes)[name]
    want, weight = AH.vertex_normals(v, f, return_weight=True)
    got = c_normals(v, f)
    check = ~(weight < 1e-3)                               # a vertex without a face (nan) is checked: (0, 0, 1)
    left_out = 1.0 - check.mean()
    err = np.abs(got[check].astype(np.float64) - want[check]).max()
    print(f"{name}: V {len(v)} F {len(f)}, left out {100 * left_out:.3f} % (cap 1 %), worst |dn| {err:.3e} (bar {NORMAL_BAR:.3e})")
    assert left_out <= 0.01
    assert err <= NORMAL_BAR
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() <= 2.0 ** -22
    # the public function gives the same bits, and so do shuffled faces and a second call
    pub = Mh.vertex_normals(dev(v), dev(f))
    assert pub.dtype == torch.float32 and np.array_equal(pub.cpu().numpy(), got)
    perm = np.random.default_rng(3).permutation(len(f))
    assert np.array_equal(c_normals(v, f[perm]), got) and np.array_equal(c_normals(v, f[perm[::-1]]), got)


def test_normals_special_cases():
    up = np.float32([0, 0, 1])
    v = np.array([(0, 0, 0), (4, 0, 0), (0, 4, 0), (5, 5, 5), (np.nan, 0, 0), (1, 1, 3)], np.float32)
    # two opposite faces at integer coordinates: exact cancellation; vertex 3 is unreferenced, 4 is not finite
    assert np.array_equal(c_normals(v, np.int64([(0, 1, 2), (0, 2, 1)])), np.tile(up, (6, 1)))
    # an out-of-range index and a non-finite vertex: those faces add nothing, the one good face decides
    got = c_normals(v, np.int64([(0, 2, 1), (0, 1, 7), (0, 1, 4), (-1, 1, 2), (2 ** 40, 1, 2)]))
    assert np.array_equal(got[:3], np.tile(np.float32([0, 0, -1]), (3, 1))) and np.array_equal(got[3:], np.tile(up, (3, 1)))
    # a degenerate face adds zero, a huge and a tiny face at one vertex keep their ratio
    w = np.array([(0, 0, 0), (1e18, 0, 0), (0, 1e18, 0), (0, 1e-18, 0), (0, 0, 1e-18), (2, 2, 2)], np.float32)
    faces = np.int64([(0, 1, 2), (0, 3, 4), (0, 5, 5)])
    got, want = c_normals(w, faces), AH.vertex_normals(w, faces)
    assert np.abs(got.astype(np.float64) - want).max() <= NORMAL_BAR and np.array_equal(got[3], np.float32([1, 0, 0]))
    assert c_normals(v, np.zeros((0, 3), np.int64)).tolist() == np.tile(up, (6, 1)).tolist()
    assert Mh.vertex_normals(dev(np.zeros((0, 3), np.float32)), dev(np.zeros((0, 3), np.int64))).shape == (0, 3)


# ------------------------------------------------------------------------------------------------ 2. one pass
def subset(n, k):
    return (np.arange(k) * n) // k + n // (2 * k)


def check_sums(state, mirror, n, label):
    sums, mags = mirror["sums"], mirror["abs"]
    got = state[AH.STATE_SUMS]
    assert got[28] == mirror["count"] and state[16] == mirror["count"] / n, (label, got[28], mirror["count"])
    bound = 2 * n * 2.0 ** -53 * mags
    err = np.abs(got - sums)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    assert (err <= bound).all(), (label, err, bound)
    return worst


@pytest.mark.parametrize("init", [None, INIT], ids=["identity", "moved"])
def test_one_pass_sums_against_the_mirror(scenes, init):
    s = scenes[SEEDS[0]]
    T = np.eye(4) if init is None else init
    worst, counts = 0.0, []
    for m in (1, 3, 130, 1271):
        ti = subset(1271, m)
        tgt, nrm = s["tv"][ti], s["nrm"][ti]
        for n in (1, 63, 65, 257, 2160):
            src = s["src"][subset(2160, n)]
            if m == 1:
                src = (src * np.float32(0.06) + tgt[0]).astype(np.float32)                # around the one target: some inside, some not
            mirror = AH.icp_pass(src, tgt, nrm, T, 0.1)
            assert mirror["tie_gap"] >= TIE_BAR and mirror["thr_margin"] >= THRESHOLD_BAR, (m, n, mirror["tie_gap"], mirror["thr_margin"])
            state = c_icp(src, tgt, nrm, max_iteration=0, init=init)
            assert np.array_equal(state[:16], T.ravel()) and state[18] == 0 and state[19] == 0 and not state[50:].any()
            worst = max(worst, check_sums(state, mirror, n, (m, n)))
            counts.append(mirror["count"])
    print(f"one pass: correspondences per case {counts}, worst error / bound {worst:.3f}")
    assert sum(c > 0 for c in counts) >= 14 and any(c == 0 for c in counts)


def test_one_pass_over_more_points_than_the_fixed_grid_has_threads(scenes):
    s = scenes[SEEDS[0]]
    n = 300_000
    assert n > ICP_GRID
    rng = np.random.default_rng(11)
    lo, hi = s["tv"].min(0), s["tv"].max(0)
    pts = rng.uniform(lo, hi, (n + 2000, 3)).astype(np.float32)
    # random points land within rounding of a tie or of the threshold now and then: those are left out (a few per 100 000), the rest
    # keeps the margins the comparison rests on
    probe = AH.icp_pass(pts, s["tv"], s["nrm"], np.eye(4), 0.1)
    ok = (probe["point_gap"] >= 4 * TIE_BAR) & (probe["point_margin"] >= 4 * THRESHOLD_BAR)
    print(f"{(~ok).sum()} of {len(pts)} random points left out for a margin")
    assert (~ok).sum() < 200
    pts = pts[ok][:n]
    assert len(pts) == n
    mirror = AH.icp_pass(pts, s["tv"], s["nrm"], np.eye(4), 0.1)
    assert mirror["tie_gap"] >= TIE_BAR and mirror["thr_margin"] >= THRESHOLD_BAR and 0.2 * n < mirror["count"] < 0.9 * n
    a, b = c_icp(pts, s["tv"], s["nrm"], max_iteration=0, calls=2)                        # the workspace starts as 0xA5 bytes; two calls on it
    assert np.array_equal(a, b)
    print(f"N = {n}: {mirror['count']} correspondences, worst error / bound {check_sums(a, mirror, n, 'large'):.3f}")


def test_prefilled_workspace_and_public_function_give_the_same_bits(scenes):
    s = scenes[SEEDS[1]]
    a, b = c_icp(s["src"], s["tv"], s["nrm"], max_iteration=0, init=INIT, calls=2)
    pub = Mh.icp_point_to_plane(dev(s["src"]), dev(s["tv"]), dev(s["nrm"]), max_iteration=0, init=INIT)
    assert np.array_equal(a, b) and np.array_equal(a, pub.state.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 3. the whole run
@pytest.mark.parametrize("seed", SEEDS)
def test_whole_run_against_the_mirror(scenes, seed):
    s = scenes[seed]
    want = AH.icp(s["src"], s["tv"], s["nrm"])
    res = Mh.icp_point_to_plane(dev(s["src"]), dev(s["tv"]), dev(s["nrm"]))
    assert res.transformation.dtype == torch.float64 and tuple(res.transformation.shape) == (4, 4) and res.transformation.is_cuda
    assert res.iterations.dtype == torch.int64 and res.converged.dtype == torch.bool and res.fitness.is_cuda and res.inlier_rmse.is_cuda
    T = res.transformation.cpu().numpy()
    dT, dr = np.abs(T - want["T"]).max(), abs(float(res.inlier_rmse) - want["rmse"])
    print(f"seed {seed}: iterations {int(res.iterations)} converged {bool(res.converged)} fitness {float(res.fitness):.6f}; worst |dT| {dT:.3e}, "
          f"|drmse| {dr:.3e} (bar {T_BAR:.0e}); residual motion {AH.residual_motion(T, s['motion'])}")
    assert int(res.iterations) == want["iterations"] and int(res.converged) == want["converged"] == 1
    assert float(res.fitness) == want["fitness"]
    assert dT <= T_BAR and dr <= T_BAR
    again = c_icp(s["src"], s["tv"], s["nrm"])
    assert np.array_equal(again, res.state.cpu().numpy())                                # all 64 doubles, bit for bit
    check_sums(again, want, len(s["src"]), seed)
    two = c_icp(s["src"], s["tv"], s["nrm"], max_iteration=2)
    assert two[18] == 2 and two[19] == 0 and np.abs(two[:16].reshape(4, 4) - AH.icp(s["src"], s["tv"], s["nrm"], max_iteration=2)["T"]).max() <= T_BAR
    rot, tr = AH.residual_motion(T, s["motion"])
    assert rot <= 5e-3 and tr <= 5e-3


def test_single_plane_returns_init_after_one_pass():
    target, normals = AH.plane_target(9)
    rng = np.random.default_rng(0)
    src = np.concatenate([rng.uniform(0.1, 0.9, (200, 2)), rng.uniform(-0.05, 0.05, (200, 1))], 1).astype(np.float32)
    for init in (None, INIT):
        state = c_icp(src, target, normals, init=init)
        assert np.array_equal(state[:16], (np.eye(4) if init is None else init).ravel())
        assert state[18] == 1 and state[19] == 1 and state[AH.STATE_SUMS][28] > 100
        up = np.zeros((6, 6))
        up[np.triu_indices(6)] = state[20:41]
        assert init is not None or not up[:, 2:5].any() and not up[2:5].any()             # at the identity: three columns exactly zero


def test_no_correspondence_no_source_and_excluded_points(scenes):
    s = scenes[SEEDS[0]]
    far = c_icp(s["src"] + np.float32(50), s["tv"], s["nrm"])
    assert np.array_equal(far[:16], np.eye(4).ravel()) and far[16] == 0 and far[17] == 0 and far[18] == 1 and far[19] == 1
    none = c_icp(np.zeros((0, 3), np.float32), s["tv"], s["nrm"], init=INIT)
    assert np.array_equal(none[:16], INIT.ravel()) and not none[16:].any()
    # non-finite sources, targets and normals take no part; the fitness denominator stays N
    src, tv, nrm = s["src"].copy(), s["tv"].copy(), s["nrm"].copy()
    src[::7, 1] = np.nan
    src[3::11, 0] = np.inf
    tv[::13, 2] = np.nan
    nrm[5::17, 0] = np.inf
    mirror = AH.icp_pass(src, tv, nrm, np.eye(4), 0.1)
    assert mirror["tie_gap"] >= TIE_BAR and mirror["thr_margin"] >= THRESHOLD_BAR
    state = c_icp(src, tv, nrm, max_iteration=0)
    check_sums(state, mirror, len(src), "excluded")
    assert 0 < mirror["count"] < 0.7 * len(src)
    dead = c_icp(s["src"], np.full_like(tv, np.nan), nrm)
    assert dead[16] == 0 and dead[19] == 1 and np.array_equal(dead[:16], np.eye(4).ravel())


# ------------------------------------------------------------------------------------------------ 4. ties
def test_duplicated_targets_go_to_the_smallest_index(scenes):
    s = scenes[SEEDS[2]]
    other = np.roll(s["nrm"], 1, axis=1)                                                 # a different unit normal for the second copy
    tgt = np.concatenate([s["tv"], s["tv"]])
    first, second = np.concatenate([s["nrm"], other]), np.concatenate([other, s["nrm"]])
    plain = AH.icp_pass(s["src"], s["tv"], s["nrm"], INIT, 0.1)
    assert plain["tie_gap"] >= TIE_BAR and plain["thr_margin"] >= THRESHOLD_BAR           # between DIFFERENT points the margins hold
    for nrm, label in ((first, "first"), (second, "second")):
        mirror = AH.icp_pass(s["src"], tgt, nrm, INIT, 0.1)
        assert mirror["index"].max() < len(s["tv"]) and mirror["count"] == plain["count"]
        a, b = c_icp(s["src"], tgt, nrm, max_iteration=0, init=INIT, calls=2)
        assert np.array_equal(a, b)
        check_sums(a, mirror, len(s["src"]), label)
    assert np.array_equal(AH.icp_pass(s["src"], tgt, first, INIT, 0.1)["sums"], plain["sums"])
    assert not np.allclose(AH.icp_pass(s["src"], tgt, second, INIT, 0.1)["sums"][:6], plain["sums"][:6], rtol=1e-3)   # the copies do differ


# ------------------------------------------------------------------------------------------------ 5. no host synchronisation
def test_icp_is_captured_in_a_graph_and_replays_bit_for_bit(scenes):
    s = scenes[SEEDS[0]]
    src, tv, nrm = dev(s["src"]), dev(s["tv"]), dev(s["nrm"])
    eager = Mh.icp_point_to_plane(src, tv, nrm, max_iteration=5).state.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                                        # any host synchronisation would break the capture
            captured = Mh.icp_point_to_plane(src, tv, nrm, max_iteration=5)
    for _ in range(2):
        captured.state.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.state, eager)
    assert int(eager[18]) == 5 and float(eager[16]) > 0.7


# ------------------------------------------------------------------------------------------------ 6. align_mesh, evaluate_raw_mesh
EVAL_CAM = CH.make_cam(160, 120, 140.0, 138.0, 80.3, 60.2)
EVAL_POSES = np.stack([np.eye(4, dtype=np.float32)] * 2)
EVAL_POSES[0, :3, 3] = (0.93, 0.71, 1.47)                     # OpenGL cameras above the height field, looking down -z
EVAL_POSES[1, :3, 3] = (1.21, 0.83, 1.43)


def camera_of(cam):
    return Camera(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], pixel_center=0.5)


def same_faces(got_v, got_f, want_v, want_f):
    return np.array_equal(got_v.cpu().numpy(), want_v) and np.array_equal(got_f.cpu().numpy(), want_f)


def test_align_mesh_and_evaluate_raw_mesh_with_icp(scenes):
    seed = SEEDS[2]
    s = scenes[seed]
    gt = (s["tv"], s["tf"])
    sv, sf = AH.lattice(54, 40, 0.3, 2.4, -0.2, 1.3)
    est = (s["src"], sf)                                                                 # the moved, noisy source as a mesh
    cam, poses = camera_of(EVAL_CAM), dev(EVAL_POSES)
    # the mirror's path, in the reference's order: cull the ground truth, align the unculled estimate to it, cull, score
    g = CH.cull(gt[0], gt[1], EVAL_POSES, EVAL_CAM, "occlusion")
    assert 0.3 * len(gt[1]) < g["keep"].sum() < 0.95 * len(gt[1])
    gv, gf = Mh.cull_mesh(dev(gt[0]), dev(gt[1]), poses, cam, "occlusion")
    assert same_faces(gv, gf, g["verts"], g["faces"])                                    # the premise: no doubtful face came out differently
    gn = AH.vertex_normals(g["verts"], g["faces"])
    want = AH.icp(est[0], g["verts"], gn)
    assert want["tie_gap"] >= TIE_BAR and want["thr_margin"] >= THRESHOLD_BAR and want["converged"] == 1
    moved = AH.transform(est[0], want["T"])
    e = CH.cull(moved, est[1], EVAL_POSES, EVAL_CAM, "occlusion")

    (av, af), res = Mh.align_mesh((dev(est[0]), dev(est[1])), (gv, gf))
    assert af.data_ptr() == dev(est[1]).data_ptr() or torch.equal(af, dev(est[1]))
    assert av.dtype == torch.float32 and np.abs(res.transformation.cpu().numpy() - want["T"]).max() <= T_BAR
    assert int(res.iterations) == want["iterations"] and float(res.fitness) == want["fitness"]
    dv = np.abs(av.cpu().numpy().astype(np.float64) - moved).max()
    print(f"aligned vertices: worst difference to the mirror {dv:.3e}; residual motion {AH.residual_motion(want['T'], s['motion'])}")
    assert dv <= 2.0 ** -22                                                             # one fp32 ulp at these coordinates
    colours = torch.arange(len(est[0]) * 3, device=DEV, dtype=torch.uint8).view(-1, 3)
    (cv, cf, cc), _ = Mh.align_mesh((dev(est[0]), dev(est[1]), colours), (gv, gf))
    assert cc is colours and torch.equal(cv, av)
    ev, ef = Mh.cull_mesh(av, af, poses, cam, "occlusion")
    assert np.array_equal(ef.cpu().numpy(), e["faces"]) and np.abs(ev.cpu().numpy() - e["verts"]).max() <= 2.0 ** -22

    args = ((dev(est[0]), dev(est[1])), (dev(gt[0]), dev(gt[1])), poses, cam, "occlusion", "occlusion")
    m = Mh.evaluate_raw_mesh(*args, num_points=20000, seed=0, align="icp")
    ref = Mh.evaluate_mesh((dev(e["verts"]), dev(e["faces"])), (dev(g["verts"]), dev(g["faces"])), num_points=20000, seed=0)
    plain = Mh.evaluate_raw_mesh(*args, num_points=20000, seed=0)
    print("aligned:", {k: round(v, 5) for k, v in m.items()})
    print("unaligned f1_1cm", round(plain["f1_1cm"], 5), "f1_5cm", round(plain["f1_5cm"], 5))
    assert tuple(m) == Mh.METRIC_KEYS
    for k in m:
        assert abs(m[k] - ref[k]) <= 1e-6, (k, m[k], ref[k])
    assert m["f1_1cm"] > plain["f1_1cm"] + 0.2 and m["acc"] < plain["acc"]
    with pytest.raises(NotImplementedError, match="mesh_alignment"):
        Mh.evaluate_raw_mesh(*args, mesh_alignment=True)
    with pytest.raises(ValueError, match="alignment"):
        Mh.evaluate_raw_mesh(*args, align="nearest")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_outputs_untouched(scenes):
    s = scenes[SEEDS[0]]
    L, INV = K.lib(), K.NGM_E_INVALID
    src, tv, nrm, tf = dev(s["src"]), dev(s["tv"]), dev(s["nrm"]), dev(s["tf"])
    n, m = len(src), len(tv)
    wsb = L.ngm_icp_point_to_plane_workspace(m, n)
    state, ws = Banded(64 * 8, PATTERN), Banded(wsb, PATTERN)
    nan, inf, big = float("nan"), float("inf"), 2 ** 31

    def icp_args(**kw):
        a = dict(source=src.data_ptr(), N=n, target=tv.data_ptr(), normals=nrm.data_ptr(), M=m, threshold=0.1, max_iteration=5, rf=1e-6, rr=1e-6,
                 init=None, state=state.ptr, ws=ws.ptr, wsb=wsb)
        a.update(kw)
        return tuple(a.values()) + (ops._stream(),)

    bad = [dict(N=-1), dict(M=-1), dict(M=0), dict(N=big), dict(M=big), dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=nan),
           dict(threshold=inf), dict(max_iteration=-1), dict(max_iteration=1001), dict(source=None), dict(target=None), dict(normals=None),
           dict(ws=None), dict(wsb=wsb - 1), dict(wsb=0)]
    for kw in bad:
        assert L.ngm_icp_point_to_plane(*icp_args(**kw)) == INV, kw
    assert L.ngm_icp_point_to_plane(*icp_args(state=None)) == INV
    torch.cuda.synchronize()
    assert bool((state.raw == PATTERN).all()) and bool((ws.raw == PATTERN).all())

    vwsb = L.ngm_mesh_vertex_normals_workspace(m)
    out, vws = Banded(12 * m, PATTERN), Banded(vwsb, PATTERN)

    def vn_args(**kw):
        a = dict(verts=tv.data_ptr(), V=m, faces=tf.data_ptr(), F=len(tf), normals=out.ptr, ws=vws.ptr, wsb=vwsb)
        a.update(kw)
        return tuple(a.values()) + (ops._stream(),)

    for kw in (dict(V=-1), dict(F=-1), dict(V=big), dict(F=big), dict(verts=None), dict(faces=None), dict(ws=None), dict(wsb=vwsb - 1), dict(wsb=0)):
        assert L.ngm_mesh_vertex_normals(*vn_args(**kw)) == INV, kw
    assert L.ngm_mesh_vertex_normals(*vn_args(normals=None)) == INV
    torch.cuda.synchronize()
    assert bool((out.raw == PATTERN).all()) and bool((vws.raw == PATTERN).all())
    # the same buffers, valid calls: the bands survive, the payloads are written
    assert L.ngm_mesh_vertex_normals(*vn_args()) == 0 and L.ngm_icp_point_to_plane(*icp_args()) == 0
    for b in (out, vws, state, ws):
        b.check()
    assert np.array_equal(out.payload(torch.float32).view(-1, 3).cpu().numpy(), c_normals(s["tv"], s["tf"]))
    assert state.payload(torch.float64)[18].item() >= 3
    with pytest.raises(K.NgmError):
        Mh.icp_point_to_plane(src, tv[:0], nrm[:0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.icp_point_to_plane(src.cpu(), tv, nrm)
