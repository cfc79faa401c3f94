"""-m gpu: culling a mesh on the device (include/ngm_hip.h ngm_mesh_depth / ngm_mesh_visibility; mesh.render_mesh_depth /
mesh_visibility / cull_mesh / evaluate_raw_mesh) against the fp64 host mirror tests/_mesh_cull_host.py and the reference's own
masks (fixture G29).

Depth maps: on the pixels the mirror does not flag as doubtful the coverage is identical and the depth is within DEPTH_BAR
(relative) of the mirror's.  Visibility: on the (vertex, pose) pairs that are not doubtful the masks are the reference's.
cull_mesh: the faces are the mirror's except those a doubtful pair decides."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_cull_host as CH  # noqa: E402
from gpu_common import DEV  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd.renderer import Camera  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Worst |z - z64| / z64 over every depth comparison of this module, measured on an MI355X: DEPTH_WORST = 1.122e-05, on the floor
# 5 cm under the camera (seen at up to 89.5 degrees of incidence; every scene within 80 degrees stays below 2.4e-06).  The bar
# is 4 x that, the margin the Adam tests take over an fp32 bound: 4.488e-05, inside the condition of at most 1e-4 (1 mm at
# 10 m, a thirtieth of eps).  Both numbers: profiles/r14_mesh_cull.json.
DEPTH_WORST = 1.122e-05
DEPTH_BAR = 4 * DEPTH_WORST
PAIR_CAP, FACE_CAP = 0.01, 0.05                      # tests/golden/make_golden_mesh_cull.py holds the mirror to both
EYE = np.eye(4, dtype=np.float32)                    # OpenGL camera at the origin looking down -z: camera space = (x, -y, -z)
CAM = CH.make_cam(64, 48, 50.0, 52.0, 32.25, 23.75)
CAM_EXACT = CH.make_cam(64, 48, 64.0, 64.0, 32.0, 24.0)          # powers of two: chosen corners project exactly
worst_seen = []


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def camera_of(cam):
    return Camera(cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], pixel_center=0.5)


def gpu_depth(verts, faces, c2ws, cam, near=0.01, far=10.0):
    d = Mh.render_mesh_depth(dev(np.asarray(verts, np.float32).reshape(-1, 3)), dev(np.asarray(faces, np.int64).reshape(-1, 3)),
                             dev(np.asarray(c2ws, np.float32).reshape(-1, 4, 4)), camera_of(cam), near, far)
    assert d.dtype == torch.float32 and tuple(d.shape) == (len(np.asarray(c2ws).reshape(-1, 4, 4)), cam["H"], cam["W"])
    return d.cpu().numpy()


def check_depth(verts, faces, c2ws, cam, near=0.01, far=10.0, label="", mirror=None):
    """the op against the mirror (of the float32 inputs the op gets): coverage identical and depth within the bar wherever the mirror
    has no doubt -> the op's maps"""
    verts, c2ws = np.asarray(verts, np.float32), np.asarray(c2ws, np.float32)
    want, doubt = mirror if mirror is not None else CH.render_depth(verts, faces, c2ws, cam, near, far)
    got = gpu_depth(verts, faces, c2ws, cam, near, far)
    sure = ~doubt
    both = sure & (want > 0) & (got > 0)
    rel = np.abs(got.astype(np.float64) - want)[both] / want[both]
    worst = float(rel.max()) if rel.size else 0.0
    worst_seen.append(worst)
    print(f"depth {label}: {int((want > 0).sum())} covered, {int((doubt & (want > 0)).sum())} doubtful, coverage differs on "
          f"{int(((got > 0) != (want > 0))[sure].sum())} sure pixels, worst relative depth error {worst:.3e} (bar {DEPTH_BAR:.3e})")
    assert np.isfinite(got).all() and (got >= 0).all()
    assert np.array_equal((got > 0)[sure], (want > 0)[sure])
    assert worst <= DEPTH_BAR
    return got


@pytest.fixture(scope="module")
def g29():
    return CH.load_g29(os.path.join(ROOT, "tests", "golden", "g29_mesh_cull.npz"))


def scaled(cam, w, h):
    return CH.make_cam(w, h, cam["fx"] * w / cam["W"], cam["fy"] * h / cam["H"], cam["cx"] * w / cam["W"], cam["cy"] * h / cam["H"])


# ------------------------------------------------------------------------------------------------ ngm_mesh_depth on G29
@pytest.mark.parametrize("size", [(160, 120), (61, 47)])
def test_depth_against_the_mirror_on_the_g29_scene(g29, size):
    cam = scaled(g29["cam"], *size)
    mirror = CH.render_depth(g29["verts"], g29["faces"], g29["c2ws"], cam)
    covered = mirror[0] > 0
    assert (mirror[1] & covered).sum() <= 0.02 * covered.sum()
    every = check_depth(g29["verts"], g29["faces"], g29["c2ws"], cam, label=f"G29 {size} all poses", mirror=mirror)
    one = check_depth(g29["verts"], g29["faces"], g29["c2ws"][:1], cam, label=f"G29 {size} P=1", mirror=(mirror[0][:1], mirror[1][:1]))
    assert np.array_equal(one[0].view(np.uint32), every[0].view(np.uint32))           # a pose's map does not depend on the others
    assert not every[5].any()                                                          # the pose outside, looking away


# ------------------------------------------------------------------------------------------------ shapes where the kernel can go wrong
def screen_to_world(cam, sx, sy, z):
    """the world point (identity pose) that projects to (sx, sy) at camera depth z"""
    return ((sx - cam["cx"]) / cam["fx"] * z, -(sy - cam["cy"]) / cam["fy"] * z, -z)


def random_tris(n, seed, cam=CAM):
    """n small triangles in view, facing the camera to within about 45 degrees"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.5, 4.0, n)
    c = np.stack(screen_to_world(cam, rng.uniform(2, cam["W"] - 2, n), rng.uniform(2, cam["H"] - 2, n), z), -1)
    v = c[:, None, :] + rng.uniform(-0.12, 0.12, (n, 3, 3)) * (1, 1, 0.5)
    return v.reshape(-1, 3).astype(np.float32), np.arange(3 * n).reshape(n, 3)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_depth_face_counts_around_a_wave(n):
    v, f = random_tris(n, 100 + n)
    got = check_depth(v, f, EYE[None], CAM, label=f"F={n}")
    assert (got > 0).any()


def wall_and_crowd():
    v, f = random_tris(300, 7)
    wall = np.array([screen_to_world(CAM, sx, sy, 4.5 + 0.01 * k) for k, (sx, sy) in enumerate(((-9, -7), (75, -6), (74, 55), (-8, 56)))], np.float32)
    faces = np.concatenate([f[:100], [[900, 901, 902], [900, 902, 903]], f[100:]])          # the wall in the middle of a wave
    return np.concatenate([v, wall]), faces


def test_depth_wall_behind_a_crowd_of_tiny_triangles():
    """two triangles that fill the screen (the wave's shared path) among 300 of a few pixels (each lane's own path)"""
    v, f = wall_and_crowd()
    got = check_depth(v, f, EYE[None], CAM, label="wall + crowd")
    assert (got > 0).all() and (got < 4.4).any() and (got > 4.4).any()
    check_depth(v[900:], [[0, 1, 2], [0, 2, 3]], EYE[None], CAM, label="wall alone")
    check_depth(v, f[[100]], EYE[None], CAM, label="one large face alone in its wave")


def test_depth_boxes_at_the_small_large_threshold():
    """bounding boxes of 8 x 4 = 32 pixels (the last that stays with its lane), 9 x 4 and 11 x 3 = 33 (the first the wave shares)"""
    tris = {"8x4": ((10.2, 10.2), (18.1, 10.3), (10.3, 14.1)), "9x4": ((10.2, 20.2), (19.1, 20.3), (10.3, 24.1)),
            "11x3": ((30.2, 10.2), (41.1, 10.3), (30.3, 13.1)), "4x8": ((50.2, 10.2), (54.1, 10.3), (50.3, 18.1))}
    vs = {k: np.array([screen_to_world(CAM, sx, sy, 2.0 + 0.1 * i) for i, (sx, sy) in enumerate(t)], np.float32) for k, t in tris.items()}
    for k, v in vs.items():
        got = check_depth(v, [[0, 1, 2]], EYE[None], CAM, label=f"box {k}")
        vv, uu = np.nonzero(got[0])
        w, h = (int(s) for s in k.split("x"))
        assert uu.max() - uu.min() + 1 <= w and vv.max() - vv.min() + 1 <= h and len(uu) > w * h // 3
    allv = np.concatenate(list(vs.values()))
    check_depth(allv, np.arange(12).reshape(4, 3), EYE[None], CAM, label="boxes together")


def test_depth_vertex_exactly_on_a_pixel_centre():
    cam = CAM_EXACT
    v = np.array([screen_to_world(cam, 20.5, 15.5, 2.0), screen_to_world(cam, 40.5, 17.5, 2.0), screen_to_world(cam, 24.5, 35.5, 2.0)], np.float32)
    assert np.array_equal(v.astype(np.float64), np.array([screen_to_world(cam, 20.5, 15.5, 2.0), screen_to_world(cam, 40.5, 17.5, 2.0),
                                                          screen_to_world(cam, 24.5, 35.5, 2.0)]))                  # exact in float32
    got = check_depth(v, [[0, 1, 2]], EYE[None], cam, label="corner on a pixel centre")
    for u, w in ((20, 15), (40, 17), (24, 35)):                       # ON the triangle counts, and the arithmetic is exact here
        assert got[0, w, u] == 2.0
    assert got[0, 15, 19] == 0 and got[0, 14, 20] == 0


def test_depth_triangles_leaving_the_image_on_every_side():
    cases = {"left": ((-20, 10), (9, 14), (-5, 30)), "right": ((55, 12), (90, 20), (60, 33)), "top": ((20, -15), (40, -3), (30, 9)),
             "bottom": ((20, 40), (44, 44), (31, 70)), "corner": ((50, 35), (90, 40), (60, 80)), "around": ((-40, -30), (200, -20), (30, 160))}
    allv = []
    for k, t in cases.items():
        v = np.array([screen_to_world(CAM, sx, sy, 2.0 + 0.2 * i) for i, (sx, sy) in enumerate(t)], np.float32)
        allv.append(v)
        got = check_depth(v, [[0, 1, 2]], EYE[None], CAM, label=f"leaving {k}")
        assert (got > 0).any()
    out = np.array([screen_to_world(CAM, sx, sy, 2.0) for sx, sy in ((-30, 5), (-3, 8), (-10, 30))], np.float32)   # wholly outside
    assert not check_depth(out, [[0, 1, 2]], EYE[None], CAM, label="outside").any()
    check_depth(np.concatenate(allv), np.arange(18).reshape(6, 3), EYE[None], CAM, label="leaving, together")


def test_depth_near_plane_and_far():
    one_behind = [(-0.6, -0.4, -1.5), (0.7, -0.5, -1.2), (0.05, 0.1, 0.8)]
    two_behind = [(-0.2, -0.3, -1.5), (0.9, -0.2, 0.6), (-0.8, 0.3, 0.4)]
    floor = [(-3.0, -0.05, 2.0), (3.0, -0.05, 2.0), (0.0, -0.05, -6.0)]
    for label, tri, near in (("one corner behind", one_behind, 0.5), ("two corners behind", two_behind, 0.5), ("floor under the camera", floor, 0.01),
                             ("one corner behind, near 0.01", one_behind, 0.01)):
        got = check_depth(tri, [[0, 1, 2]], EYE[None], CAM, near=near, label=label)
        assert (got > 0).any() and got[got > 0].min() >= near * (1 - 1e-6)
    behind = [(-1.0, -0.8, 2.0), (1.1, -0.7, 2.0), (0.1, 0.9, 2.0)]
    assert not check_depth(behind, [[0, 1, 2]], EYE[None], CAM, label="behind the camera").any()
    beyond = [(-5.0, -4.0, -12.0), (5.0, -4.0, -12.0), (0.0, 5.0, -12.0)]
    assert not check_depth(beyond, [[0, 1, 2]], EYE[None], CAM, label="beyond far").any()
    got = check_depth([(-5.0, -4.0, -12.0), (5.0, -4.0, -12.0), (0.0, 2.0, -3.0)], [[0, 1, 2]], EYE[None], CAM, label="across far")
    assert (got > 0).any() and got.max() <= 10.0


def test_depth_skipped_faces_and_a_lost_pose():
    v = np.array([(-1.0, -0.8, -2.0), (1.1, -0.7, -2.0), (0.1, 0.9, -2.0), (np.nan, 0, -2.0), (0.3, np.inf, -2.0)], np.float32)
    good = gpu_depth(v, [[0, 1, 2]], EYE[None], CAM)
    assert (good > 0).sum() > 500
    for faces in ([[0, 1, 5]], [[0, 1, -1]], [[2 ** 40, 1, 2]], [[0, 1, 3]], [[4, 1, 2]], [[0, 1, 1]], [[2, 2, 2]]):
        assert not gpu_depth(v, faces, EYE[None], CAM).any(), faces
    mixed = gpu_depth(v, [[0, 1, 5], [0, 1, 2], [0, 0, 1], [0, 1, 3], [-7, 1, 2]], EYE[None], CAM)
    assert np.array_equal(mixed.view(np.uint32), good.view(np.uint32))
    lost, singular = EYE.copy(), EYE.copy()
    lost[1, 3] = np.nan
    singular[:3, :3] = 0
    got = gpu_depth(v, [[0, 1, 2]], np.stack([lost, EYE, singular, EYE]), CAM)
    assert not got[0].any() and not got[2].any()
    assert np.array_equal(got[1].view(np.uint32), good[0].view(np.uint32)) and np.array_equal(got[3].view(np.uint32), good[0].view(np.uint32))
    assert not gpu_depth(v, np.zeros((0, 3), np.int64), EYE[None], CAM).any()                    # no faces: zero maps
    assert not gpu_depth(np.zeros((0, 3), np.float32), [[0, 1, 2]], EYE[None], CAM).any()        # no vertices
    assert gpu_depth(v, [[0, 1, 2]], np.zeros((0, 4, 4), np.float32), CAM).shape == (0, CAM["H"], CAM["W"])


def test_depth_is_repeatable_bit_for_bit(g29):
    v, f = wall_and_crowd()
    cases = [(v, f, EYE[None], CAM), (g29["verts"], g29["faces"], g29["c2ws"], g29["cam"])]
    for verts, faces, c2ws, cam in cases:
        args = (dev(np.asarray(verts, np.float32)), dev(np.asarray(faces, np.int64)), dev(np.asarray(c2ws, np.float32)), camera_of(cam))
        a = Mh.render_mesh_depth(*args)
        b = Mh.render_mesh_depth(*args)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            c = Mh.render_mesh_depth(*args)
        side.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
        assert bool((a > 0).any())


# ------------------------------------------------------------------------------------------------ ngm_mesh_visibility
def gpu_visibility(verts, c2ws, cam, depth=None, eps=0.03, nfp=None):
    i, o = Mh.mesh_visibility(dev(np.asarray(verts, np.float32).reshape(-1, 3)), dev(np.asarray(c2ws, np.float32).reshape(-1, 4, 4)),
                              camera_of(cam), None if depth is None else dev(np.asarray(depth, np.float32)), eps, nfp)
    assert i.dtype == torch.int32 and o.dtype == torch.int32
    return i.cpu().numpy(), o.cpu().numpy()


def test_visibility_against_the_reference_masks_g29(g29):
    verts, c2ws, cam, depth = g29["verts"], g29["c2ws"], g29["cam"], g29["depth"]
    _, pdoubt = CH.render_depth(verts, g29["faces"], c2ws, cam)
    _, _, doubt = CH.visibility(verts, c2ws, cam, depth, g29["eps"], pdoubt)
    assert doubt.sum() <= PAIR_CAP * doubt.size
    per_pose = [gpu_visibility(verts, c2ws[p:p + 1], cam, depth[p:p + 1], g29["eps"]) for p in range(len(c2ws))]
    ins, seen = np.stack([a for a, _ in per_pose]), np.stack([b for _, b in per_pose])
    assert set(np.unique(ins)) <= {0, 1} and set(np.unique(seen)) <= {0, 1}
    wrong_in, wrong_seen = (ins != g29["ref_in_frustum"]) & ~doubt, (seen != g29["ref_observed"]) & ~doubt
    print(f"visibility G29: {doubt.sum()} of {doubt.size} pairs doubtful; differing from the reference among them: in_frustum "
          f"{int((ins != g29['ref_in_frustum']).sum())}, observed {int((seen != g29['ref_observed']).sum())}; outside them: "
          f"{int(wrong_in.sum())}, {int(wrong_seen.sum())}")
    assert not wrong_in.any() and not wrong_seen.any()
    # all poses in one call: the sums; num_frustum_poses: later poses add to `observed` only
    nfp = g29["num_frustum_poses"]
    a, b = gpu_visibility(verts, c2ws, cam, depth, g29["eps"])
    assert np.array_equal(a, ins.sum(0)) and np.array_equal(b, seen.sum(0))
    a, b = gpu_visibility(verts, c2ws, cam, depth, g29["eps"], nfp)
    assert np.array_equal(a, ins[:nfp].sum(0)) and np.array_equal(b, seen.sum(0)) and not np.array_equal(ins[:nfp].sum(0), ins.sum(0))
    a, b = gpu_visibility(verts, c2ws, cam, depth, g29["eps"], 0)
    assert not a.any() and np.array_equal(b, seen.sum(0))
    # no depth maps: the frustum-only result
    a, b = gpu_visibility(verts, c2ws, cam, None, g29["eps"], nfp)
    assert np.array_equal(a, ins[:nfp].sum(0)) and np.array_equal(b, ins.sum(0))
    # a vertex's counts do not depend on the others: V = 1, 63, 65
    full = gpu_visibility(verts, c2ws, cam, depth, g29["eps"])
    for n in (1, 63, 65):
        start = 3000
        part = gpu_visibility(verts[start:start + n], c2ws, cam, depth, g29["eps"])
        assert np.array_equal(part[0], full[0][start:start + n]) and np.array_equal(part[1], full[1][start:start + n])
    lost = c2ws.copy()
    lost[2, 0, 0] = np.inf
    a, b = gpu_visibility(verts, lost, cam, depth, g29["eps"])
    assert np.array_equal(a, ins.sum(0) - ins[2]) and np.array_equal(b, seen.sum(0) - seen[2])


def test_visibility_calls_over_chunks_of_the_poses_add_up(g29):
    """the entry point ADDS: two calls over 5 + 3 poses into the same counters equal one call over all 8 (70 poses: the staging of 64
    poses at a time runs twice)"""
    L = K.lib()
    cam = g29["cam"]
    verts, depth = dev(g29["verts"]), dev(g29["depth"])
    c2ws = dev(np.concatenate([g29["c2ws"]] * 9)[:70])
    depth70 = torch.cat([depth] * 9)[:70].contiguous()
    intr = (cam["W"], cam["H"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    nv = verts.shape[0]

    def run(chunks, nfp):
        a = torch.full((nv,), 7, device=DEV, dtype=torch.int32)              # adds: what was there stays
        b = torch.full((nv,), -2, device=DEV, dtype=torch.int32)
        for s, e in chunks:
            K.check(L.ngm_mesh_visibility(verts.data_ptr(), nv, c2ws[s:e].data_ptr(), e - s, *intr, depth70[s:e].data_ptr(), g29["eps"],
                                          max(0, min(nfp - s, e - s)), a.data_ptr(), b.data_ptr(), ops._stream()), "ngm_mesh_visibility")
        return a - 7, b + 2
    whole = run([(0, 70)], 66)
    for chunks in ([(0, 5), (5, 70)], [(0, 64), (64, 70)], [(0, 16), (16, 32), (32, 48), (48, 64), (64, 70)]):
        part = run(chunks, 66)
        assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1])
    eight = gpu_visibility(g29["verts"], g29["c2ws"], cam, g29["depth"], g29["eps"])
    assert np.array_equal(run([(0, 8)], 8)[0].cpu().numpy(), eight[0]) and bool((whole[1] > 8).any())


# ------------------------------------------------------------------------------------------------ cull_mesh
def gpu_cull(g, method, bounds=None, poses=slice(None), **kw):
    verts = dev(g["verts"])
    ids = torch.arange(len(g["verts"]), device=DEV)
    out = Mh.cull_mesh(verts, dev(g["faces"]), dev(g["c2ws"][poses]), camera_of(g["cam"]), method,
                       bounds=None if bounds is None else dev(bounds), colors=ids, **kw)
    v, f, ids = (t.cpu().numpy() for t in out)
    assert f.dtype == np.int64 and v.dtype == np.float32
    assert np.array_equal(v, g["verts"][ids]) and (np.diff(ids) > 0).all()              # vertex order kept
    assert len(f) == 0 or (f.min() >= 0 and f.max() < len(v))
    return v, f, ids


@pytest.mark.parametrize("with_bounds", [False, True])
@pytest.mark.parametrize("method", ["frustum", "occlusion", "virt_cams"])
def test_cull_mesh_against_the_mirror_g29(g29, method, with_bounds):
    bounds = g29["bounds"] if with_bounds else None
    nfp = g29["num_frustum_poses"] if method == "virt_cams" else None
    want = CH.cull(g29["verts"], g29["faces"], g29["c2ws"], g29["cam"], method, bounds=bounds, num_frustum_poses=nfp)
    share = want["face_doubt"].sum() / max(want["start"].sum(), 1)
    assert share <= FACE_CAP and 0 < want["keep"].sum() < len(g29["faces"])
    v, f, ids = gpu_cull(g29, method, bounds, num_frustum_poses=nfp, pose_chunk=3)
    got_faces = {tuple(t) for t in ids[f].tolist()}
    assert len(got_faces) == len(f)
    want_faces = {tuple(t) for t in g29["faces"][want["keep"]].tolist()}
    doubtful = {tuple(t) for t in g29["faces"][want["face_doubt"]].tolist()}
    differ = got_faces ^ want_faces
    print(f"cull_mesh {method} bounds={with_bounds}: {len(got_faces)} faces kept (mirror {len(want_faces)}), {len(differ)} differ, "
          f"{len(doubtful)} doubtful ({share:.4%} of {int(want['start'].sum())})")
    assert differ <= doubtful
    # every vertex that is left is referred to by a face
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    if with_bounds:
        assert v[:, 0].max() <= 4.0 + 0.02 + 1e-6                                          # the annex outside the room is gone
    elif method == "frustum":
        assert v[:, 0].max() > 4.5
    # the chunk size does not matter
    v2, f2, ids2 = gpu_cull(g29, method, bounds, num_frustum_poses=nfp, pose_chunk=16)
    assert np.array_equal(ids2, ids) and np.array_equal(f2, f)


def test_cull_mesh_removes_the_hidden_side_of_the_inner_box(g29):
    """from pose 0 alone (eye at 0.5 0.5 1.2) the box's side x = 2.4 is behind the box: the occlusion methods take its faces away,
    the frustum method keeps them.  Faces at the side's rim share positions with visible vertices: only the inner ones are asked."""
    v = g29["verts"].astype(np.float64)
    c = v[g29["faces"]]
    inner = (np.abs(c[:, :, 0] - 2.4) < 1e-6).all(1) & (c[:, :, 1] > 1.35).all(1) & (c[:, :, 1] < 1.65).all(1) & \
        (c[:, :, 2] > 0.45).all(1) & (c[:, :, 2] < 1.15).all(1)
    hidden = {tuple(t) for t in g29["faces"][inner].tolist()}
    assert len(hidden) >= 20
    for method, kept in (("frustum", True), ("occlusion", False), ("virt_cams", False)):
        _, f, ids = gpu_cull(g29, method, poses=slice(0, 1))
        got = {tuple(t) for t in ids[f].tolist()}
        assert (hidden <= got) if kept else not (hidden & got), method


def test_cull_mesh_edge_cases():
    cam = camera_of(CAM)
    v, f = random_tris(40, 3)
    f = np.concatenate([f, [[0, 0, 1], [5, 120, 6], [-1, 2, 3]]])                      # repeated index, out of range twice
    vt, ft, c2w = dev(v), dev(f), dev(EYE[None])
    want = CH.cull(v, f, EYE[None], CAM, "frustum")
    assert want["keep"].sum() == 41 and not want["face_doubt"].any()                   # the repeated-index face is kept until the end
    out_v, out_f = Mh.cull_mesh(vt, ft, c2w, cam, "frustum")
    assert np.array_equal(out_f.cpu().numpy(), want["faces"]) and len(want["faces"]) == 40 and torch.equal(out_v, vt)
    away = EYE.copy()
    away[:3, :3] = np.diag([-1.0, 1.0, -1.0])                                           # turned round: nothing in view
    out_v, out_f = Mh.cull_mesh(vt, ft, dev(away[None]), cam, "occlusion")
    assert out_v.shape == (0, 3) and out_f.shape == (0, 3)
    out_v, out_f = Mh.cull_mesh(vt, ft, dev(np.zeros((0, 4, 4), np.float32)), cam, "occlusion")
    assert out_v.shape == (0, 3) and out_f.shape == (0, 3)
    out_v, out_f = Mh.cull_mesh(vt, ft[:0], c2w, cam, "occlusion")
    assert out_v.shape == (0, 3) and out_f.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ evaluate_raw_mesh
def uv_sphere(radius, centre, n_lat=24, n_lon=48):
    th = np.linspace(0, np.pi, n_lat + 1)
    ph = np.arange(n_lon) * (2 * np.pi / n_lon)
    v = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None], np.cos(th)[:, None] * np.ones((1, n_lon))], -1)
    i, j = np.arange(n_lat)[:, None] * n_lon, np.arange(n_lon)[None]
    a, b = i + j, i + (j + 1) % n_lon
    f = np.concatenate([np.stack([a, a + n_lon, b], -1).reshape(-1, 3), np.stack([b, a + n_lon, b + n_lon], -1).reshape(-1, 3)])
    return (radius * v.reshape(-1, 3) + np.asarray(centre)).astype(np.float32), f.astype(np.int64)


SPHERE_CENTRE = (0.11, -0.05, -1.75)
SPHERE_CAM = CH.make_cam(160, 120, 140.0, 138.0, 80.3, 60.2)
SPHERE_POSES = np.stack([EYE, EYE]).copy()
SPHERE_POSES[1, :3, 3] = (0.4, 0.25, 0.1)


def tilted_sphere(radius):
    """the poles 40 degrees off the viewing axis: neither on the silhouette nor in the middle of the image"""
    v, f = uv_sphere(radius, (0.0, 0.0, 0.0))
    a = np.deg2rad(40.0)
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    return (v.astype(np.float64) @ rot.T + np.asarray(SPHERE_CENTRE)).astype(np.float32), f


def test_evaluate_raw_mesh_two_concentric_half_visible_spheres():
    """radius 0.62 against 0.6, seen from two poses on one side: the far halves are culled.  The ten numbers are those of
    evaluate_mesh on the MIRROR-culled meshes.  The samples are drawn from the culled meshes, so this holds only where no
    doubtful face came out differently: for this scene none does (asserted first, face by face)."""
    est, gt = tilted_sphere(0.62), tilted_sphere(0.6)
    cam = SPHERE_CAM
    want = {}
    for name, (v, f) in (("est", est), ("gt", gt)):
        r = CH.cull(v, f, SPHERE_POSES, cam, "occlusion")
        assert 0.2 * len(f) < r["keep"].sum() < 0.6 * len(f)
        got_v, got_f, ids = gpu_cull(dict(verts=v, faces=f, c2ws=SPHERE_POSES, cam=cam), "occlusion")
        differ = {tuple(t) for t in ids[got_f].tolist()} ^ {tuple(t) for t in f[r["keep"] & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])].tolist()}
        print(f"{name}: {int(r['keep'].sum())} of {len(f)} faces kept, {int(r['face_doubt'].sum())} doubtful, {len(differ)} differ")
        assert differ <= {tuple(t) for t in f[r["face_doubt"]].tolist()}
        assert not differ
        want[name] = (dev(r["verts"]), dev(r["faces"]))
    m = Mh.evaluate_raw_mesh((dev(est[0]), dev(est[1])), (dev(gt[0]), dev(gt[1])), dev(SPHERE_POSES), camera_of(cam), "occlusion", "occlusion",
                             num_points=20000, seed=0)
    ref = Mh.evaluate_mesh(want["est"], want["gt"], num_points=20000, seed=0)
    print("half-visible spheres:", {k: round(v, 5) for k, v in m.items()})
    assert tuple(m) == Mh.METRIC_KEYS
    for k in m:
        assert abs(m[k] - ref[k]) <= 1e-6, (k, m[k], ref[k])
    # 2 cm apart wherever both are left; the two rims are not cut at the same place, so a few per cent of the points look past it
    assert abs(m["median_acc"] - 0.02) <= 0.002 and abs(m["median_comp"] - 0.02) <= 0.002
    assert m["acc_ratio"] > 0.95 and m["comp_ratio"] > 0.9 and m["f1_1cm"] == 0.0
    with pytest.raises(NotImplementedError):
        Mh.evaluate_raw_mesh((dev(est[0]), dev(est[1])), (dev(gt[0]), dev(gt[1])), dev(SPHERE_POSES), camera_of(cam), "occlusion", "occlusion",
                             mesh_alignment=True)


# ------------------------------------------------------------------------------------------------ memory safety
GUARD, PATTERN = 4096, 0xA5


@contextmanager
def guard_bands():
    """tests/test_gpu_safety.py's guard bands, restated for the allocations of the two ops (torch.empty with dtype and device):
    4 KiB of pattern on either side of every output, checked after a device synchronisation"""
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


def test_guard_bands_around_every_output(g29):
    wv, wf = wall_and_crowd()
    with guard_bands() as raws:
        for size in ((160, 120), (61, 47), (1, 1), (7, 3)):
            cam = scaled(g29["cam"], *size)
            d = Mh.render_mesh_depth(dev(g29["verts"]), dev(g29["faces"]), dev(g29["c2ws"]), camera_of(cam))
            for n in (1, 63, 65, len(g29["verts"])):
                Mh.mesh_visibility(dev(g29["verts"][:n]), dev(g29["c2ws"]), camera_of(cam), d)
        for n in (1, 63, 64, 65):
            Mh.render_mesh_depth(dev(wv), dev(wf[:n + 100]), dev(EYE[None]), camera_of(CAM))
        Mh.cull_mesh(dev(g29["verts"]), dev(g29["faces"]), dev(g29["c2ws"]), camera_of(g29["cam"]), "occlusion", pose_chunk=3)
    assert len(raws) >= 4 * (1 + 4 * 2) + 4 + 3 * 3


def test_ops_fake_shapes_and_cpu_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        v, f = torch.empty(50, 3, device=DEV), torch.empty(20, 3, dtype=torch.int64, device=DEV)
        c = torch.empty(7, 4, 4, device=DEV)
        d = torch.ops.ngm355.mesh_depth(v, f, c, 61, 47, 10.0, 10.0, 8.0, 6.0, 0.01, 10.0)
        assert d.shape == (7, 47, 61) and d.dtype == torch.float32
        i, o = torch.ops.ngm355.mesh_visibility(v, c, d, 61, 47, 10.0, 10.0, 8.0, 6.0, 0.03, 5)
        assert i.shape == (50,) and i.dtype == torch.int32 and o.shape == (50,) and o.dtype == torch.int32
    v, f, c = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.eye(4)[None]
    with pytest.raises(RuntimeError):
        Mh.render_mesh_depth(v, f, c, camera_of(CAM))
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.ngm355.mesh_depth(v, f, c, 16, 12, 10.0, 10.0, 8.0, 6.0, 0.01, 10.0)
    with pytest.raises(K.NgmError):
        Mh.render_mesh_depth(v.to(DEV), f.to(DEV), c.to(DEV), camera_of(CAM), near=0.0)
    with pytest.raises(K.NgmError):
        Mh.render_mesh_depth(v.to(DEV), f.to(DEV), c.to(DEV), camera_of(CAM), near=1.0, far=0.5)


def test_depth_bar_is_four_times_the_worst_error_seen():
    """runs last in this module: every depth comparison above stayed within the bar; the bar itself meets the issue's condition"""
    assert DEPTH_BAR == 4 * DEPTH_WORST and DEPTH_BAR <= 1e-4
    if worst_seen:
        print(f"worst relative depth error over {len(worst_seen)} comparisons: {max(worst_seen):.3e} (recorded {DEPTH_WORST:.3e}, bar {DEPTH_BAR:.3e})")
        assert max(worst_seen) <= DEPTH_BAR
