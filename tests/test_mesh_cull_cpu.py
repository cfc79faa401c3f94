"""CPU-side checks of mesh culling (include/ngm_hip.h ngm_mesh_depth / ngm_mesh_visibility; mesh.render_mesh_depth /
mesh_visibility / cull_mesh / evaluate_raw_mesh): the host mirror tests/_mesh_cull_host.py -- the GPU tests' yardstick -- against
the reference's own masks (fixture G29, tests/golden/make_golden_mesh_cull.py) and against triangles whose depth maps are
known in closed form; the face rule and the compaction on a mesh written out by hand; the C ABI's refusals, which need no
device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_cull_host as CH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_CAP, PIXEL_CAP = 0.01, 0.02                     # the issue's caps on doubtful (vertex, pose) pairs and covered pixels


@pytest.fixture(scope="module")
def g29():
    g = CH.load_g29(os.path.join(ROOT, "tests", "golden", "g29_mesh_cull.npz"))
    g["mirror_depth"], g["pixel_doubt"] = CH.render_depth(g["verts"], g["faces"], g["c2ws"], g["cam"])
    return g


# ------------------------------------------------------------------------------------------------ the mirror against G29
def test_fixture_is_data_only_and_small():
    path = os.path.join(ROOT, "tests", "golden", "g29_mesh_cull.npz")
    assert os.path.getsize(path) < 200 * 1000
    with np.load(path, allow_pickle=False) as g:
        assert all(g[k].dtype.kind in "fiub" for k in g.files)


def test_mirror_depth_maps_are_the_stored_ones_g29(g29):
    """the stored maps are the mirror's, rounded to the fixture's step: a rerun gives the same counts (a depth within rounding of
    a half step may land on either side)"""
    counts = np.rint(g29["mirror_depth"] / g29["depth_step"])
    diff = np.abs(counts - g29["depth_counts"])
    assert diff.max() <= 1 and (diff != 0).mean() <= 1e-3
    covered = g29["mirror_depth"] > 0
    assert (g29["pixel_doubt"] & covered).sum() <= PIXEL_CAP * covered.sum()
    assert not covered[5].any() and all(covered[p].any() for p in (0, 1, 2, 3, 4, 6, 7))


def test_mirror_visibility_reproduces_the_reference_g29(g29):
    ins, seen, doubt = CH.visibility(g29["verts"], g29["c2ws"], g29["cam"], g29["depth"], g29["eps"], g29["pixel_doubt"])
    assert doubt.mean() <= PAIR_CAP
    assert ((ins == g29["ref_in_frustum"]) | doubt).all() and ((seen == g29["ref_observed"]) | doubt).all()
    nv = len(g29["verts"])
    for p in (0, 1, 2, 3, 4, 6, 7):                                       # every pose that looks at the room: mixed masks
        assert 0 < g29["ref_in_frustum"][p].sum() < nv and 0 < g29["ref_observed"][p].sum() < nv
    assert not g29["ref_in_frustum"][5].any()
    hidden = (g29["ref_in_frustum"] & ~g29["ref_observed"])[:4].sum() / g29["ref_in_frustum"][:4].sum()
    assert hidden >= 0.03
    # without depth maps: seen is inside
    ins2, seen2, _ = CH.visibility(g29["verts"], g29["c2ws"], g29["cam"])
    assert np.array_equal(ins2, ins) and np.array_equal(seen2, ins)


def test_mirror_bounds_rule_reproduces_the_reference_g29(g29):
    mine = CH.cull_by_bounds(g29["verts"], g29["bounds"])
    assert np.array_equal(mine, g29["ref_bounds"]) and 0 < mine.sum() < len(mine)


# ------------------------------------------------------------------------------------------------ hand cases
CAM = CH.make_cam(64, 48, 50.0, 52.0, 32.25, 23.75)
EYE = np.eye(4)                                       # OpenGL camera at the origin looking down -z: camera space = (x, -y, -z)


def ray_reference(tri_world, cam, near=0.01, far=10.0):
    """depth map of ONE triangle under the identity pose by ray casting, no clipping and no projection of corners: the ray
    through a pixel centre meets the triangle's plane at z = n.v0 / n.d, inside or on the triangle by 3-D edge tests ->
    (depth, margin): margin = the smallest absolute edge function, normalised (small: the sample is next to an edge)"""
    t = np.asarray(tri_world, np.float64) * (1, -1, -1)
    n = np.cross(t[1] - t[0], t[2] - t[0])
    v, u = np.meshgrid(np.arange(cam["H"]), np.arange(cam["W"]), indexing="ij")
    d = np.stack([(u + 0.5 - cam["cx"]) / cam["fx"], (v + 0.5 - cam["cy"]) / cam["fy"], np.ones(u.shape)], -1)
    with np.errstate(all="ignore"):
        z = (n @ t[0]) / (d @ n)
    hit = d * z[..., None]
    e = np.stack([np.cross(t[(k + 1) % 3] - t[k], hit - t[k]) @ n for k in range(3)], -1) / (n @ n)
    inside = (e >= 0).all(-1) | (e <= 0).all(-1)
    ok = inside & (z >= near) & (z <= far)
    return np.where(ok, z, 0.0), np.abs(e).min(-1)


def check_against_rays(tri, near=0.01, far=10.0):
    depth, doubt = CH.render_depth(tri, [[0, 1, 2]], EYE[None], CAM, near, far)
    want, margin = ray_reference(tri, CAM, near, far)
    sure = ~doubt[0] & (margin > 1e-6) & (np.abs(want - near) > 1e-9) & (np.abs(want - far) > 1e-6)
    assert np.array_equal((depth[0] > 0)[sure], (want > 0)[sure])
    assert np.abs(depth[0] - want)[sure].max() <= 1e-9
    return depth[0], want


def test_triangle_facing_the_camera_has_the_plane_depth():
    depth, want = check_against_rays([(-1.0, -0.8, -2.0), (1.1, -0.7, -2.0), (0.1, 0.9, -2.0)])
    assert (depth > 0).sum() > 500 and np.abs(depth[depth > 0] - 2.0).max() <= 1e-12
    depth, want = check_against_rays([(-1.0, -0.8, -2.5), (1.1, -0.7, -1.6), (0.1, 0.9, -3.0)])          # tilted
    assert (depth > 0).sum() > 300 and depth[depth > 0].min() > 1.6 and depth.max() < 3.0


def test_both_windings_give_the_same_map():
    v = [(-1.0, -0.8, -2.5), (1.1, -0.7, -1.6), (0.1, 0.9, -3.0)]
    a = CH.render_depth(v, [[0, 1, 2]], EYE[None], CAM)
    b = CH.render_depth(v, [[0, 2, 1]], EYE[None], CAM)
    assert (a[0] > 0).any() and np.abs(a[0] - b[0]).max() <= 1e-12 and np.array_equal(a[0] > 0, b[0] > 0)


def test_triangles_cut_by_the_near_plane():
    near = 0.5
    one_behind = [(-0.6, -0.4, -1.5), (0.7, -0.5, -1.2), (0.05, 0.1, 0.8)]           # the third corner is behind the camera
    depth, _ = check_against_rays(one_behind, near=near)
    assert (depth > 0).sum() > 100 and depth[depth > 0].min() >= near - 1e-12
    two_behind = [(-0.2, -0.3, -1.5), (0.9, -0.2, 0.6), (-0.8, 0.3, 0.4)]
    depth, _ = check_against_rays(two_behind, near=near)
    assert (depth > 0).sum() > 20 and depth[depth > 0].min() >= near - 1e-12
    floor = [(-3.0, -0.05, 2.0), (3.0, -0.05, 2.0), (0.0, -0.05, -6.0)]              # a floor 5 cm under the camera
    depth, _ = check_against_rays(floor, near=0.01)
    assert (depth[CAM["H"] // 2 + 2:] > 0).mean() > 0.9 and not (depth[:CAM["H"] // 2 - 2] > 0).any()


def test_triangles_behind_the_camera_and_beyond_far_leave_nothing():
    behind = [(-1.0, -0.8, 2.0), (1.1, -0.7, 2.0), (0.1, 0.9, 2.0)]
    assert not CH.render_depth(behind, [[0, 1, 2]], EYE[None], CAM)[0].any()
    beyond = [(-5.0, -4.0, -12.0), (5.0, -4.0, -12.0), (0.0, 5.0, -12.0)]
    assert not CH.render_depth(beyond, [[0, 1, 2]], EYE[None], CAM)[0].any()
    depth, want = check_against_rays([(-5.0, -4.0, -12.0), (5.0, -4.0, -12.0), (0.0, 2.0, -3.0)])   # crosses far = 10
    assert (depth > 0).any() and depth.max() <= 10.0 and ((want == 0) & (depth == 0)).any()


def test_skipped_faces_and_lost_poses():
    v = np.array([(-1.0, -0.8, -2.0), (1.1, -0.7, -2.0), (0.1, 0.9, -2.0), (np.nan, 0, -2.0)])
    good = CH.render_depth(v, [[0, 1, 2]], EYE[None], CAM)[0]
    for faces in ([[0, 1, 4]], [[0, 1, -1]], [[0, 1, 3]], [[0, 1, 1]], [[2, 2, 2]]):
        assert not CH.render_depth(v, faces, EYE[None], CAM)[0].any(), faces
    mixed = CH.render_depth(v, [[0, 1, 4], [0, 1, 2], [0, 0, 1], [0, 1, 3]], EYE[None], CAM)[0]
    assert np.array_equal(mixed, good)
    lost = EYE.copy(); lost[1, 3] = np.nan
    both = CH.render_depth(v, [[0, 1, 2]], np.stack([lost, EYE]), CAM)[0]
    assert not both[0].any() and np.array_equal(both[1], good[0])
    ins, seen, _ = CH.visibility(v[:3], np.stack([lost, EYE]), CAM)
    assert not ins[0].any() and ins[1].all()


# ------------------------------------------------------------------------------------------------ the face rule, the compaction
def test_face_rule_and_compaction_on_a_mesh_written_out_by_hand():
    verts = np.arange(36, dtype=np.float32).reshape(12, 3)
    faces = np.array([(0, 1, 2), (2, 3, 4), (4, 5, 6), (6, 7, 8), (8, 9, 10), (1, 1, 5), (9, 10, 11), (0, 5, 9), (3, 7, 11), (2, 2, 2)])
    #                vertex: 0  1  2  3  4  5  6  7  8  9 10 11
    in_frustum = np.array([1, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 3])
    observed = np.array([0, 0, 0, 4, 0, 1, 0, 0, 0, 0, 0, 0])
    assert CH.select_faces(faces, in_frustum).tolist() == [True, False, True, False, False, True, True, True, True, False]
    keep = CH.select_faces(faces, in_frustum, observed)
    assert keep.tolist() == [False, False, True, False, False, True, False, True, True, False]
    assert CH.select_faces(faces, in_frustum, observed, th_obs=1).tolist() == [False] * 8 + [True, False]
    start = np.array([True] * 7 + [False] + [True] * 2)                      # the bounds rule took face 7 away
    assert CH.select_faces(faces, in_frustum, observed, start=start).tolist() == [False, False, True, False, False, True, False, False, True, False]
    colors = np.arange(12)[:, None] * np.ones((1, 3))
    v, f, c = CH.compact(verts, faces, keep, colors)
    # kept faces: (4 5 6), (1 1 5), (0 5 9), (3 7 11): vertices 0 1 3 4 5 6 7 9 11 stay in order -- 1 only the repeated-index face
    # refers to, and it stays, as trimesh removes unreferenced vertices BEFORE degenerate faces --, then (1 1 5) goes
    assert c[:, 0].tolist() == [0, 1, 3, 4, 5, 6, 7, 9, 11] and np.array_equal(v, verts[[0, 1, 3, 4, 5, 6, 7, 9, 11]])
    assert f.tolist() == [[3, 4, 5], [0, 4, 7], [2, 6, 8]]
    v, f = CH.compact(verts, faces, np.zeros(10, bool))
    assert v.shape == (0, 3) and f.shape == (0, 3)


# ------------------------------------------------------------------------------------------------ the C ABI, no device needed
@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from neural_graph_mapping_amd import build
        build.build(verbose=False)
    return _capi


def test_entry_points_are_declared_exported_and_additive(capi):
    hdr = open(os.path.join(ROOT, "include", "ngm_hip.h")).read()
    L = capi.lib()
    for name in ("ngm_mesh_depth", "ngm_mesh_visibility"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in capi.EXPORTED and hasattr(L, name)
    assert L.ngm_abi_version() == 11
    from neural_graph_mapping_amd import build
    assert "ngm_mesh_cull.hip" in build.SOURCES


def test_entry_points_refuse_bad_arguments_before_any_launch(capi):
    L, INV = capi.lib(), capi.NGM_E_INVALID
    p = 256                                                     # a non-NULL address: nothing below may reach the device
    big, nan = 2 ** 31, float("nan")

    def depth_args(**kw):
        a = dict(verts=p, V=4, faces=p, F=2, c2w=p, P=3, W=16, H=12, fx=10.0, fy=10.0, cx=8.0, cy=6.0, near=0.01, far=10.0, depth=p)
        a.update(kw)
        return tuple(a.values()) + (None,)

    bad = [dict(V=-1), dict(F=-1), dict(P=-1), dict(V=big), dict(F=big), dict(P=big), dict(W=0), dict(H=0), dict(W=-3), dict(near=0.0),
           dict(near=-1.0), dict(far=0.01), dict(far=0.005), dict(near=nan), dict(far=nan), dict(verts=None), dict(faces=None),
           dict(c2w=None), dict(depth=None)]
    for kw in bad:
        assert L.ngm_mesh_depth(*depth_args(**kw)) == INV, kw
        assert L.ngm_last_error().startswith(b"ngm_mesh_depth")
    assert L.ngm_mesh_depth(*depth_args(P=0, c2w=None, depth=None)) == capi.NGM_OK          # no pose: no launch
    assert L.ngm_mesh_depth(*depth_args(V=0, verts=None)) == capi.NGM_OK                      # no vertex: no launch

    def vis_args(**kw):
        a = dict(verts=p, V=4, c2w=p, P=3, W=16, H=12, fx=10.0, fy=10.0, cx=8.0, cy=6.0, depth=p, eps=0.03, nfp=3, inf=p, obs=p)
        a.update(kw)
        return tuple(a.values()) + (None,)

    bad = [dict(V=-1), dict(P=-1), dict(nfp=-1), dict(V=big), dict(P=big), dict(nfp=big), dict(W=0), dict(H=0), dict(verts=None),
           dict(c2w=None), dict(inf=None), dict(obs=None)]
    for kw in bad:
        assert L.ngm_mesh_visibility(*vis_args(**kw)) == INV, kw
        assert L.ngm_last_error().startswith(b"ngm_mesh_visibility")
    assert L.ngm_mesh_visibility(*vis_args(P=0, c2w=None, depth=None)) == capi.NGM_OK
    assert L.ngm_mesh_visibility(*vis_args(V=0, verts=None, inf=None, obs=None)) == capi.NGM_OK


def test_host_layer_refuses_cpu_tensors_and_bad_arguments(capi):
    import torch
    from neural_graph_mapping_amd import mesh as Mh
    from neural_graph_mapping_amd.renderer import Camera
    cam = Camera(16, 12, 10.0, 10.0, 8.0, 6.0, pixel_center=0.5)
    v, f, c = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.render_mesh_depth(v, f, c, cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.mesh_visibility(v, c, cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.cull_mesh(v, f, c, cam, "occlusion")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.evaluate_raw_mesh((v, f), (v, f), c, cam, "occlusion", "frustum")
    with pytest.raises(ValueError, match="Unknown culling method"):
        Mh.cull_mesh(v, f, c, cam, "nearest")
    with pytest.raises(NotImplementedError, match="mesh_alignment"):
        Mh.evaluate_raw_mesh((v, f), (v, f), c, cam, "occlusion", "frustum", mesh_alignment=True)
    with pytest.raises((RuntimeError, NotImplementedError)):           # the dispatcher itself: no CPU kernel is registered
        torch.ops.ngm355.mesh_depth(v, f, c, 16, 12, 10.0, 10.0, 8.0, 6.0, 0.01, 10.0)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.ngm355.mesh_visibility(v, c, None, 16, 12, 10.0, 10.0, 8.0, 6.0, 0.03, 1)
    assert Mh.CULLING_METHODS == ("frustum", "occlusion", "virt_cams")
    from neural_graph_mapping_amd.renderer import NeuralGraphRenderer
    assert callable(NeuralGraphRenderer.evaluate_raw_mesh)


def test_fake_tensor_shapes_of_the_two_ops(capi):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import mesh as Mh  # noqa: F401
    with FakeTensorMode():
        v, f = torch.empty(50, 3, device="cuda"), torch.empty(20, 3, dtype=torch.int64, device="cuda")
        c = torch.empty(7, 4, 4, device="cuda")
        d = torch.ops.ngm355.mesh_depth(v, f, c, 61, 47, 10.0, 10.0, 8.0, 6.0, 0.01, 10.0)
        assert d.shape == (7, 47, 61) and d.dtype == torch.float32
        for depth in (d, None):
            i, o = torch.ops.ngm355.mesh_visibility(v, c, depth, 61, 47, 10.0, 10.0, 8.0, 6.0, 0.03, 5)
            assert i.shape == (50,) and i.dtype == torch.int32 and o.shape == (50,) and o.dtype == torch.int32
