"""CPU-side checks of mesh scoring (include/ngm_hip.h ngm_surface_sample / ngm_nearest_point; mesh.sample_surface /
nearest_distances / mesh_metrics / evaluate_mesh): the host mirror tests/_mesh_metrics_host.py -- the GPU tests' yardstick --
against the reference's own numbers (fixture G27, tests/golden/make_golden_mesh_metrics.py) and against the definition of
the sampler; the C ABI's refusals, which need no device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_metrics_host as MH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_TEST_SEED = 5            # the seed tests/test_gpu_mesh_metrics.py compares face ids with
N_DRAWS = 2 ** 18


@pytest.fixture(scope="module")
def g27():
    return np.load(os.path.join(ROOT, "tests", "golden", "g27_mesh_metrics.npz"))


@pytest.fixture(scope="module")
def sampled():
    verts, faces, special = MH.sampler_test_mesh()
    return verts, faces, special, MH.sample_surface(verts, faces, N_DRAWS, GPU_TEST_SEED)


def test_mirror_metrics_reproduce_the_reference_g27(g27):
    assert int(g27["num_pairs"]) == 2
    for i in range(2):
        m = MH.metrics(g27[f"p{i}_acc_dist"], g27[f"p{i}_comp_dist"])
        for k, want in zip(MH.METRIC_KEYS, g27[f"p{i}_metrics"]):
            assert abs(m[k] - float(want)) <= 1e-6, (i, k, m[k], float(want))
    # odd and even counts on either side: both branches of np.median
    assert {len(g27["p0_acc_dist"]) % 2, len(g27["p0_comp_dist"]) % 2} == {0, 1}
    assert {len(g27["p1_acc_dist"]) % 2, len(g27["p1_comp_dist"]) % 2} == {0, 1}


def test_mirror_distances_reproduce_the_kdtree_g27(g27):
    for i in range(2):
        gt, est = g27[f"p{i}_gt"], g27[f"p{i}_est"]
        assert gt.dtype == np.float32 and est.dtype == np.float32
        d_acc, i_acc = MH.nearest(est, gt)
        d_comp, i_comp = MH.nearest(gt, est)
        assert np.abs(d_acc - g27[f"p{i}_acc_dist"]).max() <= 1e-9
        assert np.abs(d_comp - g27[f"p{i}_comp_dist"]).max() <= 1e-9
        assert np.abs(MH.distance_to(est, gt, i_acc) - d_acc).max() == 0


def test_g27_ratios_are_strict_and_no_distance_sits_on_a_threshold(g27):
    """the GPU test holds mesh_metrics to the recorded ratios at 1e-6: exact unless an fp32 distance (bar 2^-21 relative) can
    fall on the other side of 0.05 / 0.01"""
    for i in range(2):
        m = dict(zip(MH.METRIC_KEYS, g27[f"p{i}_metrics"]))
        for k in ("acc_ratio", "acc_ratio_1cm", "comp_ratio", "comp_ratio_1cm"):
            assert 0.0 < m[k] < 1.0
        for d in (g27[f"p{i}_acc_dist"], g27[f"p{i}_comp_dist"]):
            for th in (0.05, 0.01):
                assert np.abs(d - th).min() > 2.0 ** -21 * th * (1 + 2.0 ** -20)


def test_mirror_metrics_f1_is_zero_where_a_ratio_is_zero():
    m = MH.metrics(np.full(10, 0.03), np.full(7, 0.03))
    assert m["acc_ratio"] == 1.0 and m["acc_ratio_1cm"] == 0.0 and m["f1_5cm"] == 1.0 and m["f1_1cm"] == 0.0
    assert m["median_acc"] == pytest.approx(0.03) and m["median_comp"] == pytest.approx(0.03)


def test_mirror_nearest_non_finite_rules():
    refs = np.array([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0]], np.float32)
    q = np.array([[0.9, 0, 0], [np.nan, 0, 0], [-5, 0, 0], [0, -np.inf, 0]], np.float32)
    d, i = MH.nearest(q, refs)
    assert i.tolist() == [2, -1, 0, -1] and np.isnan(d[1]) and np.isnan(d[3]) and d[2] == 5.0
    d, i = MH.nearest(q, refs[[1, 3]])
    assert i.tolist() == [-1] * 4 and np.isinf(d[0]) and np.isnan(d[1]) and np.isinf(d[2])


def test_mirror_sampler_points_lie_in_their_faces(sampled):
    verts, faces, _, s = sampled
    p = verts[faces[s["face_ids"]]].astype(np.float64)
    e1, e2, w = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], s["points"] - p[:, 0]
    n = np.cross(e1, e2)
    nn = np.linalg.norm(n, axis=1)
    assert np.abs((w * n).sum(1) / nn).max() <= 1e-9                                   # in the plane
    # barycentric coordinates from the 2 x 2 normal equations
    a, b, c = (e1 * e1).sum(1), (e1 * e2).sum(1), (e2 * e2).sum(1)
    r1, r2 = (w * e1).sum(1), (w * e2).sum(1)
    det = a * c - b * b
    u, v = (c * r1 - b * r2) / det, (a * r2 - b * r1) / det
    assert min(u.min(), v.min(), (1 - u - v).min()) >= -1e-9
    assert np.abs(u - s["uv"][:, 0]).max() < 1e-6 and np.abs(v - s["uv"][:, 1]).max() < 1e-6


def test_mirror_sampler_never_draws_a_face_without_area(sampled):
    verts, faces, special, s = sampled
    area = s["area"]
    assert len(faces) == 101 and area.max() / area[area > 0].min() > 900            # ~100 faces, areas 1 : 1000
    for name, f in special.items():
        assert area[f] == 0.0, name
    assert (area[s["face_ids"]] > 0).all() and s["face_ids"].min() >= 0
    assert not np.isin(s["face_ids"], list(special.values())).any()


def test_mirror_sampler_draws_faces_in_proportion_to_area(sampled):
    """six binomial standard deviations per face; deterministic, the stream is seeded"""
    _, faces, _, s = sampled
    p = s["area"] / s["total"]
    count = np.bincount(s["face_ids"], minlength=len(faces))
    bound = 6 * np.sqrt(N_DRAWS * p * (1 - p)) + 1
    worst = np.abs(count - N_DRAWS * p) / bound
    assert worst.max() <= 1.0, (int(worst.argmax()), float(worst.max()))


def test_mirror_sampler_boundary_share_is_below_the_gpu_tests_cap(sampled):
    """the GPU test may leave out draws within 1e-5 of the total area of a cumulative-area boundary, at most 1 %"""
    share = float((sampled[3]["boundary_gap"] <= 1e-5).mean())
    assert share < 0.01, share


def test_mirror_sampler_degenerate_meshes_and_seeds():
    verts, faces, special = MH.sampler_test_mesh()
    s = MH.sample_surface(verts, faces[list(special.values())], 33, 1)
    assert np.isnan(s["points"]).all() and (s["face_ids"] == -1).all()
    a, b = MH.sample_surface(verts, faces, 64, 1), MH.sample_surface(verts, faces, 64, 2)
    assert not np.array_equal(a["points"], b["points"])
    assert np.array_equal(a["points"], MH.sample_surface(verts, faces, 64, 1)["points"])
    assert np.array_equal(a["points"][:10], MH.sample_surface(verts, faces, 10, 1)["points"])      # a function of (seed, index)
    one = MH.sample_surface(verts, faces[:1], 100, 3)
    assert (one["face_ids"] == 0).all()


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
    for name in ("ngm_surface_sample_workspace", "ngm_surface_sample", "ngm_nearest_point_workspace", "ngm_nearest_point"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in capi.EXPORTED and hasattr(L, name)
    assert L.ngm_abi_version() == 11
    from neural_graph_mapping_amd import build
    assert "ngm_mesh_eval.hip" in build.SOURCES


def test_entry_points_refuse_bad_arguments_before_any_launch(capi):
    L, INV = capi.lib(), capi.NGM_E_INVALID
    p = 256                                                     # a non-NULL address: nothing below may reach the device
    big = 2 ** 31
    assert L.ngm_surface_sample_workspace(0) == INV and L.ngm_surface_sample_workspace(-1) == INV
    assert L.ngm_surface_sample_workspace(big) == INV and L.ngm_surface_sample_workspace(100) > 800
    assert L.ngm_nearest_point_workspace(0, 5) == INV and L.ngm_nearest_point_workspace(5, -1) == INV
    assert L.ngm_nearest_point_workspace(big, 5) == INV and L.ngm_nearest_point_workspace(5, big) == INV
    assert L.ngm_nearest_point_workspace(1000, 0) >= 16 * 1000
    ws = L.ngm_surface_sample_workspace(10)
    bad = [(p, 4, p, 0, 8, 0, p, p, p, ws, None),               # no faces
           (p, 4, p, -1, 8, 0, p, p, p, ws, None), (p, -4, p, 10, 8, 0, p, p, p, ws, None), (p, 4, p, 10, -8, 0, p, p, p, ws, None),
           (p, 4, p, 10, big, 0, p, p, p, ws, None), (p, big, p, 10, 8, 0, p, p, p, ws, None),
           (None, 4, p, 10, 8, 0, p, p, p, ws, None), (p, 4, None, 10, 8, 0, p, p, p, ws, None),
           (p, 4, p, 10, 8, 0, None, p, p, ws, None), (p, 4, p, 10, 8, 0, p, None, p, ws, None),
           (p, 4, p, 10, 8, 0, p, p, None, ws, None), (p, 4, p, 10, 8, 0, p, p, p, ws - 1, None)]
    for args in bad:
        assert L.ngm_surface_sample(*args) == INV, args
        assert L.ngm_last_error().startswith(b"ngm_surface_sample")
    assert L.ngm_surface_sample(p, 4, p, 10, 0, 0, None, None, p, ws, None) == capi.NGM_OK       # nothing to draw: no launch
    ws = L.ngm_nearest_point_workspace(10, 8)
    bad = [(p, 0, p, 8, p, p, p, ws, None), (p, -1, p, 8, p, p, p, ws, None), (p, 10, p, -8, p, p, p, ws, None),
           (p, big, p, 8, p, p, p, ws, None), (p, 10, p, big, p, p, p, ws, None),
           (None, 10, p, 8, p, p, p, ws, None), (p, 10, None, 8, p, p, p, ws, None), (p, 10, p, 8, None, p, p, ws, None),
           (p, 10, p, 8, p, None, p, ws, None), (p, 10, p, 8, p, p, None, ws, None), (p, 10, p, 8, p, p, p, ws - 1, None)]
    for args in bad:
        assert L.ngm_nearest_point(*args) == INV, args
        assert L.ngm_last_error().startswith(b"ngm_nearest_point")
    assert L.ngm_nearest_point(p, 10, None, 0, None, None, p, ws, None) == capi.NGM_OK           # no query: no launch


def test_host_layer_refuses_cpu_tensors_and_bad_shapes(capi):
    import torch
    from neural_graph_mapping_amd import mesh as Mh
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.sample_surface(v, f, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.nearest_distances(v, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.mesh_metrics(v, v)
    with pytest.raises((RuntimeError, NotImplementedError)):           # the dispatcher itself: no CPU kernel is registered
        torch.ops.ngm355.nearest_point(v, v)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.ngm355.surface_sample(v, f, 4, 0)
    assert Mh.METRIC_KEYS == MH.METRIC_KEYS


def test_fake_tensor_shapes_of_the_two_ops(capi):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import mesh as Mh  # noqa: F401
    with FakeTensorMode():
        v, f = torch.empty(50, 3, device="cuda"), torch.empty(20, 3, dtype=torch.int64, device="cuda")
        p, ids = torch.ops.ngm355.surface_sample(v, f, 77, 3)
        assert p.shape == (77, 3) and p.dtype == torch.float32 and ids.shape == (77,) and ids.dtype == torch.int64
        d, i = torch.ops.ngm355.nearest_point(torch.empty(31, 3, device="cuda"), v)
        assert d.shape == (31,) and d.dtype == torch.float32 and i.shape == (31,) and i.dtype == torch.int64
