"""CPU-side checks of mesh subdivision (include/ngm_hip.h ngm_mesh_subdivide_*; mesh.subdivide_to_size, cull_mesh(max_edge=...)):
the two host mirrors of tests/_mesh_subdivide_host.py -- trimesh's loop restated, and the closed form the kernels implement, the GPU
tests' yardstick -- give the same triangles; the ops, the C ABI and the host layer refuse what they must without a device."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_subdivide_host as SH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the two mirrors
@pytest.mark.parametrize("max_edge", [0.125, 0.37109375, 5.0])
def test_closed_form_gives_the_triangles_of_the_iterative_loop(max_edge):
    v, f = SH.random_mesh(10, 11)
    sv, sf = SH.special_faces(max_edge)
    verts, faces = np.concatenate([v, sv]), np.concatenate([f, sf + len(v)])
    lengths = SH.edge_lengths(verts.astype(np.float64), faces).max(1)
    assert lengths[-2] == max_edge and lengths[-1] == 2 * max_edge                       # exactly at the rule's two boundaries
    want_soup, want_parent = SH.iterative(verts, faces, max_edge)
    got = SH.closed_form(verts, faces, max_edge)
    assert got["levels"][-3:].tolist() == [0, 0, 1]
    if max_edge < 1:
        assert got["levels"].max() >= 2 and len(np.unique(got["levels"])) >= 3
    else:
        assert not got["levels"][:-1].any()
    assert len(got["soup"]) == len(want_soup) == (4 ** got["levels"]).sum()
    assert np.array_equal(np.bincount(got["parent"], minlength=len(faces)), np.bincount(want_parent, minlength=len(faces)))
    a, oa = SH.canonical(got["soup"], decimals=7)
    b, ob = SH.canonical(want_soup, decimals=7)
    assert np.abs(a - b).max() <= 1e-9
    assert np.array_equal(got["parent"][oa], want_parent[ob])
    # the indexed mesh is its own soup; the inputs stay in place
    assert np.array_equal(got["verts"][:len(verts)], verts.astype(np.float64))
    assert np.array_equal(got["verts"][got["faces"]], got["soup"])


def test_closed_form_accepts_exactly_max_iter_and_refuses_one_more():
    v = np.array([(0, 0, 0), (8, 0, 0), (0, 3, 0)], np.float32)                          # longest edge sqrt(73): level 7 at 0.1
    f = np.array([(0, 1, 2)], np.int64)
    assert SH.levels(v, f, 0.1).tolist() == [7]
    assert SH.levels(v, f, 0.1, max_iter=7).tolist() == [7] and SH.levels(v, f, 0.1, max_iter=6).tolist() == [7]
    assert len(SH.closed_form(v, f, 0.1, max_iter=7)["faces"]) == 4 ** 7
    assert len(SH.iterative(v, f, 0.1, max_iter=7)[0]) == 4 ** 7
    for fn in (SH.closed_form, SH.iterative):
        with pytest.raises(ValueError, match="max_iter exceeded"):
            fn(v, f, 0.1, max_iter=6)
    bad = np.array([(0, 0, 0), (np.inf, 0, 0), (0, 1, 0), (np.nan, 0, 0)], np.float32)
    assert SH.levels(bad, [(0, 1, 2)], 0.1).tolist() == [11] and SH.levels(bad, [(0, 2, 3)], 0.1).tolist() == [0]
    assert SH.levels(bad, [(0, 2, 4), (0, -1, 2)], 0.1).tolist() == [0, 0]


def test_lattice_order_is_the_documented_one():
    ij, tri = SH.lattice(2)
    assert ij.tolist() == [[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [0, 2]]
    assert tri.tolist() == [[0, 1, 3], [1, 4, 3], [1, 2, 4], [3, 4, 5]]
    for n in (1, 4, 8):
        ij, tri = SH.lattice(n)
        assert len(ij) == (n + 1) * (n + 2) // 2 and len(tri) == n * n
        p = ij[tri].astype(np.float64)
        cross = (p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0])
        assert np.array_equal(cross, np.ones(n * n))                                     # every child: the parent's winding, equal area


# ------------------------------------------------------------------------------------------------ the C ABI, no device needed
@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi
    if not os.path.exists(_capi.LIB_PATH):
        from neural_graph_mapping_amd import build
        build.build(verbose=False)
    return _capi


NAMES = ("ngm_mesh_subdivide_workspace", "ngm_mesh_subdivide_count", "ngm_mesh_subdivide_emit")


def test_entry_points_are_declared_exported_and_additive(capi):
    hdr = open(os.path.join(ROOT, "include", "ngm_hip.h")).read()
    L = capi.lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in capi.EXPORTED and hasattr(L, name)
        assert getattr(L, name).argtypes is not None
    assert L.ngm_abi_version() == 11
    assert len(L.ngm_mesh_subdivide_count.argtypes) == 10 and len(L.ngm_mesh_subdivide_emit.argtypes) == 14
    import ctypes as C
    assert L.ngm_mesh_subdivide_count.argtypes[4] is C.c_double and L.ngm_mesh_subdivide_workspace.restype is C.c_int64


def test_workspace_holds_the_levels_and_the_two_scans(capi):
    L = capi.lib()
    for nf in (0, 1, 63, 2048, 2049, 5_000_000):
        assert L.ngm_mesh_subdivide_workspace(nf) >= 4 * nf + 2 * 8 * (nf + 1)
    assert L.ngm_mesh_subdivide_workspace(-1) == capi.NGM_E_INVALID and L.ngm_mesh_subdivide_workspace(2 ** 31) == capi.NGM_E_INVALID


def test_entry_points_refuse_bad_arguments_before_any_launch(capi):
    L, INV, UNS = capi.lib(), capi.NGM_E_INVALID, capi.NGM_E_UNSUPPORTED
    p, big, nan, inf = 256, 2 ** 31, float("nan"), float("inf")                          # p: a non-NULL address nothing may reach
    wsb = L.ngm_mesh_subdivide_workspace(2)

    def count_args(**kw):
        a = dict(verts=p, V=4, faces=p, F=2, max_edge=0.1, max_iter=10, ws=p, wsb=wsb, totals=p)
        a.update(kw)
        return tuple(a.values()) + (None,)

    bad = [dict(V=-1), dict(F=-1), dict(V=big), dict(F=big), dict(max_edge=0.0), dict(max_edge=-1.0), dict(max_edge=nan), dict(max_edge=inf),
           dict(max_iter=-1), dict(max_iter=11), dict(verts=None), dict(faces=None), dict(ws=None), dict(totals=None), dict(wsb=wsb - 1), dict(wsb=0)]
    for kw in bad:
        assert L.ngm_mesh_subdivide_count(*count_args(**kw)) == INV, kw
        assert L.ngm_last_error().startswith(b"ngm_mesh_subdivide_count")

    def emit_args(**kw):
        a = dict(verts=p, V=4, faces=p, F=2, attrs=None, C=0, ws=p, new_vertices=3, out_faces=5, out_verts=p, out_faces_idx=p, out_attrs=None,
                 out_parent=p)
        a.update(kw)
        return tuple(a.values()) + (None,)

    bad = [dict(V=-1), dict(F=-1), dict(new_vertices=-1), dict(out_faces=-1), dict(C=-1), dict(V=big), dict(F=big), dict(verts=None), dict(faces=None),
           dict(ws=None), dict(out_verts=None), dict(out_faces_idx=None), dict(out_parent=None), dict(attrs=p, C=3, out_attrs=None),
           dict(F=0, faces=None, ws=None)]
    for kw in bad:
        assert L.ngm_mesh_subdivide_emit(*emit_args(**kw)) == INV, kw
        assert L.ngm_last_error().startswith(b"ngm_mesh_subdivide_emit")
    for kw in (dict(new_vertices=big - 4), dict(out_faces=big), dict(attrs=p, C=3, out_attrs=p, new_vertices=big // 3)):
        assert L.ngm_mesh_subdivide_emit(*emit_args(**kw)) == UNS, kw                   # totals of 2^31 or more: refused, nothing launched
        assert L.ngm_last_error().startswith(b"ngm_mesh_subdivide_emit")


# ------------------------------------------------------------------------------------------------ ops and host layer
def test_ops_exist_with_fake_shapes_and_no_cpu_kernel(capi):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import mesh as Mh  # noqa: F401
    assert hasattr(torch.ops.ngm355, "mesh_subdivide_count") and hasattr(torch.ops.ngm355, "mesh_subdivide_emit")
    L = capi.lib()
    with FakeTensorMode():
        for nf in (1, 20, 2049):
            v, f = torch.empty(50, 3, device="cuda"), torch.empty(nf, 3, dtype=torch.int64, device="cuda")
            totals, ws = torch.ops.ngm355.mesh_subdivide_count(v, f, 0.1, 10)
            assert totals.shape == (3,) and totals.dtype == torch.int64
            assert ws.dtype == torch.uint8 and ws.shape == (L.ngm_mesh_subdivide_workspace(nf),)
            for attrs, c in ((None, 0), (torch.empty(50, 4, device="cuda"), 4)):
                ov, of, oa, par = torch.ops.ngm355.mesh_subdivide_emit(v, f, attrs, ws, 70, 90)
                assert ov.shape == (120, 3) and ov.dtype == torch.float32 and of.shape == (90, 3) and of.dtype == torch.int64
                assert oa.shape == (120, c) and oa.dtype == torch.float32 and par.shape == (90,) and par.dtype == torch.int64
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises((RuntimeError, NotImplementedError)):                             # the dispatcher itself: no CPU kernel
        torch.ops.ngm355.mesh_subdivide_count(v, f, 0.1, 10)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.ngm355.mesh_subdivide_emit(v, f, None, torch.zeros(1024, dtype=torch.uint8), 0, 1)


def test_host_layer_refuses_cpu_tensors_and_bad_arguments_before_any_launch(capi, monkeypatch):
    import torch
    from neural_graph_mapping_amd import mesh as Mh
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.subdivide_to_size(v, f, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.subdivide_to_size(v, f, 0.1, attrs=torch.zeros(3, 2))

    # the argument checks, with the device test out of the way: whatever reaches a launch fails the test
    def no_launch(*a, **k):
        raise AssertionError("a launch was reached")
    monkeypatch.setattr(Mh.ops, "_require_gpu", lambda *t: None)
    monkeypatch.setattr(Mh.K, "lib", no_launch)
    nan, inf = float("nan"), float("inf")
    for max_edge in (0.0, -0.1, nan, inf, -inf, None, "0.1", True):
        with pytest.raises(ValueError, match="max_edge"):
            Mh.subdivide_to_size(v, f, max_edge)
    for max_iter in (-1, 11, 100, 2.5, None, True):
        with pytest.raises(ValueError, match="max_iter"):
            Mh.subdivide_to_size(v, f, 0.1, max_iter=max_iter)
    for bad_v in (torch.zeros(3, 2), torch.zeros(3), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float16)):
        with pytest.raises(ValueError, match="vertices"):
            Mh.subdivide_to_size(bad_v, f, 0.1)
    for bad_f in (torch.zeros(1, 4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 3)):
        with pytest.raises(ValueError, match="faces"):
            Mh.subdivide_to_size(v, bad_f, 0.1)
    for bad_a in (torch.zeros(2, 3), torch.zeros(3), torch.zeros(3, 2, dtype=torch.float64), torch.zeros(3, 2, 2)):
        with pytest.raises(ValueError, match="attrs"):
            Mh.subdivide_to_size(v, f, 0.1, attrs=bad_a)
    assert Mh.SUBDIVIDE_MAX_ITER == 10


def test_cull_mesh_keywords_and_the_statements_that_went(capi):
    import torch
    from neural_graph_mapping_amd import mesh as Mh
    from neural_graph_mapping_amd.renderer import Camera
    sig = inspect.signature(Mh.cull_mesh)
    assert sig.parameters["max_edge"].default is None and sig.parameters["max_iter"].default == 10
    sig = inspect.signature(Mh.subdivide_to_size)
    assert list(sig.parameters) == ["verts", "faces", "max_edge", "max_iter", "attrs", "return_index"]
    assert sig.parameters["max_iter"].default == 10 and sig.parameters["attrs"].default is None and sig.parameters["return_index"].default is False
    cam = Camera(16, 12, 10.0, 10.0, 8.0, 6.0, pixel_center=0.5)
    v, f, c = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.eye(4)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.cull_mesh(v, f, c, cam, "occlusion", max_edge=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mh.evaluate_raw_mesh((v, f), (v, f), c, cam, "occlusion", "frustum", max_edge=0.1)
    with pytest.raises(NotImplementedError, match="mesh_alignment"):
        Mh.evaluate_raw_mesh((v, f), (v, f), c, cam, "occlusion", "frustum", mesh_alignment=True, max_edge=0.1)
    # nowhere does the code or a document still say that subdivision is the caller's job
    stale = re.compile(r"subdivide_to_size is not built|NOT BUILT: subdivide_to_size|fine enough|subdivision are the caller's|and subdivision out of scope",
                       re.I)
    for rel in ("neural_graph_mapping_amd/mesh.py", "include/ngm_hip.h", "DESIGN.md", "README.md", "INTEGRATION.md"):
        assert not stale.search(open(os.path.join(ROOT, rel)).read()), rel
