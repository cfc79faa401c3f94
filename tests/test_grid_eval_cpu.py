"""CPU-side checks of the lattice entry point (ngm_grid_eval_knn: one block of the mesh grid as one call) and of the
block reachability test of mesh.extract_mesh: symbols, op registration and fake shape, workspace planner, every
validation code (all of them are returned before any launch, so they are reachable with no device), and
`mesh.reachable_blocks` against brute force.  No compute calls here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngm_hip.h")


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def test_symbols_in_header_capi_and_library(capi):
    head = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = capi.lib()
    for n in ("ngm_grid_eval_knn", "ngm_grid_eval_knn_workspace"):
        assert re.search(r"\b" + n + r"\s*\(", head), n
        assert n in capi.EXPORTED and hasattr(L, n), n
    assert L.ngm_grid_eval_knn_workspace.restype is C.c_int64 and len(L.ngm_grid_eval_knn.argtypes) == 21


def test_op_is_registered_with_a_lattice_shaped_fake_and_no_cpu_kernel(capi):
    from neural_graph_mapping_amd import ops
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert hasattr(torch.ops.ngm355, "grid_eval_knn")
    fc = capi.field_cfg(encoding="nerf", num_octaves=2, num_layers=1, dim_hidden=16)
    blob = ops.cfg_blob(fc)
    with FakeTensorMode(allow_non_fake_inputs=True):                    # (the configuration blob is a real CPU tensor)
        dev = "cuda"
        xs, ys, zs = (torch.empty(n, device=dev) for n in (5, 1, 7))
        params = [torch.empty(3, *s, device=dev) for s in capi.param_shapes(fc).values()]
        out = torch.ops.ngm355.grid_eval_knn(blob, xs, ys, zs, torch.empty(3, 3, device=dev), torch.empty(3, 4, device=dev),
                                             params, 2, 10.0, 1.0, None, 0.0, 3, True)
        assert tuple(out.shape) == (5, 1, 7) and out.dtype == torch.float32
    # ROCm kernel only, like its neighbours: CPU tensors are refused, by the wrapper and by the dispatcher
    p = {n: torch.zeros(3, *s) for n, s in capi.param_shapes(fc).items()}
    ax = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grid_eval_knn(fc, p, ax, ax, ax, torch.zeros(3, 3), torch.zeros(3, 4))
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.ngm355.grid_eval_knn(blob, ax, ax, ax, torch.zeros(3, 3), torch.zeros(3, 4), list(p.values()), 2, 10.0, 1.0,
                                       None, 0.0, 3, False)


def test_workspace_is_monotone_and_never_above_the_point_entrys(capi):
    L = capi.lib()
    ws = L.ngm_grid_eval_knn_workspace
    base = ws(50, 17, 13, 11, 2)
    assert base > 0
    assert ws(50, 18, 13, 11, 2) > base and ws(50, 17, 14, 11, 2) > base and ws(50, 17, 13, 12, 2) > base
    assert ws(50, 17, 13, 11, 3) > base > ws(50, 17, 13, 11, 1)
    for nf, nx, ny, nz, k in ((50, 17, 13, 11, 2), (1, 1, 1, 1, 1), (3000, 24, 24, 24, 1), (7, 201, 201, 201, 2), (7, 5, 1, 64, 16),
                              (3, 5, 5, 5, 9)):            # (K is capped by the number of fields in both)
        assert 0 < ws(nf, nx, ny, nz, k) <= L.ngm_field_eval_knn_workspace(nf, nx * ny * nz, k), (nf, nx, ny, nz, k)
    # the planner returns the call's own codes
    assert ws(50, 0, 13, 11, 2) == capi.NGM_E_INVALID and ws(50, 17, -1, 11, 2) == capi.NGM_E_INVALID
    assert ws(0, 17, 13, 11, 2) == capi.NGM_E_UNSUPPORTED and ws(50, 17, 13, 11, 0) == capi.NGM_E_UNSUPPORTED
    assert ws(50, 1291, 1291, 1291, 1) == capi.NGM_E_UNSUPPORTED           # 1291^3 = 2 151 685 171 > 2^31 - 1
    assert ws(50, 1290, 1290, 1290, 1) > 0                                   # 1290^3 = 2 146 689 000 fits
    assert ws(50, 1024, 1024, 1024, 2) == capi.NGM_E_UNSUPPORTED           # 2^30 points, K = 2: exactly 2^31
    assert ws(50, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 16) == capi.NGM_E_UNSUPPORTED     # no overflow on the way


def test_every_validation_code_without_a_device(capi):
    """NGM_E_INVALID / NGM_E_UNSUPPORTED / NGM_E_WORKSPACE are decided before any launch: the pointers below are never read."""
    L = capi.lib()
    fc = capi.field_cfg(encoding="nerf", num_octaves=2, num_layers=1, dim_hidden=16)
    fake = 0x1000                                                       # a non-NULL address nothing dereferences on these paths
    ptrs = {n: fake for n in capi.param_shapes(fc)}
    ps = capi.params_struct(fc, ptrs, {n: 1 for n in ptrs}, None, 0)
    NF, shape, K_ = 7, (5, 4, 3), 2
    need = L.ngm_grid_eval_knn_workspace(NF, *shape, K_)

    def call(nf=NF, pos=fake, quat=fake, xs=fake, nx=shape[0], ys=fake, ny=shape[1], zs=fake, nz=shape[2], k=K_, channel=3,
             vol=fake, ws=fake, wsb=need):
        return L.ngm_grid_eval_knn(C.byref(fc), C.byref(ps), nf, pos, quat, xs, nx, ys, ny, zs, nz, k, 10.0, 1.0, 0.0, channel, 0,
                                   vol, ws, wsb, None)

    for kw in (dict(nx=0), dict(ny=0), dict(nz=-3), dict(xs=None), dict(ys=None), dict(zs=None), dict(vol=None), dict(channel=-1),
               dict(channel=4), dict(pos=None), dict(quat=None)):
        assert call(**kw) == capi.NGM_E_INVALID, kw
        assert L.ngm_last_error().decode().startswith("ngm_grid_eval_knn"), kw
    for kw in (dict(nf=0), dict(nx=1024, ny=1024, nz=1024), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), dict(k=0),
               dict(nf=40, k=17)):
        assert call(**kw) == capi.NGM_E_UNSUPPORTED, kw
    for kw in (dict(wsb=need - 1), dict(wsb=0), dict(ws=None)):
        assert call(**kw) == capi.NGM_E_WORKSPACE, kw
    # the configuration is checked first, as in every entry point
    assert L.ngm_grid_eval_knn(None, C.byref(ps), NF, fake, fake, fake, 5, fake, 4, fake, 3, K_, 10.0, 1.0, 0.0, 3, 0, fake, fake,
                               need, None) == capi.NGM_E_INVALID


def _brute_blocks(axes, block, pos, radius):
    """blocks that hold a lattice point within `radius` of a centre, in fp64"""
    starts = [range(0, len(a) - 1, block) for a in axes]
    out = torch.zeros([len(s) for s in starts], dtype=torch.bool)
    c = pos.double()
    for i, xs in enumerate(starts[0]):
        for j, ys in enumerate(starts[1]):
            for k, zs in enumerate(starts[2]):
                pts = torch.cartesian_prod(axes[0][xs:xs + block + 1], axes[1][ys:ys + block + 1], axes[2][zs:zs + block + 1]).double()
                out[i, j, k] = bool((torch.cdist(pts, c) < radius).any())
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reachable_blocks_has_no_false_negative(seed):
    from neural_graph_mapping_amd import mesh
    g = torch.Generator().manual_seed(seed)
    radius = float(0.2 + 0.6 * torch.rand((), generator=g))
    nf = int(torch.randint(1, 9, (), generator=g))
    pos = (torch.rand(nf, 3, generator=g) - 0.5) * 6 + (100.0 if seed == 5 else 0.0)       # (far from the origin: coarser fp32)
    res = float(0.08 + 0.2 * torch.rand((), generator=g))
    block = int(torch.randint(3, 9, (), generator=g))
    axes = mesh.grid_axes(pos, radius, res)
    if seed % 2:                                                        # non-uniform (still ascending) axes
        axes = [a + 0.3 * res * (torch.rand(a.shape, generator=g) - 0.5) for a in axes]
    got = mesh.reachable_blocks(axes, block, pos, radius)
    want = _brute_blocks(axes, block, pos, radius)
    assert got.shape == want.shape and got.dtype == torch.bool
    assert not bool((want & ~got).any()), "a block with a point inside a field is not marked"
    assert bool(got.any())
    print(f"reachable_blocks seed {seed}: {int(got.sum())} of {got.numel()} marked, {int((got & ~want).sum())} of them hold no inside point")


def test_reachable_blocks_two_clusters_leave_most_of_the_box_unmarked():
    from neural_graph_mapping_amd import mesh
    g = torch.Generator().manual_seed(0)
    pos = torch.cat([torch.rand(3, 3, generator=g) * 0.5, torch.rand(3, 3, generator=g) * 0.5 + torch.tensor([9.0, 0.0, 0.0])])
    axes = mesh.grid_axes(pos, 0.5, 0.1)
    got = mesh.reachable_blocks(axes, 16, pos, 0.5)
    assert 0 < int(got.sum()) < got.numel() // 2
    assert not bool((_brute_blocks(axes, 16, pos, 0.5) & ~got).any())


def test_reachable_blocks_one_point_axis_has_no_block():
    """the block loop runs range(0, len(axis) - 1, block) per axis: an axis of one point has no block, and neither has the result"""
    from neural_graph_mapping_amd import mesh
    pos = torch.zeros(2, 3)
    ax = torch.arange(-1.0, 1.0, 0.1)
    got = mesh.reachable_blocks([ax, torch.tensor([0.0]), ax], 8, pos, 0.5)
    assert tuple(got.shape) == (3, 0, 3) and got.dtype == torch.bool
    assert tuple(mesh.reachable_blocks([ax, ax[:2], ax], 8, pos, 0.5).shape) == (3, 1, 3)
