"""-m gpu: the lattice entry point (ngm_grid_eval_knn / ops.grid_eval_knn: one block of the mesh grid as one call) and
mesh.extract_mesh(fused=True) on top of it.

Everything here is compared BIT FOR BIT (torch.equal) with the staged path the project already had -- ops.field_eval_knn on
torch.cartesian_prod of the axes, mesh.extract_mesh(fused=False) -- never with the code under test: the fused path forms
the very floats of the axes inside the kernels and accumulates the blend with the same fmaf chain, so there is no
tolerance to choose.  The staged path itself is held to the oracle by test_gpu_mesh.py / test_gpu_hardening.py."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import DEV, cu, make_renderer  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import mesh as Mh  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

M1 = dict(encoding="fourier", dim_enc=64, num_layers=2)
HASH = dict(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
NERF16 = dict(encoding="nerf", num_octaves=2, num_layers=1, dim_hidden=16)                       # 12 -> 16, one layer
TRIPLANE = dict(encoding="triplane", num_components=64, resolution=16, tri_mode="sum", num_layers=3)
CONCAT = dict(encoding="fourier", dim_enc=40, num_layers=2, dim_hidden=64, skip_mode="concat")
# name -> (field kwargs, matmul mode, K, storage type)
NETS = {
    "m1_k2": (M1, "auto", 2, None),
    "hash_default_k2": (HASH, "auto", 2, None),
    "nerf_12to16_k1": (NERF16, "auto", 1, None),
    "triplane_k3": (TRIPLANE, "auto", 3, None),
    "fourier_concat_k9": (CONCAT, "auto", 9, None),
    "m1_bf16_storage": (M1, "auto", 2, torch.bfloat16),
    "m1_matmul_f32": (M1, "f32", 2, None),
}
SHAPES = [(17, 13, 11), (33, 2, 9), (5, 1, 64), (128, 128, 65), (1, 1, 5)]
_CACHE = {}


def layout(NF=7):
    """NF fields of radius 1 at (rand - 0.5) * 3 (generator seed 0), random unit quaternions"""
    g = torch.Generator().manual_seed(0)
    pos = (torch.rand(NF, 3, generator=g) - 0.5) * 3
    quat = torch.nn.functional.normalize(torch.randn(NF, 4, generator=g), dim=-1)
    return pos.to(DEV), quat.to(DEV)


def axis(n):
    return torch.tensor([0.1], device=DEV) if n == 1 else torch.linspace(-1.8, 1.8, n, device=DEV)


def network(name, NF=7):
    key = (name, NF)
    if key not in _CACHE:
        fkw, mode, K_, dt = NETS[name]
        fs = O.FieldSpec(**fkw)
        params = O.init_params(fs, NF, seed=11, sigma=3.0)
        if fkw["encoding"] == "permuto":               # (the reference initialises the table at 1e-5: give it something to blend)
            g = torch.Generator().manual_seed(3)
            params["_encoding.lattice_values"] += 0.1 * torch.randn(params["_encoding.lattice_values"].shape, generator=g)
        if dt is not None:
            params = {k: (v if k in K.NO_GRAD_PARAMS else v.to(dt)) for k, v in params.items()}
        _CACHE[key] = (K.field_cfg(**fkw, matmul_mode=mode), cu(params), K_)
    return _CACHE[key]


def inside_share(xs, ys, zs, pos, radius=1.0):
    pts = torch.cartesian_prod(xs, ys, zs).view(-1, 3)
    return float((torch.cdist(pts.double(), pos.double()).min(1)[0] < radius).double().mean())


def check_against_staged(fc, params, K_, xs, ys, zs, pos, quat, field_index=None, mask_radius=None, share=(0.05, 0.95)):
    """all four channels, plain and negated, against ONE staged evaluation of the lattice's points"""
    n = (len(xs), len(ys), len(zs))
    pts = torch.cartesian_prod(xs, ys, zs).view(-1, 3)
    ref = ops.field_eval_knn(fc, params, pts, pos, quat, K_, 10.0, 1.0, field_index, mask_radius)
    s = inside_share(xs, ys, zs, pos, mask_radius or 1.0)
    print(f"lattice {n}: {pts.shape[0]} points, inside share {s:.3f}")
    if pts.shape[0] >= 500:
        assert share[0] <= s <= share[1], s                # an all-outside (or all-inside) grid proves nothing
        assert bool((ref != 1.0).any()) and bool((ref == 1.0).all(-1).any())
    for c in range(4):
        for neg in (False, True):
            vol = ops.grid_eval_knn(fc, params, xs, ys, zs, pos, quat, K_, 10.0, 1.0, field_index, mask_radius, channel=c, negate=neg)
            want = ref[:, c].reshape(n)
            assert vol.shape == n and vol.is_contiguous()
            assert torch.equal(vol, -want if neg else want), (n, c, neg, int((vol != (-want if neg else want)).sum()))
    return ref


# ------------------------------------------------------------------------------------------------ bitwise equality with the staged entry
@pytest.mark.parametrize("name", list(NETS))
def test_every_network_equals_the_staged_entry(name):
    fc, params, K_ = network(name)
    pos, quat = layout()
    check_against_staged(fc, params, K_, axis(17), axis(13), axis(11), pos, quat)


@pytest.mark.parametrize("name,shape", [("nerf_12to16_k1", s) for s in SHAPES] + [("m1_k2", s) for s in SHAPES if s != (128, 128, 65)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_shape_equals_the_staged_entry(name, shape):
    """sides that are no multiple of anything, one-point axes, one workgroup and -- (128, 128, 65): 1.06 M points -- the
    grid-stride loop beyond 4096 x 256 threads (that shape with the one-layer 12 -> 16 network and K = 1 only: the test stays
    quick)"""
    fc, params, K_ = network(name)
    pos, quat = layout()
    check_against_staged(fc, params, K_, *(axis(n) for n in shape), pos, quat)


def test_sixteen_slot_neighbour_list_equals_the_staged_entry():
    """K = 9 on a map of 12 fields (on 7 fields K is capped at 7): the run-time-K instance of the assignment"""
    fc, params, K_ = network("fourier_concat_k9", NF=12)
    pos, quat = layout(12)
    assert K_ == 9 and pos.shape[0] > K_
    check_against_staged(fc, params, K_, axis(17), axis(13), axis(11), pos, quat)


def test_perturbed_axes_equal_the_staged_entry():
    """non-uniform axes: the kernels read the coordinates, they do not derive them from origin + step"""
    fc, params, K_ = network("m1_k2")
    pos, quat = layout()
    g = torch.Generator().manual_seed(5)
    axes = [axis(n) + (0.2 * (torch.rand(n, generator=g) - 0.5)).to(DEV) for n in (17, 13, 11)]
    assert all(float((a[1:] - a[:-1]).std()) > 1e-2 for a in axes)
    check_against_staged(fc, params, K_, *axes, pos, quat)


def test_mask_radius_equals_the_staged_entry():
    fc, params, K_ = network("m1_k2")
    pos, quat = layout()
    xs, ys, zs = axis(17), axis(13), axis(11)
    wide = check_against_staged(fc, params, K_, xs, ys, zs, pos, quat, mask_radius=1.1)
    plain = ops.field_eval_knn(fc, params, torch.cartesian_prod(xs, ys, zs), pos, quat, K_, 10.0, 1.0)
    assert int((wide != 1.0).any(-1).sum()) > int((plain != 1.0).any(-1).sum())      # the wider mask takes more points in


def test_field_index_subset_equals_the_staged_entry():
    fc, params, K_ = network("m1_k2")
    pos, quat = layout()
    rows = torch.tensor([5, 0, 3, 6], device=DEV)                          # a shuffled proper subset of the parameter rows
    xs, ys, zs = axis(17), axis(13), axis(11)
    sub = check_against_staged(fc, params, K_, xs, ys, zs, pos[rows].contiguous(), quat[rows].contiguous(), field_index=rows,
                               share=(0.05, 0.95))
    full = ops.field_eval_knn(fc, params, torch.cartesian_prod(xs, ys, zs), pos, quat, K_, 10.0, 1.0)
    assert not torch.equal(sub, full)                                       # the subset is another map


def test_large_map_equals_the_staged_entry():
    """3 000 fields on the reference's cover grid (spacing 2 r / sqrt 3): the candidate lists come from the three device-wide
    kernels (> 2 048 fields) and the grid over the centres does not fit the LDS of the assignment (> 64 KB)"""
    NF, r = 3000, 1.0
    g = torch.Generator().manual_seed(1)
    n = 15
    ax = torch.arange(n) * (2 * r / 3 ** 0.5)
    pos = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)[torch.randperm(n ** 3, generator=g)[:NF]]
    pos = (pos + 1e-3 * torch.randn(NF, 3, generator=g)).to(DEV)          # no exact distance ties
    quat = torch.nn.functional.normalize(torch.randn(NF, 4, generator=g), dim=-1).to(DEV)
    fs = O.FieldSpec(**NERF16)
    params = cu(O.init_params(fs, NF, seed=2, sigma=3.0))
    fc = K.field_cfg(**NERF16, matmul_mode="auto")
    lat = torch.linspace(-1.5, 8.0, 24, device=DEV)                        # from outside the map to its middle
    check_against_staged(fc, params, 2, lat, lat + 0.013, lat - 0.007, pos, quat)


# ------------------------------------------------------------------------------------------------ extract_mesh, fused against staged
def cluster_renderer(geometry_mode, radius=0.5, seed=4):
    """two clusters of three random-weight fields, 9 m apart"""
    g = torch.Generator().manual_seed(seed)
    pos = torch.cat([torch.rand(3, 3, generator=g) * 0.6, torch.rand(3, 3, generator=g) * 0.6 + torch.tensor([9.0, 0.0, 0.0])])
    quat = torch.nn.functional.normalize(torch.randn(6, 4, generator=g), dim=-1)
    fs = O.FieldSpec(**M1)
    params = O.init_params(fs, 6, seed=seed, sigma=3.0)
    r = make_renderer(M1, dict(field_radius=radius, geometry_mode=geometry_mode, num_samples_coarse=8, num_samples_depth_guided=16),
                      6, params)
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    return r


def same_mesh(a, b):
    assert a is not None and b is not None
    for x, y, what in zip(a, b, ("vertices", "faces", "colours")):
        assert x.shape == y.shape and torch.equal(x, y), what
    assert len(a[0]) > 100 and len(a[1]) > 100


# a level the random-weight fields do cross (the density mode's own 30.0 is for trained densities); None: the mode's level
LEVEL = dict(occupancy=None, density=0.05, neus=None, nrgbd=None)


@pytest.mark.parametrize("mode", ["occupancy", "density", "neus", "nrgbd"])
def test_extract_mesh_fused_equals_staged_in_every_geometry_mode(mode):
    r = cluster_renderer(mode)
    st_f, st_s = {}, {}
    fused = r.extract_mesh(None, resolution=0.1, threshold=LEVEL[mode], block=16, fused=True, stats=st_f)
    staged = r.extract_mesh(None, resolution=0.1, threshold=LEVEL[mode], block=16, fused=False, stats=st_s)
    same_mesh(fused, staged)
    print(mode, "fused", st_f, "staged", st_s)
    assert 0 < st_f["blocks_skipped"] < st_f["blocks_total"] == st_s["blocks_total"]
    assert st_f["blocks_evaluated"] + st_f["blocks_skipped"] == st_f["blocks_total"]
    assert st_s["blocks_skipped"] == 0 and st_s["blocks_evaluated"] == st_s["blocks_total"]
    assert 0 < st_f["blocks_with_surface"] == st_s["blocks_with_surface"] <= st_f["blocks_evaluated"]
    # with `debug` nothing is skipped and every block is recorded, as before
    dbg_f, dbg_s, st_d = {}, {}, {}
    fused_d = r.extract_mesh(None, resolution=0.1, threshold=LEVEL[mode], block=16, fused=True, stats=st_d, debug=dbg_f)
    r.extract_mesh(None, resolution=0.1, threshold=LEVEL[mode], block=16, fused=False, debug=dbg_s)
    same_mesh(fused_d, staged)
    assert st_d["blocks_skipped"] == 0 and len(dbg_f["blocks"]) == len(dbg_s["blocks"]) == st_d["blocks_total"]
    for bf, bs in zip(dbg_f["blocks"], dbg_s["blocks"]):
        assert torch.equal(bf["volume"], bs["volume"])


def test_extract_mesh_fused_equals_staged_with_transform_and_with_field_ids():
    r = cluster_renderer("nrgbd")
    c, s = 0.8, 0.6
    T = torch.tensor([[c, -s, 0, 0.3], [s, c, 0, -1.2], [0, 0, 1, 0.5], [0, 0, 0, 1.0]])
    st = {}
    same_mesh(r.extract_mesh(None, resolution=0.1, transform=T, block=16, fused=True, stats=st),
              r.extract_mesh(None, resolution=0.1, transform=T, block=16, fused=False))
    assert 0 < st["blocks_skipped"] < st["blocks_total"]
    ids = torch.tensor([4, 0, 2, 5, 99])                                   # (ids beyond the map are dropped, rm.py:2208)
    st = {}
    sub = r.extract_mesh(None, resolution=0.1, field_ids=ids, block=16, fused=True, stats=st)
    same_mesh(sub, r.extract_mesh(None, resolution=0.1, field_ids=ids, block=16, fused=False))
    assert 0 < st["blocks_skipped"] < st["blocks_total"]
    assert len(sub[0]) != len(r.extract_mesh(None, resolution=0.1, block=16)[0])           # the subset is another mesh


def test_model_radius_larger_than_the_maps_fused_equals_staged():
    """The renderer keeps two radii: the map's (config `field_radius`: pads the box by 2 r, spaces the grid) and the model's
    (the inside test of the volume evaluation).  With a model radius of 0.8 m on a map radius of 0.5 m points up to 0.8 m from a
    centre are inside a field, and blocks that hold only such points must still be evaluated: reachability is decided with
    the radius the evaluation tests, and the fused mesh is the staged one."""
    from neural_graph_mapping_amd import models as M
    from neural_graph_mapping_amd import renderer as Rr
    r_map, r_model, res, block = 0.5, 0.8, 0.1, 8
    g = torch.Generator().manual_seed(4)
    pos = torch.cat([torch.rand(3, 3, generator=g) * 0.6, torch.rand(3, 3, generator=g) * 0.6 + torch.tensor([9.0, 0.0, 0.0])])
    quat = torch.nn.functional.normalize(torch.randn(6, 4, generator=g), dim=-1)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=dict(
        encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
        encoding_kwargs=dict(dim_in=3, dim_out=64, mu=0.0, sigma=4.0, raw_coords=True), num_layers=2, dim_out=4, neus_initial_sd=1.0),
        num_knn=2, distance_factor=10.0, outside_value=1.0, field_radius=r_model, scale_mode="unit_cube").to(DEV)
    cam = Rr.Camera(640, 480, 554.2562584220408, 554.2562584220408, 319.5, 239.5, pixel_center=0.0)
    r = Rr.NeuralGraphRenderer(model, cam, Rr.shipped_config(field_radius=r_map), device=DEV)
    r.add_fields(6)
    for k, v in O.init_params(O.FieldSpec(**M1), 6, seed=4, sigma=3.0).items():
        model.all_fields_params[k].copy_(v.to(DEV))
    model.refresh_lp()
    r.set_field_poses(pos.to(DEV), quat.to(DEV))
    assert r._field_radius == r_map and abs(float(r._fc.field_radius) - r_model) < 1e-6
    axes = Mh.grid_axes(pos.to(DEV), r_map, res)
    by_map = Mh.reachable_blocks(axes, block, pos.to(DEV), r_map).cpu()
    by_model = Mh.reachable_blocks(axes, block, pos.to(DEV), r_model).cpu()
    assert int(by_map.sum()) < int(by_model.sum()) < by_model.numel() and bool((by_model | ~by_map).all())
    st_f, st_s = {}, {}
    fused = r.extract_mesh(None, resolution=res, block=block, fused=True, stats=st_f)
    staged = r.extract_mesh(None, resolution=res, block=block, fused=False, stats=st_s)
    same_mesh(fused, staged)
    assert st_f["blocks_evaluated"] == int(by_model.sum()) and 0 < st_f["blocks_skipped"] == int((~by_model).sum())
    assert st_f["blocks_with_surface"] == st_s["blocks_with_surface"]
    # the case does what it is for: some block that only the shell between the two radii reaches carries surface
    shell_only = by_model & ~by_map
    hit = 0
    for i, j, k in shell_only.nonzero().tolist():
        bx, by, bz = (axes[d][b * block:b * block + block + 1] for d, b in enumerate((i, j, k)))
        vol = r.evaluate_grid(bx, by, bz, negate=True)
        hit += int(len(Mh.marching_cubes(vol, 0.0)[0]) > 0)
    print(f"two radii: {int(by_map.sum())} blocks by the map's radius, {int(by_model.sum())} by the model's, {hit} shell-only blocks with surface")
    assert hit > 0


def test_evaluate_grid_is_the_lattice_twin_of_evaluate_points():
    r = cluster_renderer("nrgbd")
    xs, ys, zs = (torch.linspace(-0.4, 1.0, n, device=DEV) for n in (9, 7, 12))
    ref = r.evaluate_points(torch.cartesian_prod(xs, ys, zs))
    assert bool((ref != 1.0).any())
    assert torch.equal(r.evaluate_grid(xs, ys, zs), ref[:, 3].reshape(9, 7, 12))
    assert torch.equal(r.evaluate_grid(xs, ys, zs, channel=1, negate=True), -ref[:, 1].reshape(9, 7, 12))


def test_block_skipping_is_conservative():
    """A field whose centre is radius * (1 - 1e-4) from the face of an otherwise empty block, opposite a lattice point of that
    face: the point is inside the field (by 5e-5 m), so the block's volume is not constant.  The block must be evaluated."""
    radius, res, block = 0.5, 0.1, 8
    r = cluster_renderer("nrgbd", radius=radius)
    gmd = r._global_map_dict
    pos = torch.zeros(6, 3)
    pos[:, 0] = torch.tensor([0.0, 0.05, 0.1, 3.5, 6.0, 6.1])             # A: three fields around the origin, far from the block
    axes = Mh.grid_axes(pos.to(DEV), radius, res)                          # (the axes start at A's box wherever B ends up)
    face = float(axes[0][5 * block].double())                              # the plane between x-blocks 4 and 5, about 3.0
    pos[3:, 0] = torch.tensor([face + radius * (1 - 1e-4), 6.0, 6.1])      # B just beyond the face; two fields further on
    r.set_field_poses(pos.to(DEV), gmd["orientations"][:6])
    axes = Mh.grid_axes(pos.to(DEV), radius, res)
    assert float(axes[0][5 * block].double()) == face
    iy, iz = (int((axes[d] - 0.0).abs().argmin()) for d in (1, 2))         # the lattice line through B's centre
    on_face = torch.stack([axes[0][5 * block], axes[1][iy], axes[2][iz]]).cpu().double()
    d = float((on_face - pos[3].double()).norm())
    assert radius * (1 - 3e-4) < d < radius, d                             # inside B, barely
    assert float((pos[[0, 1, 2, 4, 5]].double() - on_face).norm(dim=-1).min()) > 3 * radius     # and inside nothing else
    reach = Mh.reachable_blocks(axes, block, pos.to(DEV), radius).cpu()
    blk = (4, iy // block, iz // block)
    assert bool(reach[blk]) and not bool(reach.all())
    st = {}
    fused = r.extract_mesh(None, resolution=res, block=block, fused=True, stats=st)
    same_mesh(fused, r.extract_mesh(None, resolution=res, block=block, fused=False))
    assert st["blocks_evaluated"] == int(reach.sum()) and st["blocks_skipped"] == int((~reach).sum()) > 0
    # the block does hold a point the fields reach: its volume is not constant
    bx, by, bz = (axes[i][b * block:b * block + block + 1] for i, b in enumerate(blk))
    vol = r.evaluate_grid(bx, by, bz)
    assert int((vol != 1.0).sum()) >= 1


# ------------------------------------------------------------------------------------------------ memory safety
GUARD = 4096
PATTERN = 0xA5


def test_sentinels_around_volume_workspace_and_axes_and_a_side_stream():
    """The volume and a workspace of EXACTLY ngm_grid_eval_knn_workspace bytes inside larger pattern-filled buffers (the
    workspace at an address that is not 256-byte aligned: the library aligns inside it), the axes directly against the
    pattern; every guard byte intact after the call.  The same call on a side stream gives the default stream's volume."""
    fc, params, K_ = network("m1_k2")
    pos, quat = layout()
    n = (17, 13, 11)
    L = K.lib()
    ps = ops.params_struct(fc, params)
    wsb = L.ngm_grid_eval_knn_workspace(7, *n, K_)
    assert wsb > 0
    P = n[0] * n[1] * n[2]

    def banded(nbytes, shift=0):
        raw = torch.full((GUARD + shift + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        return raw, raw[GUARD + shift:GUARD + shift + nbytes]

    vol_raw, vol = banded(4 * P)
    ws_raw, ws = banded(wsb, shift=64)
    assert ws.data_ptr() % 256 != 0
    ax_raw, ax = banded(4 * sum(n))                                          # xs | ys | zs back to back between the guards
    axf = ax.view(torch.float32)
    axf.copy_(torch.cat([axis(k) for k in n]))
    xs, ys, zs = axf[:n[0]], axf[n[0]:n[0] + n[1]], axf[n[0] + n[1]:]
    ax_before = ax_raw.clone()

    def call(volume, stream):
        K.check(L.ngm_grid_eval_knn(C.byref(fc), C.byref(ps), 7, pos.data_ptr(), quat.data_ptr(), xs.data_ptr(), n[0], ys.data_ptr(),
                                    n[1], zs.data_ptr(), n[2], K_, 10.0, 1.0, 0.0, 3, 1, volume.data_ptr(), ws.data_ptr(), wsb, stream),
                "ngm_grid_eval_knn")

    call(vol, ops._stream())
    torch.cuda.synchronize()
    for raw, payload, what in ((vol_raw, 4 * P, "volume"), (ws_raw, wsb + 64, "workspace")):
        assert bool((raw[:GUARD] == PATTERN).all()), what + ": written before"
        assert bool((raw[GUARD + payload:] == PATTERN).all()), what + ": written after"
    assert bool((ws_raw[GUARD:GUARD + 64] == PATTERN).all()), "workspace: written before its first byte"
    assert torch.equal(ax_raw, ax_before), "the axes (or their guards) were written"
    got = vol.view(torch.float32).reshape(n).clone()
    want = -ops.field_eval_knn(fc, params, torch.cartesian_prod(xs, ys, zs), pos, quat, K_, 10.0, 1.0)[:, 3].reshape(n)
    assert torch.equal(got, want) and bool((got != -1.0).any())
    side = torch.cuda.Stream()
    vol2 = torch.full((P,), float("nan"), device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(vol2, side.cuda_stream)
    side.synchronize()
    assert torch.equal(vol2.reshape(n), got)
    assert bool((ws_raw[:GUARD] == PATTERN).all()) and bool((ws_raw[GUARD + 64 + wsb:] == PATTERN).all())
