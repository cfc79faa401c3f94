"""CPU-side checks of the growing map (reserved field rows; include/ngm_hip.h ngm_fields_append, ngm_target_sample_mv_grow,
ngm_target_observed_fields_grow): symbols and struct layouts, the in-place bookkeeping of reserve_fields / add_fields on CPU
tensors, the checkpoint of a reserved map, the host restatement of the grow sampler's counts against its host-known row
capacity, the choice of the GPU test's map seed, and the argument refusals of the new ops.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngm_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _growing_map_host as G  # noqa: E402
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402

NEW = ("ngm_fields_append", "ngm_target_sample_mv_grow_workspace", "ngm_target_sample_mv_grow",
       "ngm_target_observed_fields_grow_workspace", "ngm_target_observed_fields_grow")


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


# ------------------------------------------------------------------------------------------------ ABI
def test_symbols_declared_and_exported_abi_unchanged(capi):
    head = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    L = capi.lib()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", src), n
        assert n in capi.EXPORTED and hasattr(L, n), n
    assert int(re.search(r"#define\s+NGM_ABI_VERSION\s+(\d+)", head).group(1)) == 11 == L.ngm_abi_version()
    assert int(re.search(r"#define\s+NGM_APPEND_MAX_TENSORS\s+(\d+)", src).group(1)) == capi.NGM_APPEND_MAX_TENSORS
    W = L.ngm_target_sample_mv_grow_workspace
    assert W(16, 70, 70, 12) == L.ngm_target_sample_mv_live_workspace(16, 70, 70, 12) > 0
    assert W(16, 70, 0, 0) == -1 and W(16, 0, 70, 12) == -1
    assert L.ngm_target_observed_fields_grow_workspace(24, 32) == L.ngm_target_observed_fields_workspace(24, 32) > 0
    # argument validation happens before any launch (no device here)
    assert L.ngm_fields_append(None, None) == capi.NGM_E_INVALID
    a = capi.FieldsAppendArgs(None, 0, 65, 6, 70, 8, 8, 8, 8, None, 8)              # rows [65, 71) of 70
    assert L.ngm_fields_append(C.byref(a), None) == capi.NGM_E_INVALID and b"max_fields" in L.ngm_last_error()
    a.num_new, a.num_fields_dev = 5, None
    assert L.ngm_fields_append(C.byref(a), None) == capi.NGM_E_INVALID and b"NULL" in L.ngm_last_error()


def test_struct_layouts_match_header(capi, tmp_path):
    at = [f[0] for f in capi.AppendTensor._fields_]
    fa = [f[0] for f in capi.FieldsAppendArgs._fields_]
    fmt = " ".join(["%zu"] * (2 + len(at) + len(fa)))
    args = ",".join(["sizeof(ngm_append_tensor)"] + [f"offsetof(ngm_append_tensor,{f})" for f in at] +
                    ["sizeof(ngm_fields_append_args)"] + [f"offsetof(ngm_fields_append_args,{f})" for f in fa])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngm_hip.h"\n'
                   f'int main(){{printf("{fmt}\\n",{args});return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    AT, FA = capi.AppendTensor, capi.FieldsAppendArgs
    assert sizes == ([C.sizeof(AT)] + [getattr(AT, f).offset for f in at] + [C.sizeof(FA)] + [getattr(FA, f).offset for f in fa])


def test_ops_registered_with_fake_shapes(capi):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import ops
    i32 = lambda: torch.zeros(1, dtype=torch.int32, device="cuda")
    with FakeTensorMode(allow_non_fake_inputs=True):
        dev = "cuda"
        out = torch.ops.ngm355.target_sample_mv_grow(
            torch.zeros(70, dtype=torch.int64, device=dev), i32(), torch.zeros(16, 4, 4, device=dev), i32(), i32(),
            torch.zeros(20, 24, 32, 4, device=dev), torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(70, 3, device=dev),
            None, [1.0, 1.0, 0.0, 0.0], 1.0, 70, 12, 32, 0, 0, 3, 1)
        shapes = {k: tuple(v.shape) for k, v in zip(ops.TARGET_SAMPLE_MV_LIVE_OUT, out)}
        assert shapes["ijs"] == (12, 32, 2) and shapes["subset_observed"] == (6,) and shapes["subset_random"] == (12,)
        px, used = torch.ops.ngm355.target_observed_fields_grow(
            torch.zeros(24, 32, 4, device=dev), torch.zeros(4, 4, device=dev), torch.zeros(70, 3, device=dev), i32(), None, None,
            torch.zeros(70, dtype=torch.int64, device=dev), i32(), [1.0, 1.0, 0.0, 0.0], 0.35, 70, 64, 0, 0)
        assert tuple(px.shape) == (64,) and px.dtype == torch.int64 and used.dtype == torch.int32
    assert hasattr(torch.ops.ngm355, "fields_append")


# ------------------------------------------------------------------------------------------------ bookkeeping on CPU tensors
def cpu_renderer(weight_dtype=None):
    fkw = dict(encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
               encoding_kwargs=dict(dim_in=3, dim_out=32, mu=0.0, sigma=4.0, raw_coords=True), num_layers=1, dim_out=4,
               neus_initial_sd=1.0)
    torch.manual_seed(3)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=fkw, num_knn=2,
                             distance_factor=10.0, outside_value=1.0, field_radius=1.0, scale_mode="unit_cube",
                             weight_dtype=weight_dtype)
    cam = Rr.Camera(32, 24, 25.0, 25.0, 15.5, 11.5)
    return Rr.NeuralGraphRenderer(model, cam, Rr.shipped_config(), device="cpu")


def storages(r):
    """data pointer of every storage of the reservation, through the public views"""
    p = {"param " + k: v.untyped_storage().data_ptr() for k, v in r._model.all_fields_params.items()}
    for k, st in r._optim_state.items():
        p["exp_avg " + k], p["exp_avg_sq " + k] = st["exp_avg"].untyped_storage().data_ptr(), st["exp_avg_sq"].untyped_storage().data_ptr()
    if r._model.lp_fields_params is not None:
        p.update({"lp " + k: v.untyped_storage().data_ptr() for k, v in r._model.lp_fields_params.items()})
    md = r._global_map_dict
    p.update({k: md[k].untyped_storage().data_ptr() for k in ("positions", "orientations", "training_iterations")})
    p["num_fields_dev"] = r._reserved["num_fields_dev"].data_ptr()
    return p


def snapshot(r, rows):
    s = {"param " + k: v[:rows].clone() for k, v in r._model.all_fields_params.items()}
    for k, st in r._optim_state.items():
        s["exp_avg " + k], s["exp_avg_sq " + k] = st["exp_avg"][:rows].clone(), st["exp_avg_sq"][:rows].clone()
    if r._model.lp_fields_params is not None:
        s.update({"lp " + k: v[:rows].clone() for k, v in r._model.lp_fields_params.items()})
    md = r._global_map_dict
    s.update({k: md[k][:rows].clone() for k in ("positions", "orientations", "training_iterations")})
    return s


@pytest.mark.parametrize("weight_dtype", [None, "bfloat16"])
def test_reserved_bookkeeping_on_cpu_tensors(weight_dtype):
    r = cpu_renderer(weight_dtype)
    assert r._reserved is None
    r.reserve_fields(G.CAPACITY)
    base = storages(r)
    proto = {k: v.detach().clone() for k, v in r._model._prototype_field.state_dict().items()}
    g = torch.Generator().manual_seed(1)
    num = 0
    for step, n_new in enumerate((40, 20, 10)):             # 40, 60 (the GPU test's start), then + 10 to the capacity
        old = snapshot(r, num)
        pos, quat = torch.randn(n_new, 3, generator=g), torch.randn(n_new, 4, generator=g)
        r.add_fields(n_new, positions=pos, orientations=quat)
        num += n_new
        assert storages(r) == base, "the reservation's storage moved"
        md = r._global_map_dict
        assert md["num"] == num == int(r._reserved["num_fields_dev"]) and r._reserved["num_fields_dev"].dtype == torch.int32
        assert md["positions"].shape == (num, 3) and md["orientations"].shape == (num, 4)
        for k, v in r._model.all_fields_params.items():
            assert v.shape[0] == num and v.is_contiguous(), k
            assert torch.equal(v[num - n_new:], proto[k].expand(n_new, *proto[k].shape)), k                  # new rows = the prototype
            for m in r._optim_state[k].values():
                assert m.shape == v.shape and not m[num - n_new:].any(), k                                   # zero moments
        if weight_dtype:
            for k, v in r._model.lp_fields_params.items():
                want = r._model.all_fields_params[k]
                want = want if k in ("_neus_sd",) else want.to(torch.bfloat16)
                assert v.shape[0] == num and v.dtype == want.dtype and torch.equal(v, want), k
        assert torch.equal(md["positions"][num - n_new:], pos) and torch.equal(md["orientations"][num - n_new:], quat)
        assert not md["training_iterations"][num - n_new:num].any()
        now = snapshot(r, num - n_new)
        for k in old:                                       # the old rows and their moments: bit for bit untouched
            assert torch.equal(now[k], old[k]), (step, k)
        # "train" the fields held so far: the next append must leave every bit of this alone
        with torch.no_grad():
            for k, v in r._model.all_fields_params.items():
                v.add_(torch.randn(v.shape, generator=g) * 0.01)
                for m in r._optim_state[k].values():
                    m.add_(torch.rand(m.shape, generator=g))
            r._model.refresh_lp()
            r._training_iterations()[:num] += 3
        assert storages(r) == base
    # the 71st field: refused, nothing changes
    before, ptrs = snapshot(r, G.CAPACITY), storages(r)
    with pytest.raises(ValueError, match="reserved"):
        r.add_fields(1, positions=torch.zeros(1, 3), orientations=torch.zeros(1, 4))
    with pytest.raises(ValueError, match="reserved"):
        r._model.add_fields(1)
    after = snapshot(r, G.CAPACITY)
    assert storages(r) == ptrs and r._global_map_dict["num"] == G.CAPACITY == int(r._reserved["num_fields_dev"])
    assert all(torch.equal(after[k], before[k]) for k in before)
    # loop closure: all poses move, in place; growth does not go through set_field_poses
    new_pos = torch.randn(G.CAPACITY, 3, generator=g)
    r.set_field_poses(new_pos, after["orientations"])
    assert storages(r) == ptrs and torch.equal(r._global_map_dict["positions"], new_pos)
    with pytest.raises(ValueError, match="add_fields"):
        r.set_field_poses(torch.zeros(71, 3), torch.zeros(71, 4))
    assert torch.equal(r.get_field_ids(6), torch.arange(60)) and r.get_field_ids().shape == (G.CAPACITY,)      # 9 / 6 / 3 counted above


def test_unreserved_paths_are_todays():
    r = cpu_renderer()
    r.add_fields(5)
    p0 = {k: v.data_ptr() for k, v in r._model.all_fields_params.items()}
    r.add_fields(3)                                         # torch.cat: new tensors, as before
    assert all(v.shape[0] == 8 and v.data_ptr() != p0[k] for k, v in r._model.all_fields_params.items())
    with pytest.raises(ValueError, match="reserve_fields"):
        r.add_fields(1, positions=torch.zeros(1, 3), orientations=torch.zeros(1, 4))
    pos = torch.zeros(8, 3)
    r.set_field_poses(pos, torch.zeros(8, 4))
    assert r._global_map_dict["positions"] is pos           # the caller's tensor, not a copy
    # reserving a map that already holds fields keeps them, their moments and their poses
    r._optim_state["_linears.0.weight"]["exp_avg"].fill_(2.0)
    keep = {k: v.clone() for k, v in r._model.all_fields_params.items()}
    r.reserve_fields(12)
    assert all(torch.equal(r._model.all_fields_params[k], keep[k]) for k in keep)
    assert bool((r._optim_state["_linears.0.weight"]["exp_avg"] == 2.0).all()) and r._global_map_dict["num"] == 8
    with pytest.raises(ValueError, match="already holds"):
        r.reserve_fields(7)


def test_checkpoint_of_a_reserved_map_holds_num_rows(tmp_path):
    r = cpu_renderer("bfloat16")
    r.reserve_fields(G.CAPACITY)
    r.add_fields(9, positions=torch.randn(9, 3), orientations=torch.randn(9, 4))
    r._training_iterations()[:9] += 2
    path = str(tmp_path / "ck.pt")
    r.save_model(path)
    ck = torch.load(path)
    assert set(ck) == {"map_dict", "all_fields_params", "state_dict"} and ck["map_dict"]["num"] == 9
    for k, v in ck["all_fields_params"].items():
        assert v.shape[0] == 9 and v.untyped_storage().nbytes() == v.numel() * v.element_size(), k
        assert torch.equal(v, r._model.all_fields_params[k])
    for k in ("positions", "orientations", "training_iterations"):
        v = ck["map_dict"][k]
        assert v.shape[0] == 9 and v.untyped_storage().nbytes() == v.numel() * v.element_size(), k
    assert os.path.getsize(path) < 3 * sum(v.numel() * 4 for v in ck["all_fields_params"].values()) + 65536
    r2 = cpu_renderer("bfloat16")
    r2.reserve_fields(G.CAPACITY)
    r2.load_model(path)                                     # reallocates: leaves reserved mode
    assert r2._reserved is None and r2._model._reserved is None and r2._global_map_dict["num"] == 9
    for k, v in r2._model.all_fields_params.items():
        assert v.shape[0] == 9 and v.untyped_storage().nbytes() == v.numel() * v.element_size(), k
    assert r2._model.lp_fields_params["_linears.0.weight"].shape[0] == 9
    r2.add_fields(1)                                        # today's path again
    assert r2._model.all_fields_params["_linears.0.weight"].shape[0] == 10


# ------------------------------------------------------------------------------------------------ the sampler's counts
def test_grow_counts_fit_the_host_known_capacity(capi):
    MAXF, T = G.CAPACITY, G.T
    for W in (1, 2, 3):
        for rank in range(W):
            n_obs_max, n_rand_max, cap = capi.target_sample_mv_grow_plan(MAXF, MAXF, T, G.R, W, rank)
            assert cap == G.grow_capacity(MAXF, T, W, rank) == min(T, G.owned(MAXF, W, rank))
            # at nf == max_fields: the parent's formula for a map of that many fields, whatever the observed count
            assert (n_obs_max, n_rand_max, cap) == capi.target_sample_mv_live_plan(MAXF, MAXF, T, G.R, W, rank)
            for nf in (0, 1, 5, 12, 13, 64, 65, 70):
                for nc_dev in (0, 1, 5, 6, 7, nf, nf + 3, 10 ** 6, -2):
                    f, nc, n_obs, n_rand = G.grow_counts(nc_dev, nf, MAXF, MAXF, T)
                    assert (f, nc, n_obs, n_rand) == capi.grow_counts(nc_dev, nf, MAXF, MAXF, T)
                    assert 0 <= nc <= f == nf and n_obs <= n_obs_max and n_rand <= n_rand_max
                    assert n_obs + n_rand == min(T, nf)                      # the device draws exactly that many fields
                    # of which this rank owns at most its fields among the nf in force: within the host-known rows
                    assert min(n_obs + n_rand, G.owned(nf, W, rank)) <= cap
                    if 0 <= nc_dev <= nf:                                    # and what an unreserved map of nf fields plans
                        assert (n_obs, n_rand) == capi.target_sample_mv_plan(nc_dev, nf, T, G.R, W, rank)[:2]
                        assert capi.target_sample_mv_plan(nc_dev, nf, T, G.R, W, rank)[2] <= cap
    assert capi.grow_counts(5, 99, 70, 70, 12)[0] == 70 and capi.grow_counts(5, -1, 70, 70, 12) == (0, 0, 0, 0)


def test_map_seed_trains_new_fields_only_after_the_growth():
    """the choice of tests/test_gpu_growing_map.py's map (G.MAP_SEED): the host predicts at least one field >= START among
    the trained ones after the growth -- in G.TRAINED_NEW_ITERATIONS of those 10 iterations -- and, before it, only ids
    below START (there are no others)"""
    pred = G.predict_trained(G.MAP_SEED)
    assert len(pred) == 4 * G.PER_FRAME
    before, after = pred[:G.GROW_AFTER * G.PER_FRAME], pred[G.GROW_AFTER * G.PER_FRAME:]
    assert all(nf == G.START and (k < G.START).all() for nf, k in before) and sum(len(k) for _, k in before) > 0
    hits = sum(1 for nf, k in after if (k >= G.START).any())
    assert all(nf == G.CAPACITY for nf, _ in after) and hits == G.TRAINED_NEW_ITERATIONS >= 1


# ------------------------------------------------------------------------------------------------ refusals
def test_validators_raise_before_launch(capi):
    from neural_graph_mapping_amd import ops
    i32 = lambda: torch.zeros(1, dtype=torch.int32)
    good = dict(current_field_ids=torch.zeros(70, dtype=torch.int64), current_count=i32(), c2ws=torch.zeros(6, 4, 4), num_frames=i32(),
                num_fields_dev=i32(), rgbd_store=torch.zeros(8, 24, 32, 4), frame_to_store=torch.zeros(6, dtype=torch.int64),
                field_positions=torch.zeros(70, 3))

    def call(**kw):
        a = dict(good)
        rest = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, radius=1.0, max_fields=70, num_train_fields=12, num_rays_per_field=16, iteration=0)
        for k in list(kw):
            (a if k in a else rest)[k] = kw[k]
        return ops.target_sample_mv_grow(**a, **rest)
    with pytest.raises(TypeError, match="num_fields_dev"):
        call(num_fields_dev=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="num_fields_dev"):
        call(num_fields_dev=60)
    with pytest.raises(TypeError, match="current_count"):
        call(current_count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="field_positions"):                   # capacity mismatch: 60 pose rows for 70 reserved fields
        call(field_positions=torch.zeros(60, 3))
    with pytest.raises(ValueError, match="max_current"):                       # more id slots than reserved fields
        call(current_field_ids=torch.zeros(71, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()

    ogood = dict(rgbd=torch.zeros(24, 32, 4), c2w=torch.eye(4), field_positions=torch.zeros(70, 3))

    def obs(**kw):
        a = dict(ogood)
        rest = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, radius=0.35, num_fields=70, num_points=64, frame=0, num_fields_dev=i32())
        for k in list(kw):
            (a if k in a else rest)[k] = kw[k]
        return ops.target_observed_fields(**a, **rest)
    with pytest.raises(TypeError, match="num_fields_dev"):
        obs(num_fields_dev=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="field_positions"):
        obs(field_positions=torch.zeros(69, 3))
    with pytest.raises(ValueError, match="ids_out"):                           # capacity mismatch: 60 slots for 70 reserved fields
        obs(ids_out=torch.zeros(60, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        obs()

    def tensors(rows=70, lp=None, dt=torch.float32):
        return [dict(param=torch.zeros(rows, 4, 8, dtype=dt), exp_avg=torch.zeros(rows, 4, 8), exp_avg_sq=torch.zeros(rows, 4, 8),
                     prototype=torch.zeros(4, 8), lp=lp)]

    def app(ts=None, first=60, n=10, **kw):
        a = dict(new_positions=torch.zeros(n, 3), new_orientations=torch.zeros(n, 4), positions=torch.zeros(70, 3),
                 orientations=torch.zeros(70, 4), training_iterations=torch.zeros(70, dtype=torch.int64), num_fields_dev=i32())
        a.update(kw)
        return ops.fields_append(tensors() if ts is None else ts, first=first, **a)
    with pytest.raises(TypeError, match="num_fields_dev"):
        app(num_fields_dev=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="capacity"):                          # rows [61, 71) of 70
        app(first=61)
    with pytest.raises(ValueError, match="capacity mismatch"):                 # a tensor reserved for 60 rows under 70 pose rows
        app(tensors(rows=60))
    with pytest.raises(ValueError, match="capacity mismatch"):
        app(tensors(lp=torch.zeros(60, 4, 8, dtype=torch.bfloat16)))
    with pytest.raises(TypeError, match="bfloat16 or float16"):
        app(tensors(lp=torch.zeros(70, 4, 8, dtype=torch.float64)))
    with pytest.raises(TypeError, match="float32"):
        app(tensors(dt=torch.float64))
    with pytest.raises(ValueError, match="orientations"):
        app(orientations=torch.zeros(69, 4))
    with pytest.raises(TypeError, match="training_iterations"):
        app(training_iterations=torch.zeros(70, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        app()
