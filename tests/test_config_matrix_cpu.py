"""CPU companion of tests/test_gpu_config_matrix.py: the table of tests/_config_matrix.py builds and evaluates in the oracle,
its fused-step problems can be made kink-free inside the usual cap, it is internally consistent, and the library's validator
draws the line where the table says it does (argument validation needs no GPU), and the library's two host-side plans
(ngm_debug_plan_fwd, ngm_debug_plan_bwd) reproduce the table's forward and backward columns.  For the storage axis
(tests/test_gpu_storage_matrix.py): the rounded twin problems are inside the conditions under which a bitwise comparison of the
two storages says something, before any kernel runs, and `storage16` follows from the fp32 columns."""
import ctypes as C

import pytest
import torch

import _config_matrix as CM
from gpu_common import matrix_knn_case, matrix_points_case, matrix_step_case, matrix_storage_twin, matrix_twin_oracle
from neural_graph_mapping_amd import _capi as K
from oracle import ngm_oracle as O


@pytest.mark.parametrize("name", CM.NAMES)
def test_entry_builds_and_evaluates_in_the_oracle(name):
    """O.FieldSpec, K.field_cfg and O.init_params agree on the shapes; forward and backward are finite and every trainable
    tensor receives a gradient (4 layers, 3 layers at 32 units and every other refused entry included: the oracle has no
    kernel list)."""
    e = CM.BY_NAME[name]
    fs, fc = O.FieldSpec(**e["fkw"]), K.field_cfg(**e["fkw"])
    assert (fs.dim_enc, fs.dim_hidden, fs.num_layers) == (fc.dim_enc, fc.dim_hidden, fc.num_layers)
    assert {k: tuple(v) for k, v in fs.param_shapes().items()} == {k: tuple(v) for k, v in K.param_shapes(fc).items()}
    for P in (1, 257):
        c = matrix_points_case(e, P)
        assert c["out"].shape == (3, P, 4) and torch.isfinite(c["out"]).all()
        for k in K.param_names(fc):
            if k in K.NO_GRAD_PARAMS:
                continue
            g = c["grads"][k]
            assert g.shape == c["params"][k].shape and torch.isfinite(g).all(), k
            assert P == 1 or float(g.abs().max()) > 0, k
    k = matrix_knn_case(e)
    assert k["ref"].shape == (500, 4) and torch.isfinite(k["ref"]).all()
    assert 0 < int((k["ref"] != 1.0).any(-1).sum()) < 500          # points inside and outside the fields


@pytest.mark.parametrize("shape", CM.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", [e["name"] for e in CM.ENTRIES if any(CM.runs(o) for o in e["step"].values())])
def test_fused_step_problem_is_kink_free_inside_the_cap(name, shape):
    """kink_free_draws converges for every entry whose fused step is expected to run and neutralises at most 15 % of the rays
    (its own `max_neutralised` default, asserted inside); the oracle's losses and gradients on the result are finite."""
    c = matrix_step_case(CM.BY_NAME[name], shape)
    assert len(c["kink"]) == 1 and c["kink"][0]["neutralised_frac"] <= 0.15
    assert torch.isfinite(c["pred"]["rgbds"]).all()
    for k, g in c["grads"].items():
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k


def test_table_is_internally_consistent():
    assert len(set(CM.NAMES)) == len(CM.ENTRIES) >= 40
    fwd_shapes, variants = set(), set()
    for e in CM.ENTRIES:
        for s in CM.SURFACES:
            assert set(e[s]) >= {"f32", "auto"}, (e["name"], s)                     # every (entry, surface) pair has an expectation
            for mode, o in e[s].items():
                assert mode in ("f32", "auto", "bf16x3")
                if o == CM.REFUSE:
                    continue
                kind = {"points": "fwd", "render": "fwd", "knn": "fwd", "autograd": "bwd", "step": "step"}[s]
                assert o[0] == kind and e["shape"] in CM.FORWARD_SHAPES, (e["name"], s, mode)   # every "runs" names a kernel
                fwd_shapes.add(e["shape"])
                if kind == "fwd":
                    assert o[1] in ("f32", "bf16x3")
                elif kind == "bwd":
                    assert o[1] in CM.BWD_VARIANTS and o[2] in CM.BWD_VARIANTS
                    variants.update(o[1:])
                else:
                    assert o[1] in ("f32", "bf16x3") and o[2] in CM.BWD_VARIANTS and o[3] in (0, 1)
                    variants.add(o[2])
        if e["shape"] is None:
            assert all(o == CM.REFUSE for s in CM.SURFACES for o in e[s].values()), e["name"]
    assert fwd_shapes == set(CM.FORWARD_SHAPES)          # no instantiation of the forward dropped from the table
    assert variants == set(CM.BWD_VARIANTS)              # nor a backward kernel


def test_forward_shape_follows_from_the_widths():
    for e in CM.ENTRIES:
        fc = K.field_cfg(**e["fkw"])
        mi, mh = (fc.dim_enc + 31) // 32, (fc.dim_hidden + 31) // 32
        assert mi == mh, e["name"]                        # what check_field_cfg demands of every entry
        if e["shape"] is not None:
            assert e["shape"] == f"<{mi},{mh},{fc.num_layers}>", e["name"]


F16_MIN_NORMAL = 2.0 ** -14


@pytest.mark.parametrize("wd", CM.STORAGE)
@pytest.mark.parametrize("name", CM.NAMES)
def test_rounded_twin_is_a_problem_worth_comparing(name, wd):
    """The point-evaluation parameters of every entry (the refused ones are handed to the library too), rounded to either storage type: finite (max |w| = 8.565, far
    from fp16's 65504), at least half of each tensor's elements changed by the rounding (the twin is another problem than the
    case), under 1 % of a tensor's elements lost to zero, fp16 subnormals present in every entry (so their widening is
    exercised), the 16-bit set exactly the fp32 twin, and the oracle's forward at the rounded parameters finite.  The step and
    kNN parameters of the entry stay finite too."""
    e = CM.BY_NAME[name]
    dt = getattr(torch, wd)
    c = matrix_points_case(e, 257)
    tw = matrix_storage_twin(c, dt)
    assert matrix_storage_twin(c, dt) is tw                              # cached
    subnormal = 0
    for k, v in c["params"].items():
        r, lp = tw["f32"][k], tw["lp"][k]
        assert r.dtype == torch.float32 and torch.isfinite(r).all(), k
        if k in K.NO_GRAD_PARAMS:
            assert lp.dtype == torch.float32 and torch.equal(r, v) and torch.equal(lp, v), k
            continue
        assert lp.dtype == dt and torch.equal(lp.float(), r) and torch.equal(r.to(dt), lp), k      # representable: the round trip is exact
        assert float(v.abs().max()) < 2.0 ** 15, k                          # half of fp16's range (the largest weight is 8.565)
        assert float((r != v).float().mean()) >= 0.5, (k, "rounding changes less than half of the elements")
        assert float(((r == 0) & (v != 0)).float().mean()) < 0.01, (k, "rounding loses 1 % of the elements to zero")
        h = v.to(torch.float16).float().abs()
        subnormal += int(((h > 0) & (h < F16_MIN_NORMAL)).sum())
    assert subnormal >= 1, "no fp16 subnormal in the entry: their widening would not be exercised"
    out = matrix_twin_oracle(e, dt)
    assert out.shape == (3, 257, 4) and torch.isfinite(out).all() and not torch.equal(out, c["out"])
    for other in (matrix_knn_case(e),) + tuple(matrix_step_case(e, s) for s in CM.STEP_SHAPES):
        for k, v in matrix_storage_twin(other, dt)["f32"].items():
            assert torch.isfinite(v).all() and float(v.abs().max()) < 65504, k


def test_storage_axis_follows_from_the_fp32_columns():
    """storage16 is defined for every (entry, surface, mode): the entry's own outcome, REFUSE_STORAGE for the triplane planes and
    for nothing else; what refuses in fp32 refuses (a 16-bit copy opens no kernel), what runs names the same kernels."""
    assert CM.STORAGE == ("bfloat16", "float16")
    tri = 0
    for e in CM.ENTRIES:
        for s in CM.SURFACES:
            for mode in CM.modes(e, s):
                o = CM.storage16(e, s, mode)
                if e["fkw"]["encoding"] == "triplane":
                    assert o == CM.REFUSE_STORAGE and not CM.runs(o)
                    tri += 1
                else:
                    assert o == e[s][mode] and o != CM.REFUSE_STORAGE and CM.runs(o) == (e[s][mode] != CM.REFUSE)
    assert tri > 0
    with pytest.raises(KeyError):
        CM.storage16(CM.ENTRIES[0], "points", "fp8")


@pytest.fixture(scope="module")
def lib():
    try:
        return K.lib()
    except Exception as ex:                               # the package's own tests require the library: fail, do not skip
        pytest.fail(f"libngm_hip.so is not built: {ex}")


@pytest.mark.parametrize("name", CM.NAMES)
def test_validator_refuses_exactly_what_no_kernel_takes(lib, name):
    """check_field_cfg through ngm_render_workspace (no launch, no GPU): entries without any kernel are refused with
    NGM_E_UNSUPPORTED and a message that says which depths exist; every other entry gets a workspace size."""
    e = CM.BY_NAME[name]
    fc, rc = K.field_cfg(**e["fkw"]), K.render_cfg(num_samples_coarse=5, num_samples_guided=2)
    ws = lib.ngm_render_workspace(C.byref(fc), C.byref(rc), 3, 37, 1)
    if e["shape"] is None:
        assert ws == K.NGM_E_UNSUPPORTED
        msg = lib.ngm_last_error().decode()
        assert "num_layers" in msg and "kernel" in msg
    else:
        assert ws > 0


def _plan(lib, fc, rc, F, n, stash_offered=0):
    """ngm_debug_plan_bwd: (status, variant, comp_fused, stash kind, stash layers, forward arithmetic); guided rays, seeds written
    for the backward's targets -- what the fused step of the matrix does"""
    out = (C.c_int32 * 5)()
    status = lib.ngm_debug_plan_bwd(C.byref(fc), None if rc is None else C.byref(rc), F, n, 1, stash_offered, 1, out)
    return (status,) + tuple(out)


ARITHMETIC = {K.MATMUL["f32"]: "f32", K.MATMUL["bf16x3"]: "bf16x3"}
SURFACE = {"render": 0, "points": 1, "knn": 2}          # ngm_debug_plan_fwd (= the index of ngm_debug_last_matmul)


def _plan_fwd(lib, fc, rc, surface, F, n, guided=1):
    """ngm_debug_plan_fwd: (status, {shape, arithmetic, one-tile, waves, LDS bytes, neus instance})"""
    out = (C.c_int32 * 12)()
    status = lib.ngm_debug_plan_fwd(C.byref(fc), None if rc is None else C.byref(rc), SURFACE[surface], F, n, guided, out)
    return status, dict(shape=f"<{out[0]},{out[1]},{out[2]}>", mm=ARITHMETIC.get(out[3]), one_tile=out[4], waves=out[5], lds=out[6],
                        neus=out[7])


def test_plan_query_reproduces_the_step_and_autograd_columns(lib):
    """The backward plan (plan_mlp_bwd behind ngm_debug_plan_bwd: no launch, no GPU) against every (entry, mode) cell of the
    `step` and `autograd` columns: backward variant and fusion flag at both STEP_SHAPES, the forward arithmetic from the forward
    plan (ngm_debug_plan_fwd); the point evaluation's variant at P = 257 with a stash offered and without; three-layer entries
    refused with NGM_E_UNSUPPORTED; an explicit bf16x3 outside its shape refused by the forward plan, by name."""
    for e in CM.ENTRIES:
        if e["shape"] is None:
            continue
        for mode, o in e["step"].items():
            fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
            for F, R, n_c, n_g in CM.STEP_SHAPES:
                rc = K.render_cfg(geometry_mode=e["geometry"], num_samples_coarse=n_c, num_samples_guided=n_g)
                status, variant, fused, kind, layers, mm = _plan(lib, fc, rc, F, R)
                if o == CM.REFUSE and fc.num_layers <= 2:
                    fstatus, _ = _plan_fwd(lib, fc, rc, "render", F, R)
                    assert fstatus == K.NGM_E_UNSUPPORTED and "bf16x3" in lib.ngm_last_error().decode(), (e["name"], mode)
                elif o == CM.REFUSE:
                    assert status == K.NGM_E_UNSUPPORTED and "forward only" in lib.ngm_last_error().decode(), (e["name"], mode)
                else:
                    fstatus, f = _plan_fwd(lib, fc, rc, "render", F, R)
                    assert status == fstatus == K.NGM_OK and (f["mm"], variant, fused) == o[1:], (e["name"], mode, (F, R))
                    assert ARITHMETIC[mm] == f["mm"] and f["shape"] == e["shape"]
                    assert (variant not in (2, 3, 5) or kind == (2 if variant == 5 else 1)) and (layers > 0) == (kind != 0)
        for mode, o in e["autograd"].items():
            fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
            got = [_plan(lib, fc, None, 3, 257, stash_offered=s) for s in (1, 0)]
            if o == CM.REFUSE:
                assert fc.num_layers == 3 and [g[0] for g in got] == [K.NGM_E_UNSUPPORTED] * 2, (e["name"], mode)
            else:
                assert [g[:2] for g in got] == [(K.NGM_OK, o[1]), (K.NGM_OK, o[2])], (e["name"], mode)
                assert [g[3] for g in got] == [int(o[1] == 3), 0] and all(g[2] == 0 for g in got)    # only k_field_bwd_b3 reads a stash


def test_forward_plan_reproduces_the_forward_columns(lib):
    """The forward plan (plan_fwd behind ngm_debug_plan_fwd: no launch, no GPU) against every (entry, mode) cell of the `points`,
    `render` and `knn` columns: compiled shape and arithmetic -- 257 points per field, the 7-field kNN case, the fused forward at
    both STEP_SHAPES.  A refused cell is NGM_E_UNSUPPORTED: the validator's for the entries without a shape, the plan's -- naming
    the mode -- for an explicit bf16x3 outside its shape."""
    for e in CM.ENTRIES:
        for surface in ("points", "render", "knn"):
            for mode, o in e[surface].items():
                fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
                if surface == "render":
                    calls = [(K.render_cfg(geometry_mode=e["geometry"], num_samples_coarse=n_c, num_samples_guided=n_g), F, R)
                             for F, R, n_c, n_g in CM.STEP_SHAPES]
                else:
                    calls = [(None, 3, 257)] if surface == "points" else [(None, 7, 500)]
                for rc, F, n in calls:
                    status, f = _plan_fwd(lib, fc, rc, surface, F, n)
                    msg = lib.ngm_last_error().decode()
                    if o == CM.REFUSE:
                        assert status == K.NGM_E_UNSUPPORTED, (e["name"], surface, mode)
                        assert ("num_layers" in msg) if e["shape"] is None else (mode == "bf16x3" and "bf16x3" in msg and e["shape"] in msg)
                    else:
                        assert status == K.NGM_OK and (f["shape"], f["mm"]) == (e["shape"], o[1]), (e["name"], surface, mode, f)
                        assert f["waves"] in (4, 8) and 0 < f["lds"] <= 160 * 1024 and f["neus"] == int(surface == "render" and e["geometry"] == "neus")


def test_validator_and_shape_table_agree(lib):
    """check_field_cfg's width and depth rules against the one list of compiled shapes (NGM_FWD_SHAPES): over every Fourier
    (dim_enc, dim_hidden, num_layers) the validator either refuses, or the forward plan of each surface finds a compiled shape
    -- the plan's own "no forward kernel" refusal is unreachable in the full build -- and every compiled shape is reached."""
    fc, rc = K.field_cfg(), K.render_cfg(num_samples_coarse=5, num_samples_guided=2)
    reached = set()
    for L_ in range(1, K.NGM_MAX_LAYERS + 1):
        for D in range(3, 65):
            for H in range(1, 65):
                fc.dim_enc, fc.dim_hidden, fc.num_layers = D, H, L_
                got = [_plan_fwd(lib, fc, rc if s == "render" else None, s, 3, 37) for s in ("render", "points", "knn")]
                assert len({g[0] for g in got}) == 1 and got[0][0] in (K.NGM_OK, K.NGM_E_UNSUPPORTED), (D, H, L_, got)
                if got[0][0] == K.NGM_OK:
                    assert len({g[1]["shape"] for g in got}) == 1 and got[0][1]["shape"] in CM.FORWARD_SHAPES, (D, H, L_, got)
                    reached.add(got[0][1]["shape"])
                else:
                    assert "no forward kernel" not in lib.ngm_last_error().decode(), (D, H, L_)
    assert reached == set(CM.FORWARD_SHAPES)


def test_neus_fused_rule_is_the_plans(lib):
    """NeuralGraphRenderer._neus_fused (which neus configurations take the fused step rather than the staged one) says what the
    forward plan says about the fused forward with geometry neus, for every entry that has a forward at all."""
    import types
    from neural_graph_mapping_amd.renderer import NeuralGraphRenderer
    rc = K.render_cfg(geometry_mode="neus", num_samples_coarse=5, num_samples_guided=2)
    seen = set()
    for e in CM.ENTRIES:
        if e["shape"] is None:
            continue
        for mode in ("f32", "auto"):
            fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
            status, f = _plan_fwd(lib, fc, rc, "render", 3, 37)
            rule = NeuralGraphRenderer._neus_fused(types.SimpleNamespace(_fc=fc))
            assert rule == (status == K.NGM_OK), (e["name"], mode)
            assert status in (K.NGM_OK, K.NGM_E_UNSUPPORTED) and (status != K.NGM_OK or (f["neus"] == 1 and f["mm"] == "f32"))
            seen.add(rule)
    assert seen == {True, False}


ONE_TILE_NETS = ("fourier64_L2", "hash16_L1")


def _one_tile(lib, name, F):
    """512 rays x (8 + 16) samples per field, mode auto: rays per wave x samples per ray <= 32 at F = 4 (256 CUs: 64 workgroups of
    8 rays per field, one ray per wave), not at F = 8 (16 rays per workgroup, two per wave)"""
    fc = K.field_cfg(**CM.BY_NAME[name]["fkw"], matmul_mode="auto")
    status, f = _plan_fwd(lib, fc, K.render_cfg(num_samples_coarse=8, num_samples_guided=16), "render", F, 512)
    assert status == K.NGM_OK
    return f["one_tile"]


def test_one_tile_wave_step_is_planned_for_small_batches_only(lib):
    """The one-tile rule without a GPU (the library assumes the MI355X's 256 CUs there), and its switch: with NGM_NO_HALF_STEP=1
    (read once per process: a child process) no plan is one-tile."""
    import os
    import subprocess
    import sys
    for name in ONE_TILE_NETS:
        assert (_one_tile(lib, name, 4), _one_tile(lib, name, 8)) == (1, 0), name
    code = ("import sys; sys.path[:0] = %r; import test_config_matrix_cpu as T; from neural_graph_mapping_amd import _capi as K; "
            "print([T._one_tile(K.lib(), n, F) for n in T.ONE_TILE_NETS for F in (4, 8)])" % (sys.path,))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NGM_NO_HALF_STEP="1"), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "[0, 0, 0, 0]", (r.stdout, r.stderr[-2000:])
