"""CPU companion of tests/test_gpu_config_matrix.py: the table of tests/_config_matrix.py builds and evaluates in the oracle,
its fused-step problems can be made kink-free inside the usual cap, it is internally consistent, and the library's validator
draws the line where the table says it does (argument validation needs no GPU)."""
import ctypes as C

import pytest
import torch

import _config_matrix as CM
from gpu_common import matrix_knn_case, matrix_points_case, matrix_step_case
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


def test_plan_query_reproduces_the_step_and_autograd_columns(lib):
    """The backward plan (plan_mlp_bwd behind ngm_debug_plan_bwd: no launch, no GPU) against every (entry, mode) cell of the
    `step` and `autograd` columns: forward arithmetic, backward variant and fusion flag at both STEP_SHAPES; the point
    evaluation's variant at P = 257 with a stash offered and without; three-layer entries refused with NGM_E_UNSUPPORTED.
    Left out: the cells whose refusal is the forward launcher's (explicit bf16x3 outside its shape), not the plan's."""
    arithmetic = {K.MATMUL["f32"]: "f32", K.MATMUL["bf16x3"]: "bf16x3"}
    skipped = set()
    for e in CM.ENTRIES:
        if e["shape"] is None:
            continue
        for mode, o in e["step"].items():
            fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
            for F, R, n_c, n_g in CM.STEP_SHAPES:
                rc = K.render_cfg(geometry_mode=e["geometry"], num_samples_coarse=n_c, num_samples_guided=n_g)
                status, variant, fused, kind, layers, mm = _plan(lib, fc, rc, F, R)
                if o == CM.REFUSE and fc.num_layers <= 2:
                    skipped.add((e["name"], mode))
                elif o == CM.REFUSE:
                    assert status == K.NGM_E_UNSUPPORTED and "forward only" in lib.ngm_last_error().decode(), (e["name"], mode)
                else:
                    assert status == K.NGM_OK and (arithmetic[mm], variant, fused) == o[1:], (e["name"], mode, (F, R))
                    assert (variant not in (2, 3, 5) or kind == (2 if variant == 5 else 1)) and (layers > 0) == (kind != 0)
        for mode, o in e["autograd"].items():
            fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
            got = [_plan(lib, fc, None, 3, 257, stash_offered=s) for s in (1, 0)]
            if o == CM.REFUSE:
                assert fc.num_layers == 3 and [g[0] for g in got] == [K.NGM_E_UNSUPPORTED] * 2, (e["name"], mode)
            else:
                assert [g[:2] for g in got] == [(K.NGM_OK, o[1]), (K.NGM_OK, o[2])], (e["name"], mode)
                assert [g[3] for g in got] == [int(o[1] == 3), 0] and all(g[2] == 0 for g in got)    # only k_field_bwd_b3 reads a stash
    forward_refusals = {(e["name"], mode) for e in CM.ENTRIES if e["shape"] is not None for mode, o in e["render"].items()
                        if o == CM.REFUSE and e["fkw"]["num_layers"] <= 2}
    assert skipped == forward_refusals and len(skipped) <= 2
