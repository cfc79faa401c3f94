"""16-bit weight storage on every surface of every accepted configuration: bit for bit the fp32 twin, or the table's refusal.

The promise (ops.params_struct, csrc/ngm_device.h "reduced-precision parameter STORAGE"): `weight_dtype: bfloat16 | float16` is
storage only -- a 16-bit element is widened exactly where a field is staged or the hash table gathered, all arithmetic is fp32.
So a field set whose fp32 masters hold 16-bit-representable values computes the same bits from either storage.  Six pieces of
staging code keep that promise, each with its own vector-load decision, ragged tail and column split:

  FieldStage::issue      csrc/ngm_field.h            every forward shape, k_field_bwd (variant 0)
  FieldStage16::issue    csrc/ngm_bwd16.h            k_field_bwd16 (variant 1), k_field_bwd16s (variant 2)
  b3 prologue gathers    csrc/ngm_bwd_b3.h, ngm_field_bwd_b3.hip     k_field_bwd_b3 (variant 3)
  k_hash_mlp_bwd prologue  csrc/ngm_hash_bwd.hip     variant 5
  hash table gather      ngm_ldp2 / ngm_ldp2x4       every hash forward and backward
  standalone encode      csrc/ngm_field_fwd.hip      ngm_encode_fwd, ngm_encode_bwd

The table is tests/_config_matrix.py (CM.storage16: the entry's own outcome -- same arithmetic, backward variant, comp_fused,
asserted after every run so that like is compared with like; the triplane entry refuses).  The twin problem is
gpu_common.matrix_storage_twin: the matrix case's parameters rounded to the storage type, once kept as fp32, once converted.
Every comparison is torch.equal: the reference is exact, no tolerance exists here.  A fault in a staging routine is silent --
a tail element read from the next row, the halves of a packed pair swapped, a padded column that is not zero all give
plausible numbers -- and any of them breaks equality.

Non-vacuity, in every test: outputs finite, every gradient tensor non-zero, the twin's result differs from the unrounded
case's (rounding moved the problem), and the fp32 twin's point evaluation meets the fp64 oracle AT THE ROUNDED PARAMETERS at
the entry's forward bar (_anchored: the twin is a correct evaluation of the rounded network, not merely equal to its sibling).

Padded row strides (section 9 below): params_struct hands any stride(0) to the kernels as long as a row is contiguous.  Every
staging routine either tests the row address before a vector load (FieldStage::issue, FieldStage16::issue: `vec`) or loads
element by element (ngm_ldp / ngm_ldp_gather: the b3 and k_hash_mlp_bwd prologues, the output layer, biases, Fourier weights,
the encode stage); the hash gather loads one whole entry (4 / 8 bytes), and a table padded by whole entries keeps entries
naturally aligned.  With one extra element per row, odd rows start 2-byte aligned (16-bit) / 4-byte aligned (fp32): entries
with Din % 4 == 0 then take the `vec == false because the row address is misaligned` branch in rows 1, 3, ... and the vector
branch in rows 0, 2, ...; the result must equal the contiguous run's bit for bit, in all three storage types."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import _config_matrix as CM  # noqa: E402
from gpu_common import (DEV, NRGBD_KW, close, cu, make_renderer, make_target, matrix_knn_case, matrix_points_case,  # noqa: E402
                        matrix_step_case, matrix_storage_twin, matrix_twin_oracle)
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from test_gpu_config_matrix import (_fwd_bar, _next_call_succeeds, _refused, _renderer, _reported, _state,  # noqa: E402
                                    _step_matches)

L = K.lib
DT = {"bfloat16": torch.bfloat16, "float16": torch.float16}
NAME_DT = [(n, wd) for n in CM.NAMES for wd in CM.STORAGE]
name_dt = pytest.mark.parametrize("name,wd", NAME_DT, ids=[f"{n}-{wd}" for n, wd in NAME_DT])
shapes = pytest.mark.parametrize("shape", CM.STEP_SHAPES, ids=lambda s: "x".join(map(str, s)))


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a, b), (what, f"{int((a != b).sum())} of {a.numel()} elements differ, max |diff| "
                                     f"{float((a.double() - b.double()).abs().max()):.3e}")


def _same_bits(a, b, what):
    """scalars that may legitimately be NaN (a loss term whose selection is empty): the bit patterns"""
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), (what, a, b)


def _finite(t, what):
    assert bool(torch.isfinite(t).all()), what


def _moved(a, b, what):
    assert not torch.equal(a, b), f"{what}: rounding the weights did not change the result -- a vacuous comparison"


def _grads_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        _finite(a[k], (what, k))
        assert k in K.NO_GRAD_PARAMS or bool(a[k].any()), (what, k, "an all-zero gradient compares nothing")
        _same(a[k], b[k], (what, k))


def _refused_storage(exc):
    assert isinstance(exc.value, K.NgmError) and exc.value.code == K.NGM_E_INVALID, exc.value
    assert "triplane encoding needs fp32 planes" in str(exc.value)


def _refusal(expect):
    return _refused_storage if expect == CM.REFUSE_STORAGE else _refused


_ANCHORED = {}


def _anchored(e, wd):
    """the fp32 twin's point evaluation (P = 257, mode f32) against the fp64 oracle at the rounded parameters, at the entry's
    forward bar: once per entry and storage type"""
    if (e["name"], wd) in _ANCHORED or not CM.runs(e["points"]["f32"]):
        return
    c = matrix_points_case(e, 257)
    tw = matrix_storage_twin(c, DT[wd])
    with torch.no_grad():
        out = ops.field_eval(K.field_cfg(**e["fkw"], matmul_mode="f32"), cu(tw["f32"]), c["q"].to(DEV), c["pos"].to(DEV),
                             c["quat"].to(DEV))
    close(out, matrix_twin_oracle(e, DT[wd]), **_fwd_bar(e, "points"))
    _ANCHORED[(e["name"], wd)] = True


def _unchanged(params, before):
    for k, v in params.items():
        assert torch.equal(v, before[k]), (k, "a refused call changed a parameter")


# ------------------------------------------------------------------------------------------------ 1: point evaluation, forward
@name_dt
def test_points_forward(name, wd):
    e = CM.BY_NAME[name]
    refused = False
    _anchored(e, wd)
    for mode in CM.modes(e, "points"):
        expect = CM.storage16(e, "points", mode)
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        for P in (1, 257):
            c = matrix_points_case(e, P)
            tw = matrix_storage_twin(c, DT[wd])
            args = (c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
            with torch.no_grad():
                if CM.runs(expect):
                    a = ops.field_eval(fc, cu(tw["f32"]), *args)
                    assert _reported(1) == expect[1], (mode, P)
                    b = ops.field_eval(fc, cu(tw["lp"]), *args)
                    assert _reported(1) == expect[1], (mode, P)
                    _finite(a, (mode, P))
                    _same(b, a, ("points", mode, P))
                    _moved(a, ops.field_eval(fc, cu(c["params"]), *args), ("points", mode, P))
                else:
                    lp = cu(tw["lp"])
                    before = {k: v.clone() for k, v in lp.items()}
                    with pytest.raises(K.NgmError) as exc:
                        ops.field_eval(fc, lp, *args)
                    _refusal(expect)(exc)
                    _unchanged(lp, before)
                    refused = True
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 2: point evaluation, autograd
def _eval_bwd_ops(fc, params, q, pos, quat, d_out):
    """The two ops behind ops.field_eval's autograd formula, dispatched as it dispatches them, called directly -> (output,
    {trainable name: fp32 gradient}).  The backward ops return fp32 gradients whatever the storage; the autograd engine then
    casts a gradient to its leaf's type, so the `.grad` of a 16-bit leaf is that gradient rounded -- by PyTorch, not by a kernel
    (the product differentiates the fp32 masters).  The bitwise comparison of the two storages is made on what the ops return."""
    names = K.param_names(fc)
    plist = [params[n] for n in names]
    blob = ops.cfg_blob(fc)
    sb = int(L().ngm_field_eval_stash_bytes(C.byref(fc), q.shape[0], q.shape[1]))
    if 0 < sb <= ops.FIELD_EVAL_STASH_MAX_BYTES:
        out, stash = torch.ops.ngm355.field_eval_train(blob, q, pos, quat, plist)
        g = torch.ops.ngm355.field_eval_bwd_stash(blob, q, pos, quat, d_out, stash, plist)
    else:
        out = torch.ops.ngm355.field_eval(blob, q, pos, quat, plist)
        g = torch.ops.ngm355.field_eval_bwd(blob, q, pos, quat, d_out, plist)
    return out, {n: x for n, x in zip(names, g) if n not in K.NO_GRAD_PARAMS}


@name_dt
def test_points_autograd(name, wd):
    e = CM.BY_NAME[name]
    c = matrix_points_case(e, 257)
    tw = matrix_storage_twin(c, DT[wd])
    args = (c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
    refused = False
    _anchored(e, wd)
    for mode in CM.modes(e, "autograd"):
        expect = CM.storage16(e, "autograd", mode)
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        keep = ops.FIELD_EVAL_STASH_MAX_BYTES
        try:
            for i, stash_max in enumerate((keep, 0)):       # with the activation stash, then the recomputing backward
                ops.FIELD_EVAL_STASH_MAX_BYTES = stash_max

                def run(params):
                    pg = {k: v.to(DEV).requires_grad_(k not in K.NO_GRAD_PARAMS) for k, v in params.items()}
                    out = ops.field_eval(fc, pg, *args)
                    (out * c["d_out"].to(DEV)).sum().backward()
                    return out.detach(), {k: v.grad for k, v in pg.items() if v.requires_grad}
                if CM.runs(expect):
                    a, ga = run(tw["f32"])
                    assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                    b, gb = run(tw["lp"])
                    assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                    _finite(a, (mode, stash_max))
                    _same(b, a, ("autograd", mode, stash_max))
                    # the kernels' own fp32 gradients, from the two ops behind the autograd formula
                    a2, da = _eval_bwd_ops(fc, cu(tw["f32"]), *args, c["d_out"].to(DEV))
                    assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                    b2, db = _eval_bwd_ops(fc, cu(tw["lp"]), *args, c["d_out"].to(DEV))
                    assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                    _same(a2, a, ("autograd ops", mode, stash_max))
                    _same(b2, a, ("autograd ops", mode, stash_max))
                    assert all(g.dtype == torch.float32 for g in db.values())
                    _grads_same(db, da, ("autograd ops", mode, stash_max))
                    _grads_same(ga, da, ("autograd, fp32 leaves", mode, stash_max))
                    for k, g in gb.items():          # what the engine leaves in a 16-bit leaf: that fp32 gradient, cast
                        _same(g, da[k].to(DT[wd]), ("autograd, 16-bit leaves", mode, stash_max, k))
                    if i == 0:
                        _moved(a, run(c["params"])[0], ("autograd", mode))
                else:
                    pg = {k: v.to(DEV).requires_grad_(k not in K.NO_GRAD_PARAMS) for k, v in tw["lp"].items()}
                    before = {k: v.detach().clone() for k, v in pg.items()}
                    with pytest.raises(K.NgmError) as exc:
                        out = ops.field_eval(fc, pg, *args)
                        (out * c["d_out"].to(DEV)).sum().backward()
                    _refusal(expect)(exc)
                    refused = True
                    for k, v in pg.items():
                        assert v.grad is None or not bool(v.grad.any()), k
                    _unchanged({k: v.detach() for k, v in pg.items()}, before)
        finally:
            ops.FIELD_EVAL_STASH_MAX_BYTES = keep
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 3: fused training step
LOSS_SKIP = ("grads", "prediction")


def _snap(res):
    """the renderer's result lives in its workspace: a copy that survives the next call"""
    p = res["prediction"]
    s = dict(rgbds=p.rgbds.clone(), term_probs=p.term_probs.clone(), color_vars=p.color_vars.clone(),
             depth_vars=p.depth_vars.clone(), loss={k: v.clone() for k, v in res.items() if k not in LOSS_SKIP})
    if "grads" in res:
        s["grads"] = {k: v.clone() for k, v in res["grads"].items()}
    return s


def _steps_same(a, b, what, grads=True):
    for k in ("rgbds", "term_probs", "color_vars", "depth_vars"):
        _finite(a[k], (what, k))
        _same(b[k], a[k], (what, k))
    assert a["loss"].keys() == b["loss"].keys()
    for k in a["loss"]:
        _same_bits(b["loss"][k], a["loss"][k], (what, k))
    # (a loss term whose selection is empty is NaN, and so is `combined` then: compared as bits above, like compare_losses does)
    assert any(bool(torch.isfinite(v)) for v in a["loss"].values()), (what, "every loss term is NaN")
    if grads:
        _grads_same(b["grads"], a["grads"], what)


def _twin_case(c, wd):
    return dict(c, params=matrix_storage_twin(c, DT[wd])["f32"])


def _trainable(k):
    return k not in K.NO_GRAD_PARAMS


def _updated_same(ra, rb, wd, what, rows=None):
    """after one update=True step from the same state: masters and both moments of the 16-bit renderer `rb` equal the fp32
    twin's `ra` after its own step, every 16-bit copy is the rounded master; the step moved something (rows: the selected ones)"""
    sa, sb = _state(ra), _state(rb)
    moved = False
    for k, v in sa.items():
        _same(sb[k], v, (what, "update", k))
        _finite(v, (what, k))
    for k, v in rb._model.all_fields_params.items():
        if _trainable(k) and k != "_neus_sd":
            _same(rb._model.lp_fields_params[k], v.to(DT[wd]), (what, "16-bit copy", k))
            sel = v if rows is None else v[rows]
            moved |= float((sel - sel.to(DT[wd]).float()).abs().max()) > 0
    assert moved, (what, "the step left every master representable: nothing was updated")
    assert ra._step == rb._step == 1


@shapes
@name_dt
def test_fused_step(name, wd, shape):
    e = CM.BY_NAME[name]
    c = matrix_step_case(e, shape)
    ids = torch.arange(c["F"])
    jit = (c["u_c"].to(DEV), c["u_g"].to(DEV))
    refused = False
    _anchored(e, wd)
    for mode in CM.modes(e, "step"):
        expect = CM.storage16(e, "step", mode)
        if expect == CM.REFUSE_STORAGE:
            with pytest.raises(NotImplementedError, match="not built for the triplane encoding"):
                _renderer(e, c, mode, weight_dtype=wd)
            continue
        ct = _twin_case(c, wd)
        tgt = make_target(c["t"], ids)
        ra, rb = _renderer(e, ct, mode), _renderer(e, ct, mode, weight_dtype=wd)
        assert rb._model.lp_fields_params["_linears.0.weight"].dtype == DT[wd] and ra._model.lp_fields_params is None
        if not CM.runs(expect):
            refused = True
            for update in (False, True):
                before, step0 = _state(rb), rb._step
                with pytest.raises(K.NgmError) as exc:
                    rb.optimization_iteration(tgt, *jit, update=update)
                _refused(exc)
                torch.cuda.synchronize()
                after = _state(rb)
                assert before.keys() == after.keys()
                for k, v in before.items():
                    assert torch.equal(v, after[k]), k
                assert rb._step == step0 and (rb._step_dev is None or int(rb._step_dev) == step0)
            continue
        snaps = []
        for r in (ra, rb):
            snaps.append(_snap(r.optimization_iteration(tgt, *jit, update=False)))
            torch.cuda.synchronize()
            assert (_reported(0), L().ngm_debug_last_bwd_variant(), L().ngm_debug_last_comp_fused()) == expect[1:], mode
        _steps_same(snaps[0], snaps[1], ("step", mode))
        _moved(snaps[0]["rgbds"], _snap(_renderer(e, c, mode).optimization_iteration(tgt, *jit, update=False))["rgbds"], ("step", mode))
        # one update from the same state (update=False moved nothing); one only: afterwards the twin's masters are no longer representable
        ups = []
        for r in (ra, rb):
            ups.append(_snap(r.optimization_iteration(tgt, *jit, update=True)))
            torch.cuda.synchronize()
            assert (_reported(0), L().ngm_debug_last_bwd_variant(), L().ngm_debug_last_comp_fused()) == expect[1:], mode
        _steps_same(ups[0], ups[1], ("step update", mode), grads=False)
        _updated_same(ra, rb, wd, ("step", mode))
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 3b: rows that are not the identity
# one entry per backward variant; the case's three fields live in rows [F + 1, 0, 2] of a set of F + 2
SUBSET = {0: ("fourier_20to32_concat_L2", "auto"), 1: ("fourier_33to48_L1", "auto"), 2: ("fourier_61to64_L2", "f32"),
          3: ("fourier64_L2", "auto"), 5: ("hash9_T8_L1", "auto")}


def _in_rows(c, params, ids, seed):
    """the case's fields in the rows `ids` of a set of F + 2 fields; the other rows hold other fields (16-bit representable,
    like the twin's)"""
    from oracle import ngm_oracle as O
    n = c["F"] + 2
    g = torch.Generator().manual_seed(seed)
    full = {k: v.to(torch.bfloat16).float() if _trainable(k) else v for k, v in O.init_params(c["fs"], n, seed=seed, sigma=3.0).items()}
    pos, quat = torch.randn(n, 3, generator=g), torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1)
    for k in full:
        full[k][ids] = params[k]
    pos[ids], quat[ids] = c["pos"], c["quat"]
    return dict(c, F=n, params=full, pos=pos, quat=quat)


@pytest.mark.parametrize("wd", CM.STORAGE)
@pytest.mark.parametrize("variant", CM.BWD_VARIANTS)
def test_fused_step_rows_not_identity(variant, wd):
    name, mode = SUBSET[variant]
    e = CM.BY_NAME[name]
    expect = CM.storage16(e, "step", mode)
    assert expect[2] == variant
    c = matrix_step_case(e, CM.STEP_SHAPES[0])
    assert c["F"] == 3 and c["sd"] is None
    ids = torch.tensor([c["F"] + 1, 0, 2])
    rest = torch.tensor([1, 3])
    _anchored(e, wd)
    # the subset path against the reference: the unrounded case in those rows, fp32 storage, the case's own cached oracle results
    _step_matches(e, c, mode, expect, r=_renderer(e, _in_rows(c, c["params"], ids, 4242), mode), ids=ids)
    c5 = _in_rows(c, matrix_storage_twin(c, DT[wd])["f32"], ids, 4242)
    tgt = make_target(c["t"], ids)
    jit = (c["u_c"].to(DEV), c["u_g"].to(DEV))
    ra, rb = _renderer(e, c5, mode), _renderer(e, c5, mode, weight_dtype=wd)
    snaps = []
    for r in (ra, rb):
        snaps.append(_snap(r.optimization_iteration(tgt, *jit, update=False)))
        torch.cuda.synchronize()
        assert (_reported(0), L().ngm_debug_last_bwd_variant(), L().ngm_debug_last_comp_fused()) == expect[1:]
    _steps_same(snaps[0], snaps[1], ("rows", variant))
    # the same fields in rows 0..2 of a set of three give the same bits: the row selection selects, nothing else
    r3 = _renderer(e, _twin_case(c, wd), mode, weight_dtype=wd)
    _steps_same(snaps[1], _snap(r3.optimization_iteration(make_target(c["t"], torch.arange(3)), *jit, update=False)), ("rows vs identity", variant))
    before = _state(rb)
    for r in (ra, rb):
        r.optimization_iteration(tgt, *jit, update=True)
        torch.cuda.synchronize()
        assert L().ngm_debug_last_bwd_variant() == variant
    _updated_same(ra, rb, wd, ("rows", variant), rows=ids.to(DEV))
    after = _state(rb)
    for k, v in before.items():
        _same(after[k][rest.to(DEV)], v[rest.to(DEV)], ("rows not selected", k))            # masters, moments and copies
        pname = k.split("::", 1)[1]
        if _trainable(pname) and pname != "_neus_sd":
            assert not torch.equal(after[k][ids.to(DEV)], v[ids.to(DEV)]), ("rows selected did not move", k)


# ------------------------------------------------------------------------------------------------ 4: fused render forward
def _render(e, c, mode, params, wd=None):
    """ops.render_ijs_fused under no_grad; neus through the renderer, which passes the per-field `_neus_sd`
    (test_gpu_config_matrix.test_fused_render_forward)"""
    if e["geometry"] == "neus":
        r = _renderer(e, dict(c, params={k: v.float() for k, v in params.items()}), mode, **({"weight_dtype": wd} if wd else {}))
        ctx = r._iteration_forward(make_target(c["t"], torch.arange(c["F"])), c["u_c"].to(DEV), c["u_g"].to(DEV), advance=False)
        return tuple(ctx["w"][k].clone() for k in ("rgbds", "color_vars", "depth_vars", "term_probs"))
    cam = Rr.Camera(640, 480, NRGBD_KW["fx"], NRGBD_KW["fy"], 319.5, 239.5, pixel_center=0.0)
    rc = Rr.make_render_cfg(cam, Rr.shipped_config(**c["ckw"]), guided=True)
    t = cu(c["t"])
    with torch.no_grad():
        out = ops.render_ijs_fused(K.field_cfg(**e["fkw"], matmul_mode=mode), rc, params, t["ijs"], t["c2ws"], t["near"], t["far"],
                                   t["gt"], c["pos"].to(DEV), c["quat"].to(DEV), c["u_c"].to(DEV), c["u_g"].to(DEV))
    return out[:4]


@shapes
@name_dt
def test_fused_render_forward(name, wd, shape):
    e = CM.BY_NAME[name]
    c = matrix_step_case(e, shape)
    tw = matrix_storage_twin(c, DT[wd])
    refused = False
    _anchored(e, wd)
    for mode in CM.modes(e, "render"):
        expect = CM.storage16(e, "render", mode)
        if CM.runs(expect):
            a = _render(e, c, mode, cu(tw["f32"]))
            assert _reported(0) == expect[1], mode
            b = _render(e, c, mode, cu(tw["lp"]), wd)
            assert _reported(0) == expect[1], mode
            for x, y, k in zip(a, b, ("rgbds", "color_vars", "depth_vars", "term_probs")):
                _finite(x, (mode, k))
                _same(y, x, ("render", mode, k))
            _moved(a[0], _render(e, c, mode, cu(c["params"]))[0], ("render", mode))
        else:
            lp = cu(tw["lp"])
            before = {k: v.clone() for k, v in lp.items()}
            with pytest.raises(K.NgmError) as exc:
                _render(e, c, mode, lp, wd)
            _refusal(expect)(exc)
            _unchanged(lp, before)
            refused = True
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 5: kNN evaluation
@name_dt
def test_knn_evaluation(name, wd):
    e = CM.BY_NAME[name]
    c = matrix_knn_case(e)
    tw = matrix_storage_twin(c, DT[wd])
    g = torch.Generator().manual_seed(5)
    sub = torch.randperm(c["NF"], generator=g)[:c["NF"] - 2]              # a shuffled proper subset of the rows
    assert not torch.equal(sub, sub.sort().values)
    refused = False
    _anchored(e, wd)
    for mode in CM.modes(e, "knn"):
        expect = CM.storage16(e, "knn", mode)
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        pts = c["pts"].to(DEV)

        def run(params, rows=None):
            pos, quat = (c["pos"], c["quat"]) if rows is None else (c["pos"][rows], c["quat"][rows])
            return ops.field_eval_knn(fc, params, pts, pos.to(DEV), quat.to(DEV), c["K"], 10.0, 1.0,
                                      field_index=None if rows is None else rows.to(DEV))
        if CM.runs(expect):
            outs = []
            for rows in (None, sub):
                a = run(cu(tw["f32"]), rows)
                assert _reported(2) == expect[1], mode
                b = run(cu(tw["lp"]), rows)
                assert _reported(2) == expect[1], mode
                _finite(a, (mode, rows))
                _same(b, a, ("knn", mode, rows))
                assert 0 < int((a != 1.0).any(-1).sum()) < c["P"]            # points inside and outside the fields
                _moved(a, run(cu(c["params"]), rows), ("knn", mode, rows))
                outs.append(a)
            assert not torch.equal(outs[0], outs[1])                         # the subset is another map
        else:
            lp = cu(tw["lp"])
            before = {k: v.clone() for k, v in lp.items()}
            with pytest.raises(K.NgmError) as exc:
                run(lp)
            _refusal(expect)(exc)
            _unchanged(lp, before)
            refused = True
    if refused:
        _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 6: standalone encode stage
ENCODED = [n for n in CM.NAMES if CM.BY_NAME[n]["fkw"]["encoding"] in ("fourier", "permuto")]
ENC_PARAM = {"fourier": "_encoding._linear.weight", "permuto": "_encoding.lattice_values"}


@pytest.mark.parametrize("wd", CM.STORAGE)
@pytest.mark.parametrize("name", ENCODED)
def test_encode_stage(name, wd):
    """ops.encode / ops.encode_bwd: the stage reads the encoding's own tensor, element by element (Fourier) or entry by entry
    (hash); the network behind it is not evaluated and its depth rule not applied (check_field_cfg(fc, false)): the stage runs for
    the entries every other surface refuses, too"""
    e = CM.BY_NAME[name]
    c = matrix_points_case(e, 257)
    tw = matrix_storage_twin(c, DT[wd])
    fc = K.field_cfg(**e["fkw"])
    args = (c["pos"].to(DEV), c["quat"].to(DEV))
    q = c["q"].to(DEV)
    d_enc = torch.randn(c["F"], c["P"], fc.dim_enc, generator=torch.Generator().manual_seed(31)).to(DEV)
    _anchored(e, wd)
    a, b = ops.encode(fc, cu(tw["f32"]), q, *args), ops.encode(fc, cu(tw["lp"]), q, *args)
    _finite(a, "encode")
    _same(b, a, "encode")
    _moved(a, ops.encode(fc, cu(c["params"]), q, *args), "encode")
    ga, gb = ops.encode_bwd(fc, cu(tw["f32"]), q, d_enc, *args), ops.encode_bwd(fc, cu(tw["lp"]), q, d_enc, *args)
    assert list(ga) == [ENC_PARAM[e["fkw"]["encoding"]]]
    _grads_same(gb, ga, "encode_bwd")
    if e["fkw"]["encoding"] == "fourier":          # (the hash table's gradient does not depend on the table: nothing to move)
        _moved(ga[ENC_PARAM["fourier"]], ops.encode_bwd(fc, cu(c["params"]), q, d_enc, *args)[ENC_PARAM["fourier"]], "encode_bwd")


# ------------------------------------------------------------------------------------------------ 7: the one-call image path
IMAGE = {"<1,1,1>": "hash9_T8_L1", "<1,1,2>": "fourier_32to17_L2", "<2,2,1>": "fourier_61to64_L1",
         "<2,2,2>": "fourier_40to64_concat_L2", "<2,2,3>": "fourier64_add_L3"}


def _image(e, c, params, mode="auto"):
    """8 x 6 pixels spread over the image, 16 samples per ray, the kNN case's seven fields (K = 3) seen from z = +5 along -z"""
    rows, cols = torch.linspace(0, 479, 6).round().long(), torch.linspace(0, 639, 8).round().long()
    ijs = torch.stack(torch.meshgrid(rows, cols, indexing="ij"), -1).reshape(-1, 2).to(DEV)
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([1.5, 1.5, 5.0])
    rc = K.render_cfg(geometry_mode=e["geometry"], num_samples_coarse=16, num_samples_guided=0, **NRGBD_KW)
    return ops.render_eval_knn(K.field_cfg(**e["fkw"], matmul_mode=mode), rc, params, ijs, c2w.to(DEV), c["pos"].to(DEV),
                               c["quat"].to(DEV), c["K"], 10.0, 1.0, seed=3)


@pytest.mark.parametrize("wd", CM.STORAGE)
@pytest.mark.parametrize("fwd_shape", CM.FORWARD_SHAPES)
def test_image_path(fwd_shape, wd):
    e = CM.BY_NAME[IMAGE[fwd_shape]]
    c = matrix_knn_case(e)
    assert e["shape"] == fwd_shape and c["NF"] == 7 and c["K"] == 3
    tw = matrix_storage_twin(c, DT[wd])
    _anchored(e, wd)
    a, b = _image(e, c, cu(tw["f32"])), _image(e, c, cu(tw["lp"]))
    assert _reported(2) == CM.storage16(e, "knn", "auto")[1]
    for x, y, k in zip(a, b, ("rgbd", "color_vars", "depth_vars", "term")):
        assert x.shape[0] == 48
        _finite(x, k)
        _same(y, x, ("image", k))
    assert float(a[0].std(0).max()) > 0                                     # the rays see different things
    _moved(a[0], _image(e, c, cu(c["params"]))[0], "image")


# ------------------------------------------------------------------------------------------------ 8: refusals of the storage itself
@pytest.mark.parametrize("wd", CM.STORAGE)
def test_triplane_refuses_16_bit_storage(wd):
    """every triplane entry: NotImplementedError where a field set is built (covered per mode in test_fused_step), NGM_E_INVALID
    at the ops level on every surface (tests 1, 2, 4, 5 above); here the table's side of it, and the encode stage"""
    tri = [e for e in CM.ENTRIES if e["fkw"]["encoding"] == "triplane"]
    assert tri
    for e in tri:
        assert all(CM.storage16(e, s, m) == CM.REFUSE_STORAGE for s in CM.SURFACES for m in CM.modes(e, s))
        with pytest.raises(NotImplementedError, match="not built for the triplane encoding"):
            make_renderer({**e["fkw"], "weight_dtype": wd}, dict(num_samples_coarse=5, num_samples_depth_guided=2), 2)
        c = matrix_points_case(e, 257)
        lp = cu(matrix_storage_twin(c, DT[wd])["lp"])
        assert lp["_encoding.plane_coef"].dtype == DT[wd]
        before = {k: v.clone() for k, v in lp.items()}
        with pytest.raises(K.NgmError) as exc:
            ops.encode(K.field_cfg(**e["fkw"]), lp, c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
        _refused_storage(exc)
        _unchanged(lp, before)
    _next_call_succeeds()


# ------------------------------------------------------------------------------------------------ 9: padded row strides
# one entry (at least) per staging routine; Din % 4 == 0 in every layer reaches the misaligned-row branch of `vec`
PADDED = ["fourier64_L2",                   # FieldStage <2,2,2>, FieldStage16 (variant 1, f32), b3 gathers (variant 3, auto); Din 64
          "fourier_20to32_concat_L2",       # FieldStage CAT: Din 20 and 52, H % 4 == 0: both column parts vector-loaded; variant 0
          "fourier_61to64_L1",              # Din 61: never a vector load, ragged tail; variants 3 / 1
          "fourier_20to32_L2",              # FieldStage16<2,2,2> (variant 1); Din 20 / 32
          "fourier64_add_L3",               # FieldStage <2,2,3>
          "hash16_L1"]                      # hash gather (table padded by one whole entry), FieldStage16 (variant 1)
STORED = ("float32",) + CM.STORAGE
POISON = float("nan")                       # what the padding holds: an element read from it shows in the result


def _padded(params):
    """every tensor as rows of a buffer one element longer than the row (the hash table: one entry = two elements longer)"""
    out = {}
    for k, v in params.items():
        n, pad = v[0].numel(), 2 if k == "_encoding.lattice_values" else 1
        buf = torch.full((v.shape[0], n + pad), POISON, dtype=v.dtype, device=v.device)
        buf[:, :n] = v.reshape(v.shape[0], n)
        out[k] = buf[:, :n].view(v.shape)
        assert out[k].stride(0) == n + pad and out[k][0].is_contiguous() and torch.equal(out[k], v)
    return out


def _stored(c, st):
    return cu(c["params"] if st == "float32" else matrix_storage_twin(c, DT[st])["lp"])


@pytest.mark.parametrize("st", STORED)
@pytest.mark.parametrize("name", PADDED)
def test_padded_rows_points_and_autograd(name, st):
    e = CM.BY_NAME[name]
    c = matrix_points_case(e, 257)
    args = (c["q"].to(DEV), c["pos"].to(DEV), c["quat"].to(DEV))
    flat = _stored(c, st)
    pad = _padded(flat)
    for mode in CM.modes(e, "points"):
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        with torch.no_grad():
            a, b = ops.field_eval(fc, flat, *args), ops.field_eval(fc, pad, *args)
        _finite(a, mode)
        _same(b, a, ("padded points", mode))
    for mode in CM.modes(e, "autograd"):
        expect = CM.storage16(e, "autograd", mode)
        if not CM.runs(expect):
            continue
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        keep = ops.FIELD_EVAL_STASH_MAX_BYTES
        try:
            for i, stash_max in enumerate((keep, 0)):
                ops.FIELD_EVAL_STASH_MAX_BYTES = stash_max
                res = []
                for params in (flat, pad):
                    pg = {k: v.detach().requires_grad_(k not in K.NO_GRAD_PARAMS) for k, v in params.items()}
                    assert all(pg[k].stride() == params[k].stride() for k in pg)
                    out = ops.field_eval(fc, pg, *args)
                    (out * c["d_out"].to(DEV)).sum().backward()
                    assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                    res.append((out.detach(), {k: v.grad.contiguous() for k, v in pg.items() if v.requires_grad}))
                _same(res[1][0], res[0][0], ("padded autograd", mode, stash_max))
                _grads_same(res[1][1], res[0][1], ("padded autograd", mode, stash_max))
                # (a 16-bit leaf's .grad is the engine's cast of the fp32 gradient: the ops' own fp32 gradients as well)
                (oa, da), (ob, db) = (_eval_bwd_ops(fc, p, *args, c["d_out"].to(DEV)) for p in (flat, pad))
                assert L().ngm_debug_last_bwd_variant() == expect[1 + i], (mode, stash_max)
                _same(ob, oa, ("padded autograd ops", mode, stash_max))
                _grads_same(db, da, ("padded autograd ops", mode, stash_max))
        finally:
            ops.FIELD_EVAL_STASH_MAX_BYTES = keep


@pytest.mark.parametrize("st", STORED)
@pytest.mark.parametrize("name", PADDED)
def test_padded_rows_render_knn_encode(name, st):
    e = CM.BY_NAME[name]
    c = matrix_step_case(e, CM.STEP_SHAPES[0])
    flat = _stored(c, st)
    for mode in CM.modes(e, "render"):
        if not CM.runs(CM.storage16(e, "render", mode)):
            continue
        a, b = _render(e, c, mode, flat), _render(e, c, mode, _padded(flat))
        for x, y, k in zip(a, b, ("rgbds", "color_vars", "depth_vars", "term_probs")):
            _finite(x, (mode, k))
            _same(y, x, ("padded render", mode, k))
    c = matrix_knn_case(e)
    flat = _stored(c, st)
    pad = _padded(flat)
    sub = torch.tensor([5, 1, 6, 3])                                          # odd and even rows, out of order
    for mode in CM.modes(e, "knn"):
        fc = K.field_cfg(**e["fkw"], matmul_mode=mode)
        for rows in (None, sub):
            pos, quat = (c["pos"], c["quat"]) if rows is None else (c["pos"][rows], c["quat"][rows])
            a, b = (ops.field_eval_knn(fc, p, c["pts"].to(DEV), pos.to(DEV), quat.to(DEV), c["K"], 10.0, 1.0,
                                       field_index=None if rows is None else rows.to(DEV)) for p in (flat, pad))
            _finite(a, (mode, rows))
            _same(b, a, ("padded knn", mode, rows))
    c = matrix_points_case(e, 257)
    flat = _stored(c, st)
    pad = _padded(flat)
    fc = K.field_cfg(**e["fkw"])
    args = (c["pos"].to(DEV), c["quat"].to(DEV))
    q = c["q"].to(DEV)
    d_enc = torch.randn(c["F"], c["P"], fc.dim_enc, generator=torch.Generator().manual_seed(31)).to(DEV)
    a, b = ops.encode(fc, flat, q, *args), ops.encode(fc, pad, q, *args)
    _finite(a, "encode")
    _same(b, a, "padded encode")
    _grads_same(ops.encode_bwd(fc, pad, q, d_enc, *args), ops.encode_bwd(fc, flat, q, d_enc, *args), "padded encode_bwd")


def test_padded_entries_cover_the_staging_routines():
    """the table's side of section 9: what PADDED reaches, from the table alone"""
    variants, shapes_, cat = set(), set(), False
    for n in PADDED:
        e = CM.BY_NAME[n]
        shapes_.add(e["shape"])
        cat |= e["fkw"].get("skip_mode") == "concat"
        for o in e["autograd"].values():
            if CM.runs(o):
                variants.update(o[1:])
    assert variants == {0, 1, 3} and cat                 # (variants 2 and 5 exist in the fused step only: no ops-level surface)
    assert shapes_ >= {"<1,1,1>", "<1,1,2>", "<2,2,1>", "<2,2,2>", "<2,2,3>"}
    assert any(CM.is_hash(CM.BY_NAME[n]) for n in PADDED)
