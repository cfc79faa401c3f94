"""The hash encoding's kernels against their float32 restatement at rounding-level bars.

Every other comparison of the permutohedral hash encoding runs against the fp64 oracle or on inputs that differ by the fp32
rounding of the world -> field transform, and its bars absorb the conditioning of the INPUT (a lattice coordinate of 1e4-1e5
turns a position error of 1e-7 into a weight error of 5e-3).  Here the reference is `oracle.ngm_oracle.permuto_simplex` run
in float32 on the very field-frame tensor handed to the kernel (scale_mode "no", no pose): equal hashed indices, weights
equal to an ulp.  What is left is the kernels' own arithmetic, and every bar below is derived from it (eps = 2^-24), none
fitted to what a kernel produced:

  forward (ops.encode, k_encode_points)        |E - E_ref| <= 16 eps M                M = max |table value| of the four vertices
      four fmaf roundings of a partial sum that never exceeds M (weights >= 0, sum 1): 4 eps M; an allowance of 2 eps
      (absolute) on each of the four weights: 8 eps M; together 12 eps M, 16 leaves a margin.  (The allowance was sized for
      bw[0] associated as d3 + (1 + (0 - d0)) against the restatement's (d3 + 1) - d0.  The kernel now associates it as the
      restatement does: an absolute deviation of an ulp of 1 is no RELATIVE deviation of a small weight, and the table
      gradient below, whose bar is relative to the terms d w, missed its bar by up to 3.4x with the other association.)
  forward (ops.field_eval, encode_hash)        the above + 4 eps |E_ref|
      through a pass-through network (W0 = I, one-hot output rows): two matrix passes of one non-zero product each, 2 eps
      per pass allowed.  Both `mlp_matmul` settings resolve to the fp32 MFMA for this network (asserted), so the bf16 split
      is not involved; it would be exact on these weights as well (b3_split is an exact three-way truncation split and the
      weight 1.0 has a high part only).
  table gradient (ops.encode_bwd, k_hash_grad) |G - G_ref| <= eps (4 + c_s) A + n 2^-40 + eps |G_ref|
      G_ref = float64 sum of v = float32(d w32) (the kernel's one product rounding), A = sum |v|, n = number of terms of the
      entry.  4: product rounding and weight deviation.  n 2^-40: `to_fix` truncates every converted value toward zero by
      less than 2^-40 (a merged run converts once, so n bounds it).  eps |G_ref|: the final conversion to float.
      c_s = 0 on inputs without runs.  Where runs merge, a value reaches the last lane of its run through
      seg_scan_add_n's SIX steps (row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31), each one v_fmac with a single rounding of
      a partial sum bounded by the run's sum of |v|: (1 + eps)^6 - 1 <= 6 eps + 15 eps^2, so c_s = 6 + 2 = 8.
      NGM_HASH_ATOMICS_FLOAT: n 2^-40 is replaced by eps n A (n fp32 additions into an accumulator bounded by A).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _permuto_probe as PP  # noqa: E402
from gpu_common import DEV, MARGINS, _test_id  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402

EPS = PP.EPS
F = 2
C_SCAN = 6 + 2        # seg_scan_add_n: six fmac steps (+2: the second-order terms of six compounded roundings), see above
_CACHE = {}


# ------------------------------------------------------------------------------------------------ cases
def _fc(nr_levels=16, log2=12, atomics="exact", matmul="f32"):
    fc = K.field_cfg(encoding="permuto", num_layers=1, nr_levels=nr_levels, log2_hashmap_size=log2, coarsest_scale=1.0,
                     finest_scale=1e-4, scale_mode="no", matmul_mode=matmul)
    fc.hash_grad_atomics = K.HASH_ATOMICS[atomics]
    return fc


def _params(fc, seed=0):
    """distinct shifts and tables per field, table values uniform in [0.5, 1); the linear layers zero"""
    key = ("params", fc.nr_levels, fc.log2_hashmap_size, seed)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 + seed)
        p = {n: torch.zeros(F, *s) for n, s in K.param_shapes(fc).items()}
        p["_encoding.lattice_values"] = 0.5 + 0.5 * torch.rand(F, *K.param_shapes(fc)["_encoding.lattice_values"], generator=g)
        p["_encoding.lattice_values"].clamp_(max=float(np.nextafter(np.float32(1.0), np.float32(0.0))))
        p["_encoding.random_shift_per_level"] = torch.stack([PP.shifts(fc.nr_levels, 50 + 7 * f + seed) for f in range(F)])
        _CACHE[key] = p
    return _CACHE[key]


def _points(name, fc, params):
    """(F,P,3) float32 field-frame points of a named case, built per field on that field's shifts, and whether runs can merge"""
    key = ("points", name, fc.nr_levels, fc.log2_hashmap_size)
    if key in _CACHE:
        return _CACHE[key]
    fs, T = PP.spec(fc.nr_levels, fc.log2_hashmap_size), 1 << fc.log2_hashmap_size
    sh = params["_encoding.random_shift_per_level"]
    kind, _, arg = name.partition(":")
    xs = []
    for f in range(F):
        s = 100 * f + 1
        if kind == "uniform":
            xs.append(PP.uniform(int(arg), sh[f], fs, T, seed=s))
        elif kind == "ties":
            xs.append(PP.ties(sh[f], fs, seed=s))
        elif kind == "runs":
            xs.append(PP.runs(PP.run_lengths(1024), seed=s))
        elif kind == "one_run":
            xs.append(PP.runs([1024], seed=s))
        elif kind == "heads":
            xs.append(PP.heads(int(arg), 16, sh[f], fs, T, seed=s))
        elif kind == "alternating":
            xs.append(PP.alternating(int(arg), sh[f], fs, T, seed=s))
        elif kind == "ray_like":
            xs.append(PP.ray_like(int(arg), 64, seed=s))
        elif kind == "mixed":                                     # rays, then points without runs: 1025 points, one chunk
            xs.append(torch.cat([PP.ray_like(8, 64, seed=s), PP.uniform(513, sh[f], fs, T, seed=s)]))
        else:
            raise KeyError(name)
    n = min(x.shape[0] for x in xs)                               # (the tie set's size depends on the shifts by a few points)
    x = torch.stack([x[:n] for x in xs]).contiguous()
    assert x.dtype == torch.float32
    merges = kind not in ("uniform", "alternating")
    _CACHE[key] = (x, merges)
    return _CACHE[key]


def _reference(name, fc, params, x):
    key = ("ref", name, fc.nr_levels, fc.log2_hashmap_size)
    if key not in _CACHE:
        fs, T = PP.spec(fc.nr_levels, fc.log2_hashmap_size), 1 << fc.log2_hashmap_size
        _CACHE[key] = [PP.simplex32(x[f], params["_encoding.random_shift_per_level"][f], fs, T) for f in range(F)]
    return _CACHE[key]


def _d_enc(P, D, seed=0):
    return torch.randn(F, P, D, generator=torch.Generator().manual_seed(77 + seed))


def _record(name, ratio, tol=1.0):
    MARGINS.append(dict(test=_test_id(), name=name, err=float(ratio), tol=tol))


def _held(err, bar, what):
    """err <= bar elementwise (bar == 0: exactly equal); records and prints the worst err / bar"""
    ratio = float(np.max(np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: worst err / bar = {ratio:.3e}, max err = {float(err.max()):.3e}")
    _record("permuto_exact " + what + " err/bar", ratio)
    assert ratio <= 1.0, (what, ratio, float(err.max()))
    return ratio


# ------------------------------------------------------------------------------------------------ forward
def _forward_bar(ref, table, f):
    idx, w = ref[f]
    E, M = PP.expected_encoding(idx, w, table[f].double().numpy())
    return E, 16 * EPS * np.repeat(M, 2, axis=1)                  # 16 eps M (derivation: module docstring)


FORWARD_CASES = ["uniform:1", "uniform:63", "uniform:64", "uniform:65", "uniform:513", "ties"]


@pytest.mark.parametrize("name", FORWARD_CASES)
def test_encode_forward_vs_fp32_restatement(name):
    fc = _fc()
    params = _params(fc)
    x, _ = _points(name, fc, params)
    ref = _reference(name, fc, params, x)
    out = ops.encode(fc, {k: v.to(DEV) for k, v in params.items()}, x.to(DEV)).cpu().double().numpy()
    for f in range(F):
        E, bar = _forward_bar(ref, params["_encoding.lattice_values"], f)
        _held(np.abs(out[f] - E), bar, f"encode fwd {name} field {f}")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_encode_forward_16bit_table_storage_vs_fp32_restatement(dt):
    """the tie set once more with the table stored in 16 bits: the kernel widens a stored value exactly, so the expectation is
    the same sum over the ROUNDED table, at the same bar"""
    fc = _fc()
    params = _params(fc)
    x, _ = _points("ties", fc, params)
    ref = _reference("ties", fc, params, x)
    lp = {k: (v if k in K.NO_GRAD_PARAMS else v.to(dt)) for k, v in params.items()}
    out = ops.encode(fc, {k: v.to(DEV) for k, v in lp.items()}, x.to(DEV)).cpu().double().numpy()
    rounded = lp["_encoding.lattice_values"].float()
    assert not torch.equal(rounded, params["_encoding.lattice_values"])
    for f in range(F):
        E, bar = _forward_bar(ref, rounded, f)
        _held(np.abs(out[f] - E), bar, f"encode fwd {dt} table ties field {f}")


def _pass_through(params, j):
    """W0 = I, b0 = 0 (ReLU is the identity: every feature is >= 0.5 sum w > 0); output row c = one-hot on feature 4 j + c"""
    p = dict(params)
    p["_linears.0.weight"] = torch.eye(32).repeat(F, 1, 1)
    w1 = torch.zeros(F, 4, 32)
    for c in range(4):
        w1[:, c, 4 * j + c] = 1.0
    p["_linears.1.weight"] = w1
    return p


@pytest.mark.parametrize("mm", ["f32", "auto"])
@pytest.mark.parametrize("name", ["uniform:513", "ties"])
def test_fused_forward_encode_hash_vs_fp32_restatement(name, mm):
    fc = _fc(matmul=mm)
    params = _params(fc)
    x, _ = _points(name, fc, params)
    ref = _reference(name, fc, params, x)
    xd = x.to(DEV)
    outs = []
    with torch.no_grad():
        for j in range(8):
            outs.append(ops.field_eval(fc, {k: v.to(DEV) for k, v in _pass_through(params, j).items()}, xd).cpu())
            assert K.lib().ngm_debug_last_matmul(1) == K.MATMUL["f32"]       # points surface: fp32 MFMA under both settings
    out = torch.cat(outs, -1).double().numpy()                              # (F,P,32): feature 4 j + c from evaluation j
    for f in range(F):
        E, bar = _forward_bar(ref, params["_encoding.lattice_values"], f)
        # + 4 eps |E_ref|: two matrix passes, one non-zero product each
        _held(np.abs(out[f] - E), bar + 4 * EPS * np.abs(E), f"field_eval fwd {mm} {name} field {f}")


# ------------------------------------------------------------------------------------------------ table gradient
def _grad_bar(G_ref, A, n, merges, flt):
    n = n[..., None].astype(np.float64)
    c_s = C_SCAN if merges else 0
    acc = EPS * n * A if flt else n * 2.0 ** -40
    return EPS * (4 + c_s) * A + acc + EPS * np.abs(G_ref)


def _check_table_grad(G, ref, d_enc, T, merges, flt, what):
    """G (F,L,T,2) from the kernel against the expectation of every field; -> worst ratio, max |G - G_ref|, max |G_ref|"""
    G = G.detach().cpu().double().numpy()
    worst, emax, gmax = 0.0, 0.0, 0.0
    for f in range(F):
        idx, w = ref[f]
        G_ref, A, n = PP.expected_table_grad(idx, w, d_enc[f].numpy(), T)
        # the contract of to_fix and of the Q23.40 accumulator: products (|d w| <= |d|) below 2^22, sums below 2^23
        assert float(np.abs(d_enc[f].numpy()).max()) < 2.0 ** 22
        assert float(np.abs(G_ref).max()) < 2.0 ** 23 * 0.99
        err = np.abs(G[f] - G_ref)
        assert (G[f][n == 0] == 0.0).all(), what                            # entries no term reaches: exactly zero
        worst = max(worst, _held(err, _grad_bar(G_ref, A, n, merges, flt), f"{what} field {f}"))
        emax, gmax = max(emax, float(err.max())), max(gmax, float(np.abs(G_ref).max()))
    return worst, emax, gmax


def _run_encode_bwd(fc, params, x, d_enc):
    got = ops.encode_bwd(fc, {k: v.to(DEV) for k, v in params.items()}, x.to(DEV), d_enc.to(DEV))
    return got["_encoding.lattice_values"]


def _table_grad_case(name, atomics="exact", nr_levels=16, log2=12, scale=1.0):
    fc = _fc(nr_levels=nr_levels, log2=log2, atomics=atomics)
    params = _params(fc)
    x, merges = _points(name, fc, params)
    ref = _reference(name, fc, params, x)
    d_enc = (_d_enc(x.shape[1], fc.dim_enc) * scale).float()
    G = _run_encode_bwd(fc, params, x, d_enc)
    what = f"encode_bwd {atomics} L={nr_levels} T=2^{log2} {name}" + (f" x{scale:g}" if scale != 1.0 else "")
    return _check_table_grad(G, ref, d_enc, 1 << log2, merges, atomics == "float", what), (fc, params, x, d_enc, G)


GRAD_CASES = (["uniform:%d" % p for p in (1, 64, 511, 512, 513, 4096)]            # one chunk: k_hash_grad writes the table
              + ["uniform:4097", "uniform:9000"]                                   # several chunks: through k_hash_reduce
              + ["runs", "one_run"] + ["heads:%d" % h for h in (1, 39, 40, 41, 64)]
              + ["alternating:2048", "ray_like:32", "ties"])


@pytest.mark.parametrize("name", GRAD_CASES)
def test_table_gradient_vs_fp32_restatement(name):
    _table_grad_case(name)


@pytest.mark.parametrize("name", ["runs", "uniform:9000"])
def test_table_gradient_float_atomics_vs_fp32_restatement(name):
    _table_grad_case(name, atomics="float")


@pytest.mark.parametrize("nr_levels", [1, 5, 16])
def test_table_gradient_level_counts(nr_levels):
    """5: the odd-level block decode of k_hash_grad; 1: a single level and a two-feature d_enc"""
    _table_grad_case("mixed", nr_levels=nr_levels)


@pytest.mark.parametrize("log2", [4, 8, 13])
def test_table_gradient_table_sizes(log2):
    """T = 16: every entry collides; 2^13: the largest table the exact accumulator fits in LDS"""
    _table_grad_case("mixed", log2=log2)


def test_table_gradient_table_size_14_is_refused_cleanly_or_runs_on_float_atomics():
    """2^14 entries: the Q23.40 accumulators of one level (256 KB) do not fit the LDS.  The entry point refuses with
    NGM_E_UNSUPPORTED before it launches anything (ngm_hash_grad_takes); fp32 accumulators (128 KB) fit and meet the bar."""
    fc = _fc(log2=14)
    params = _params(fc)
    x, _ = _points("mixed", fc, params)
    with pytest.raises(K.NgmError) as e:
        _run_encode_bwd(fc, params, x, _d_enc(x.shape[1], fc.dim_enc))
    assert e.value.code == K.NGM_E_UNSUPPORTED and "table size" in str(e.value)
    torch.cuda.synchronize()
    # every backward is planned before it launches: the point evaluation's refuses as well
    p = {k: v.to(DEV) for k, v in _pass_through(params, 0).items()}
    with pytest.raises(K.NgmError) as e:
        torch.ops.ngm355.field_eval_bwd(ops.cfg_blob(fc), x.to(DEV), None, None, torch.ones(F, x.shape[1], 4, device=DEV),
                                        [p[n] for n in K.param_names(fc)])
    assert e.value.code == K.NGM_E_UNSUPPORTED and "hash table too large" in str(e.value)
    torch.cuda.synchronize()
    _table_grad_case("mixed", atomics="float", log2=14)


@pytest.mark.parametrize("k", [-30, -20, 0, 16])
def test_table_gradient_scale(k):
    """d_enc 2^k on uniform(4096): the same bar at every scale.  At k = -30 the products are ~2^-32 and the n 2^-40 of the
    fixed-point truncation dominates the bar; at k = +16 the products (< 2^16 |d| < 2^22) stay inside to_fix's contract.
    Records what fixed point costs relative to the gradient's own size."""
    (worst, emax, gmax), _ = _table_grad_case("uniform:4096", scale=2.0 ** k)
    print(f"gradient scale 2^{k}: max|G - G_ref| / max|G_ref| = {emax / gmax:.3e}")
    _record(f"permuto_exact gradient scale 2^{k}: max|G-G_ref|/max|G_ref|", emax / gmax, tol=float("nan"))


def test_table_gradient_exact_mode_is_order_independent():
    """exact atomics, one chunk: the integer sums do not depend on the order of the points, nor on the run"""
    (_, _, _), (fc, params, x, d_enc, G) = _table_grad_case("uniform:4096")
    fs = PP.spec()
    sh = params["_encoding.random_shift_per_level"]
    perms = [PP.permutation_without_runs(x[f], sh[f], fs, 4096, seed=5 + f) for f in range(F)]
    xp = torch.stack([x[f][perms[f]] for f in range(F)]).contiguous()
    dp = torch.stack([d_enc[f][perms[f]] for f in range(F)]).contiguous()
    assert torch.equal(_run_encode_bwd(fc, params, xp, dp), G)
    (_, _, _), (fc, params, x, d_enc, G1) = _table_grad_case("runs")
    assert torch.equal(_run_encode_bwd(fc, params, x, d_enc), G1)


@pytest.mark.parametrize("mm", ["f32", "auto"])
@pytest.mark.parametrize("name", ["uniform:513", "ray_like:8"])
def test_table_gradient_through_autograd(name, mm):
    """ops.field_eval(...).backward() with the pass-through network: dL/dE is d_out in the four selected columns (exact
    through W1^T and W0^T = I: one non-zero product per sum) and zero elsewhere, the table gradient is k_hash_grad's behind
    the MLP backward the plan promises (variant 1, k_field_bwd16, for this network under both settings)."""
    fc = _fc(matmul=mm)
    params = _params(fc)
    x, merges = _points(name, fc, params)
    ref = _reference(name, fc, params, x)
    P = x.shape[1]
    d_out = torch.randn(F, P, 4, generator=torch.Generator().manual_seed(31))
    for j in range(8):
        p = {k: v.to(DEV) for k, v in _pass_through(params, j).items()}
        p["_encoding.lattice_values"].requires_grad_()
        out = ops.field_eval(fc, p, x.to(DEV))
        (out * d_out.to(DEV)).sum().backward()
        assert K.lib().ngm_debug_last_bwd_variant() == 1
        d_enc = torch.zeros(F, P, 32)
        d_enc[..., 4 * j:4 * j + 4] = d_out
        _check_table_grad(p["_encoding.lattice_values"].grad, ref, d_enc, 4096, merges, False, f"autograd {mm} {name} columns {4 * j}..")
