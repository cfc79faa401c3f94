"""The sparse per-field Adam update, once, in float64, with an elementwise bound on what an fp32 evaluation of it may
differ by -- the one reference the library's six hand copies of the update are held to (tests/test_gpu_adam.py), and the
fp32 restatement + its mutants that show the bar can fail (tests/test_adam_host_cpu.py).  numpy only.

The update is torch.optim.Adam with L2-coupled weight decay (the gradient becomes g + wd p BEFORE the moments), one step
counter shared by all rows, `step` = the NEW count (1 for the first update):

    gg = g + wd p          m' = b1 m + (1 - b1) gg          v' = b2 v + (1 - b2) gg^2
    D  = sqrt(v') / sqrt(1 - b2^step) + eps                 u  = lr / (1 - b1^step) m' / D          p' = p - u

The bound is first-order error propagation through that formula with e = 2^-24 (half an ulp, relative) per fp32
operation, A = |g| + |wd p|:

    dgg = 2e A
    dm  = (1 - b1) dgg + 2e (b1 |m| + (1 - b1) |gg|)
    dv  = (1 - b2) (2 |gg| dgg + dgg^2) + 3e (b2 v + (1 - b2) gg^2)
    dsq = min(dv / (2 sqrt v'), sqrt dv) + e sqrt v'            (the first term only where v' > 0)
    dD  = dsq / sqrt(1 - b2^step) + 3e D
    du  = lr / (1 - b1^step) (dm / D + |m'| dD / D^2) + 4e |u|
    dp  = du + e |p'|

plus an absolute floor of the smallest normal fp32 on dm and dv and of that floor times lr on dp: NO CLAIM IS MADE ABOUT
DENORMALS -- a kernel may flush them or keep them, both pass.  A plain fp32 evaluation in the kernels' operation order
(`adam_fp32`) stays within 1x the bound; the GPU kernels are held to BAR = 4x: one factor 2 for fused multiply-add
contraction and a 1-ulp sqrtf, one factor 2 of margin.  The factor is not tuned on the kernels."""
import numpy as np

EPS32 = 2.0 ** -24
TINY32 = float(np.finfo(np.float32).tiny)          # 1.18e-38, smallest normal
BAR = 4.0

# (lr, beta1, beta2, eps, weight_decay): the shipped set, the same without decay, and one far from it
HYPER = {
    "shipped": (1e-3, 0.9, 0.999, 1e-15, 1e-5),
    "no_decay": (1e-3, 0.9, 0.999, 1e-15, 0.0),
    "far": (3e-2, 0.8, 0.99, 1e-8, 1e-2),
}
# the CPU test's five sets: the three above and two that move one thing each (a large eps; heavy decay with a small lr)
HYPER_CPU = dict(HYPER, big_eps=(1e-3, 0.9, 0.999, 1e-4, 1e-5), heavy_decay=(1e-4, 0.9, 0.999, 1e-15, 1e-1))
STEPS = (1, 2, 7, 1000, 100000)


def _f32(x):
    """a scalar hyper-parameter as the C ABI receives it (a float argument), widened back"""
    return float(np.float32(x))


def _np64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    assert x.dtype == np.float32, f"fp32 inputs expected, got {x.dtype}"
    return x.astype(np.float64)


def adam_ref64(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """fp32 arrays (numpy or torch) -> ((p', m', v'), (dp, dm, dv)) in float64; `step` is the new count (>= 1)."""
    p, g, m, v = _np64(p), _np64(g), _np64(m), _np64(v)
    lr, b1, b2, eps, wd = _f32(lr), _f32(beta1), _f32(beta2), _f32(eps), _f32(wd)
    step = int(step)
    assert step >= 1
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    e = EPS32
    gg = g + wd * p
    mn = b1 * m + (1.0 - b1) * gg
    vn = b2 * v + (1.0 - b2) * gg * gg
    sq = np.sqrt(vn)
    D = sq / np.sqrt(bc2) + eps
    u = lr / bc1 * mn / D
    pn = p - u

    A = np.abs(g) + np.abs(wd * p)
    dgg = 2 * e * A
    dm = (1.0 - b1) * dgg + 2 * e * (b1 * np.abs(m) + (1.0 - b1) * np.abs(gg))
    dv = (1.0 - b2) * (2 * np.abs(gg) * dgg + dgg * dgg) + 3 * e * (b2 * v + (1.0 - b2) * gg * gg)
    dm = dm + TINY32
    dv = dv + TINY32
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(vn > 0, dv / (2 * sq), np.inf)
    dsq = np.minimum(lin, np.sqrt(dv)) + e * sq
    dD = dsq / np.sqrt(bc2) + 3 * e * D
    du = lr / bc1 * (dm / D + np.abs(mn) * dD / (D * D)) + 4 * e * np.abs(u)
    dp = du + e * np.abs(pn) + TINY32 * lr
    return (pn, mn, vn), (dp, dm, dv)


def adam_fp32(p, g, m, v, lr, beta1, beta2, eps, wd, step, mutant=None):
    """The update evaluated in plain fp32 numpy in the kernels' operation order (bias corrections in double, rounded once,
    as every site does).  `mutant`: one of MUTANTS -- the same with one deliberate fault, for the CPU test."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=np.float32) for x in (p, g, m, v))
    lr_, b1, b2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
    s = int(step) + (1 if mutant == "step_plus_one" else 0)
    if mutant == "betas_swapped":
        b1, b2 = b2, b1
    lr_bc1 = f(float(lr_) / (1.0 - float(b1) ** s))
    inv_sqrt_bc2 = f(1.0) if mutant == "no_bias_correction2" else f(1.0 / np.sqrt(1.0 - float(b2) ** s))
    one = f(1.0)
    if mutant in ("no_decay", "decoupled_decay"):
        gg = g
    else:
        gg = g + wd * p
    mn = b1 * m + (one - b1) * gg
    vn = b2 * v + (one - b2) * gg * gg
    vd = v if mutant == "old_v" else vn
    if mutant == "eps_in_sqrt":
        den = np.sqrt(vd + eps) * inv_sqrt_bc2
    else:
        den = np.sqrt(vd) * inv_sqrt_bc2 + eps
    with np.errstate(divide="ignore", invalid="ignore"):
        pn = p - lr_bc1 * (mn / den)
    if mutant == "decoupled_decay":                    # AdamW: p (1 - lr wd) instead of the gradient term
        pn = pn - lr_ * wd * p
    assert pn.dtype == mn.dtype == vn.dtype == np.float32
    return pn, mn, vn


MUTANTS = ("step_plus_one", "betas_swapped", "no_decay", "decoupled_decay", "eps_in_sqrt", "no_bias_correction2", "old_v")


def draw_inputs(n, seed, scale=1.0, zero_moments=0.25):
    """n elements mixing |p| in {1e-5, 1e-2, 1}, |g| in {0, 1e-8, 1e-3, 1} * scale, and zero and non-zero moments (a share
    `zero_moments` has m = v = 0; the others hold what an earlier gradient h of the same family of magnitudes would have
    left: |m| = (0.1 .. 1) |h|, v = (0.1 .. 1) h^2).  Every magnitude carries a random factor in [0.5, 1.5) and a random
    sign, so mantissas are generic.  fp32 arrays (p, g, m, v)."""
    r = np.random.default_rng(seed)
    sgn = lambda: r.choice([-1.0, 1.0], n)
    wob = lambda: r.uniform(0.5, 1.5, n)
    p = sgn() * wob() * r.choice([1e-5, 1e-2, 1.0], n)
    g = sgn() * wob() * r.choice([0.0, 1e-8, 1e-3, 1.0], n) * scale
    h = wob() * r.choice([1e-8, 1e-3, 1.0], n) * scale
    m = sgn() * r.uniform(0.1, 1.0, n) * h
    v = r.uniform(0.1, 1.0, n) * h * h
    z = r.random(n) < zero_moments
    m[z], v[z] = 0.0, 0.0
    return tuple(x.astype(np.float32) for x in (p, g, m, v))


def ratios(got, ref, bound):
    """|got - ref| / bound per element, for (p, m, v) triples -> three float64 arrays (non-finite results count as inf)"""
    out = []
    for a, b, d in zip(got, ref, bound):
        a = _np64(a)
        with np.errstate(invalid="ignore"):
            q = np.abs(a - b) / d
        q[~np.isfinite(a)] = np.inf
        out.append(q)
    return out


def summarize(rs):
    """worst ratio and the share of elements above 1x the bound, per output -> dict(p=(worst, share), m=..., v=...)"""
    return {k: (float(q.max()) if q.size else 0.0, float((q > 1.0).mean()) if q.size else 0.0) for k, q in zip("pmv", rs)}
