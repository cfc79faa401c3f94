"""Inputs of the quadrature tests and their fp64 reference -- host only (torch on the CPU + the oracle), shared by
test_quadrature_cases_cpu.py (the conditions the inputs must meet) and test_gpu_quadrature_exact.py (the kernels).

Why the recipes exist: with `geoms = 0.1 * randn` and geometry_factor 20 every sample's occupancy is near 0.5, a ray is opaque
after a few dozen samples, and at the suite's bars nothing a kernel does past its first 64-sample wave step can be seen (the
CPU test pins the figure).  `thin_inputs` spreads the reference weight along the whole ray instead:

  * per ray an optical-depth budget b in [1, 3]: the termination probability is 1 - exp(-b), 0.63 .. 0.95;
  * that weight is split over the ray's 64-sample wave steps in proportions 0.75 .. 1.25 and, inside a step, over its
    samples in proportions 0.4 .. 1.2, so that EVERY wave step carries weight (the last step of S = 65 holds one sample, that
    of S = 1000 forty: a split per sample alone leaves them under any bar).  A sample's occupancy is w_k / T_k, about b / S
    near the camera and growing along the ray, capped at 0.5;
  * the mode's occupancy function is inverted in fp64: occupancy logit(o) / gf; nrgbd +-logit((1 + sqrt(1 - o)) / 2) / gf with
    a random sign; density -log1p(-o) / delta over the samples that are not negated (the relu is off on
    the others); neus u_{k+1} = u_k - o_k (u_k + 1e-5) from u_0 = 0.3 with u rising instead on the other samples (the clamp
    at zero is active there), g = logit(u) / (isd gf), isd in [0.5, 1.5]; both with at most 46 live samples per ray
    (_live_samples says why): two to sixteen per wave step, occupancy exactly 0 on the others.  (A random walk `0.05 * randn.cumsum` saturates
    the sigmoid from a few dozen samples on: 40 % of the rays at S = 63 and 98 % at S = 1024 then hold a pair of neighbours
    within 1e-4 of the clamp's kink, where no gradient comparison is meaningful.)
  * stratified distances: bin k of [0.5, 3.5] plus jitter inside the middle 80 % of the bin, so deltas are bounded below;
  * ray 0 carries the exact-zero probes geoms[0, 0] = geoms[0, 3] = 0 (occupancy exactly 1 in nrgbd: the ray is opaque, which
    is why the conditions exempt it).
All values are rounded to fp32 before anything is computed from them: kernel and reference read the same numbers."""
import math

import torch

from oracle import ngm_oracle as O

GF = 20.0
POINTWISE = ("nrgbd", "occupancy")
OUT_NAMES = ("C", "D", "Cv", "Dv", "term", "W")
MODES = ("nrgbd", "occupancy", "density", "neus")

# ---- the shapes of test_gpu_quadrature_exact.py (the CPU test checks the conditions at every one of them)
WHOLE_S = (64, 128, 192, 256, 320, 384, 448, 512)          # whole-ray forward and backward, NST = 1..8; 256 = one gather chunk
WHOLE_BIG_S = (576, 1024)                                   # whole-ray forward, generic backward
MULTI_WHOLE = ((6151, 64), (6151, 256), (12301, 64))        # 2 and 3 rays per wave (one ray per wave up to 6144 rays)
GENERIC_S = {m: (((1,) if m in POINTWISE else ()) + (2, 63, 65, 200, 255) + (() if m in POINTWISE else (256,)) +
                 (257, 577, 1000, 1023) + (() if m in POINTWISE else (1024,))) for m in MODES}
FULL_N, FULL_S = 200000, (1, 2, 7, 24)                      # 33 rays per wave: a batch of 32 rays, then a batch of one
MULTI_GENERIC = ((6151, 200), (6151, 300))
PACKED_S = (64, 320, 1024, 100, 300)
ALL_MODE_S = sorted({(m, s) for m in POINTWISE for s in WHOLE_S + WHOLE_BIG_S + PACKED_S} | {("density", 100)} |
                    {(m, s) for m in MODES for s in GENERIC_S[m] + FULL_S + (200, 300) if s > (0 if m in POINTWISE else 1)})


def s_eff(mode, S):
    return S - 1 if mode in ("density", "neus") else S


def _stratified(N, S, gen):
    width = 3.0 / S
    k = torch.arange(S, dtype=torch.float64)
    return 0.5 + (k + 0.1 + 0.8 * torch.rand(N, S, generator=gen, dtype=torch.float64)) * width


def _target_occupancy(N, Se, gen, live=None, budget=(1.0, 3.0)):
    """(N, Se) occupancies whose weights o_k T_k follow the split described above; `live` (N, Se) bool: samples that may carry
    weight (the others get none and do not attenuate)"""
    if live is None:
        live = torch.ones(N, Se, dtype=torch.bool)
    nst = (Se + 63) // 64
    b = budget[0] + (budget[1] - budget[0]) * torch.rand(N, generator=gen, dtype=torch.float64)
    term = 1.0 - torch.exp(-b)
    ps = 0.75 + 0.5 * torch.rand(N, nst, generator=gen, dtype=torch.float64)
    pk = (0.4 + 0.8 * torch.rand(N, Se, generator=gen, dtype=torch.float64)) * live
    step = torch.arange(Se) // 64
    has = torch.zeros(N, nst, dtype=torch.float64).index_add_(1, step, live.double()) > 0
    ps = ps * has
    w_step = term[:, None] * ps / ps.sum(-1, keepdim=True)
    in_step = torch.zeros(N, nst, dtype=torch.float64).index_add_(1, step, pk).clamp_min(1e-300)
    w = w_step[:, step] * pk / in_step[:, step]                     # planned weight of every sample
    occ = torch.zeros(N, Se, dtype=torch.float64)
    T = torch.ones(N, dtype=torch.float64)
    for k in range(Se):                                              # the cap feeds back into T: sequential
        o = torch.minimum(w[:, k] / T, torch.full_like(T, 0.5))
        occ[:, k] = o
        T = T * (1.0 - o)
    return occ


def _live_samples(N, Se, gen, most=32):
    """(N, Se) bool: the samples of a density / neus ray that carry weight.  Both modes form the occupancy as a difference of
    two numbers near each other (1 - exp(-x); (u_k - u_k+1) / u_k), whose fp32 rounding is 6e-8 ABSOLUTE whatever the
    occupancy: at an occupancy of 1e-3 -- a thin ray of 1024 live samples -- the weight itself is good to 3e-5 in ANY fp32
    evaluation, the torch restatement included, which is three times the bar d_colors is held to.  So `most` live samples
    (occupancy >= 0.01: rounding <= 6e-6) are shared evenly among a ray's wave steps, at least two per step -- its first and
    its last sample (that is where a carry enters and leaves) --, and sixteen in the last step, whose
    weights are the ray's smallest anyway (the rounding scales with the transmittance); on the others the relu is off / the
    clamp active: 32 live samples per ray at one or two wave steps, 40 at four or five, 46 at sixteen (2 x 15 + 16).  Short
    rays have a fifth of their samples off, as at S = 24: 4 of 23.  The scans INSIDE a wave step therefore multiply mostly by
    one in these two modes on long rays; what they show there is the carry, the next-sample reads and the clamp / relu
    switches, while the scan itself is covered densely by the pointwise modes, which run the same kernels."""
    nst = (Se + 63) // 64
    live = torch.zeros(N, Se, dtype=torch.bool)
    for j in range(nst):
        lo, hi = 64 * j, min(64 * j + 64, Se)
        n = hi - lo
        want = min(n - n // 5, max(2, most // nst, 16 if j == nst - 1 else 0))
        score = torch.rand(N, n, generator=gen)
        score[:, 0] = 2.0
        score[:, -1] = 3.0                                           # (n = 1: the one sample)
        rank = score.argsort(-1, descending=True).argsort(-1)
        live[:, lo:hi] = rank < want
    return live


def thin_inputs(mode, N, S, seed, probes=True):
    """-> dict(colors (N,S,3), geoms (N,S), dists (N,S), depths (N,S), isds (N,1) | None), fp32"""
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * S + len(mode))
    Se = s_eff(mode, S)
    colors = torch.rand(N, S, 3, generator=gen, dtype=torch.float64).float()
    dists = _stratified(N, S, gen).float()
    depths = dists * 0.9
    isds = None
    geoms = torch.zeros(N, S, dtype=torch.float64)
    if mode in POINTWISE:
        occ = _target_occupancy(N, Se, gen)
        if mode == "occupancy":
            geoms = torch.logit(occ) / GF
        else:
            sign = torch.where(torch.rand(N, S, generator=gen) < 0.5, -1.0, 1.0).double()
            geoms = sign * torch.logit((1.0 + torch.sqrt(1.0 - occ)) / 2.0) / GF
    elif Se > 0:
        live = _live_samples(N, Se, gen)
        # d occ / d g does not grow with the occupancy here as the pointwise modes' does, so the gradient falls with the
        # transmittance itself: a budget of 0.6 .. 1.2 (term 0.45 .. 0.7) keeps the ray's end in sight
        occ = _target_occupancy(N, Se, gen, live, (0.6, 1.2))
        mag = 0.5 + torch.rand(N, Se, generator=gen, dtype=torch.float64)
        if mode == "density":
            delta = (dists[:, 1:] - dists[:, :-1]).double()
            g = -torch.log1p(-occ) / delta
            off = -mag * (1.0 / Se) / delta
            geoms[:, :Se] = torch.where(live, g, off)
            geoms[:, Se] = mag[:, 0] / 3.0                          # the dropped last sample: any value
        else:
            # u falls by its occupancy on a live sample and rises by 0.3 .. 0.9 / Se on the others (at least three times the band
            # of neus_kink_rays; e^0.9 over a whole ray, so u stays inside 0.015 .. 0.75 and the sigmoid is never saturated)
            isds = (0.5 + torch.rand(N, 1, generator=gen, dtype=torch.float64)).float()
            u = torch.empty(N, S, dtype=torch.float64)
            u[:, 0] = 0.3
            for k in range(Se):
                down = u[:, k] - occ[:, k] * (u[:, k] + 1e-5)
                u[:, k + 1] = torch.where(live[:, k], down, u[:, k] * (1.0 + 0.6 * mag[:, k] / Se))
            geoms = torch.logit(u) / (isds.double() * GF)
    else:
        isds = (0.5 + torch.rand(N, 1, generator=gen, dtype=torch.float64)).float() if mode == "neus" else None
        geoms = torch.rand(N, S, generator=gen, dtype=torch.float64)
    geoms = geoms.float()
    if probes and mode != "neus":
        geoms[0, 0] = 0.0                                            # occ == 1 exactly (nrgbd): the recursion must be exact
        if S > 3:
            geoms[0, 3] = 0.0
    return dict(colors=colors, geoms=geoms, dists=dists, depths=depths, isds=isds)


def opaque_inputs(mode, N, S, seed):
    """the suite's earlier recipe (test_quadrature_backward_vs_oracle and its neighbour-mode sibling): sharp transmittance"""
    gen = torch.Generator().manual_seed(99991 * seed + S + len(mode))
    colors = torch.rand(N, S, 3, generator=gen)
    if mode in POINTWISE:
        geoms = 0.1 * torch.randn(N, S, generator=gen)
    elif mode == "density":
        geoms = torch.randn(N, S, generator=gen)
    else:
        geoms = 0.05 * torch.randn(N, S, generator=gen).cumsum(-1).flip(-1)
    dists = torch.sort(torch.rand(N, S, generator=gen) * 3 + 0.5, -1)[0]
    isds = (0.5 + torch.rand(N, 1, generator=gen)) if mode == "neus" else None
    return dict(colors=colors, geoms=geoms, dists=dists, depths=dists * 0.9, isds=isds)


def mixed_thin_rays(mode, N):
    """(N,) bool: the rays of `mixed_inputs` that come from `thin_inputs` -- every other ray; in neus three of four: its
    earlier recipe (a random walk through the sigmoid) puts a pair of neighbours within 1e-4 of the clamp's kink on 12 % of
    its rays at S = 24, and at most 5 % of a case's rays may be left out of the gradient comparison for that"""
    return torch.arange(N) % (4 if mode == "neus" else 2) != 0


def mixed_inputs(mode, N, S, seed):
    """opaque-ish and thin rays interleaved: sharp and flat transmittance both cross ray boundaries inside a wave step"""
    a, b = opaque_inputs(mode, N, S, seed), thin_inputs(mode, N, S, seed, probes=False)
    thin = mixed_thin_rays(mode, N)
    out = {}
    for k in a:
        if a[k] is None:
            out[k] = None
            continue
        out[k] = torch.where(thin.view(-1, *([1] * (a[k].dim() - 1))), b[k], a[k])
    return out


def cotangents(N, seed):
    gen = torch.Generator().manual_seed(31 * seed + 5)
    return dict(dC=torch.randn(N, 3, generator=gen), dD=torch.randn(N, generator=gen), dT=torch.randn(N, generator=gen))


def reference(mode, inp, cot=None, dtype=torch.float64, gf=GF):
    """`oracle.ngm_oracle.quadrature` in `dtype` on the (fp32) inputs: the six outputs and, with cotangents, autograd's
    d_colors / d_geoms / d_isds.  dtype = float64 is the reference; float32 is the torch restatement whose own error against
    the reference sets the bars."""
    leaf = lambda x: x.detach().to(dtype, copy=True).requires_grad_(cot is not None)       # (copy: never the caller's tensor)
    c, g = leaf(inp["colors"]), leaf(inp["geoms"])
    i = None if inp.get("isds") is None else leaf(inp["isds"])
    outs = O.quadrature(mode, c, g, inp["dists"].to(dtype), inp["depths"].to(dtype), gf, i)
    res = {n: o.detach() for n, o in zip(OUT_NAMES, outs)}
    if cot is not None:
        C, D, _, _, T, _ = outs
        ((C * cot["dC"].to(dtype)).sum() + (D * cot["dD"].to(dtype)).sum() + (T * cot["dT"].to(dtype)).sum()).backward()
        res["d_colors"], res["d_geoms"] = c.grad, g.grad
        if i is not None:
            res["d_isds"] = i.grad
    return res


def step_shares(W):
    """(N, S_w) weights -> (N, ceil(S_w / 64)): each 64-sample wave step's share of its ray's total weight"""
    N, Sw = W.shape
    nst = (Sw + 63) // 64
    Wp = torch.zeros(N, nst * 64, dtype=W.dtype)
    Wp[:, :Sw] = W
    return Wp.view(N, nst, 64).sum(-1) / W.sum(-1, keepdim=True)


def neus_kink_rays(inp, gf=GF, band=1e-4):
    """(N,) bool: rays with a pair of neighbours whose |u_k - u_{k+1}| / (u_k + 1e-5) is below `band` in fp64: the clamp's side,
    and with it the whole gradient of the pair, is undecided between two fp32 evaluations"""
    u = torch.sigmoid(inp["isds"].double() * gf * inp["geoms"].double())
    if u.shape[-1] < 2:
        return torch.zeros(u.shape[0], dtype=torch.bool)
    return ((u[:, :-1] - u[:, 1:]).abs() / (u[:, :-1] + 1e-5) < band).any(-1)


# ---- the fused image call (pair records): a map whose medium is thin
PAIR_FIELD = dict(encoding="fourier", dim_enc=64, num_layers=2)
PAIR_CASES = ((1, 64, 3000, 1024), (2, 384, 3000, 1024), (4, 640, 3000, 1024), (5, 192, 3000, 1024), (8, 256, 3000, 1024),
              (2, 384, 13000, 13000))                       # (K, S, rays, ray block); 13000 rays in one block: 3 rays per wave


def pair_scene(mode, S, N, seed=0):
    """Fifty unit-radius fields on a 5 x 5 x 2 grid (z = -2, -1.5), N rays from cameras around (0, 0, 1) looking down -z: a ray
    enters the fields at a distance of ~1.55 and leaves them beyond 4 (rays towards the image corners leave sideways, earlier);
    near is 0 .. 0.1 and far 3.75 .. 3.9, so the first wave step of a ray of 128 samples or more lies outside every field, the
    next is mixed, and the fields reach the last one.  The last layer is set so that the occupancy inside a field is about
    2 / S (an optical depth of ~1.2 over the ray) times e^(+-1) from place to place; outside a field the model's constant
    must be transparent too: 1.0 in nrgbd, -1.0 in occupancy (with 1.0 empty space is opaque there).
    -> dict(pos, quat, params, ijs, c2ws, near, far, outside_value)"""
    fs = O.FieldSpec(**PAIR_FIELD)
    gen = torch.Generator().manual_seed(4243 * seed + S)
    g = torch.arange(-1.0, 1.01, 0.5)
    pos = torch.stack(torch.meshgrid(g, g, torch.tensor([-2.0, -1.5]), indexing="ij"), -1).reshape(-1, 3)
    pos = pos + 1e-3 * torch.randn(pos.shape, generator=gen)
    NF = pos.shape[0]
    quat = torch.nn.functional.normalize(torch.randn(NF, 4, generator=gen), dim=-1)
    params = O.init_params(fs, NF, seed=3, sigma=3.0)
    occ = 2.0 / S
    g0 = math.log(occ / (1.0 - occ)) / GF if mode == "occupancy" else math.log((1 + math.sqrt(1 - occ)) / (1 - math.sqrt(1 - occ))) / GF
    params["_linears.2.weight"][:, 3] *= 0.5
    params["_linears.2.bias"][:, 3] = g0
    params["_linears.2.bias"][:, :3] = 0.2 + 0.6 * torch.rand(NF, 3, generator=gen)
    ijs = torch.stack((torch.randint(0, 480, (N,), generator=gen), torch.randint(0, 640, (N,), generator=gen)), -1)
    c2ws = torch.eye(4).repeat(N, 1, 1)
    c2ws[:, :3, 3] = 0.1 * torch.randn(N, 3, generator=gen)
    c2ws[:, 2, 3] += 1.0
    near, far = 0.1 * torch.rand(N, generator=gen), 3.75 + 0.15 * torch.rand(N, generator=gen)
    return dict(fs=fs, pos=pos, quat=quat, params=params, ijs=ijs, c2ws=c2ws, near=near, far=far,
                outside_value=-1.0 if mode == "occupancy" else 1.0)


def pair_conditions(o4, W, outside_value, chunk_steps):
    """shares of the rays (fp64 reference weights W (N,S), staged outputs o4 (N,S,4)) that meet each condition of the pair-record
    cases: >= 10 % of the weight in one wave step of the second or a later gather chunk; >= 10 % in each of two different steps;
    a step wholly outside every field next to a mixed one -> dict of three fractions"""
    N, S = W.shape
    sh = step_shares(W)
    nst = sh.shape[-1]
    later = sh[:, chunk_steps:].max(-1).values >= 0.1 if nst > chunk_steps else torch.zeros(N, dtype=torch.bool)
    two = (sh >= 0.1).sum(-1) >= 2
    out = (o4[..., 3] == outside_value).view(N, nst, 64)
    allout, mixed = out.all(-1), out.any(-1) & ~out.all(-1)
    return dict(later_chunk=float(later.float().mean()), two_steps=float(two.float().mean()),
                outside_and_mixed=float((allout.any(-1) & mixed.any(-1)).float().mean()), mixed=float(mixed.any(-1).float().mean()))
