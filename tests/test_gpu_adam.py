"""Every site of the one sparse per-field Adam update (csrc/ngm_adam.h; k_adam_multi's scalar branch writes the same lines
out) against ONE float64 reference (tests/_adam_host.py), one update at a time, past step one and from non-zero moments, at
4x the reference's fp32 error bound (BAR; tests/test_adam_host_cpu.py shows that seven plausible faults break it).  The six
sites:

    1  k_adam_sparse                      ops.adam_sparse_ (bias corrections on the host)
    2  k_adam_multi, float4 and scalar    ngm_adam_sparse_multi; the renderer's triplane planes and `_neus_sd`
    3  k_grad_reduce<COUNTED>             fused step, more than 8 backward workgroups per field
    4  grad_reduce_one / k_grad_reduce_flat<COUNTED>   8 or fewer; also what rides inside the k_hash_grad launch
    5  k_hash_grad's epilogue             hash tables, one chunk per (field, level)
    6  k_hash_reduce                      hash tables, several chunks

(a) drives sites 1 and 2 with synthetic tensors; (b) teacher-forces sites 2 to 6 through the renderer: every iteration
snapshots the state, takes the gradient of an update=False call, runs the same call with update=True and compares the new
state of the active rows with the reference applied to (snapshot, gradient) -- the next iteration continues from the GPU's
own state, so nothing accumulates, the training step's chaos does not enter and the tolerance stays the single-step bound.
Each fused case asserts which site it reached (launch counters of ngm_profile_read and plan_bwd's rule restated here)
and prints the worst error-to-bound ratios."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from neural_graph_mapping_amd import _capi as K  # noqa: E402

pytestmark = pytest.mark.gpu

if not os.path.exists(K.LIB_PATH):       # a fresh checkout: build on demand (collection must not fail)
    from neural_graph_mapping_amd import build as _build
    _build.build(verbose=False)

from _adam_host import BAR, HYPER, STEPS, adam_ref64, draw_inputs, ratios, summarize  # noqa: E402
from gpu_common import DEV, make_renderer, make_target, synth_target  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402

SCALES = (1.0, 1e-4, 1e3, 1e-2, 1e14)          # of |g| and the moments, one per entry of STEPS; |g| <= 1.5e14 < 1e15
LP = {None: None, "float16": torch.float16, "bfloat16": torch.bfloat16}


def bits(t):
    """the tensor's bit patterns (bitwise comparisons: -0.0 != 0.0, NaN == NaN)"""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a), bits(b)))


class Acc:
    """worst error-to-bound ratio and share of elements above 1x the bound, per output, over many comparisons"""

    def __init__(self):
        self.worst, self.over, self.n = dict(p=0.0, m=0.0, v=0.0), dict(p=0, m=0, v=0), dict(p=0, m=0, v=0)

    def add(self, rs):
        for k, q in zip("pmv", rs):
            if q.size:
                self.worst[k] = max(self.worst[k], float(q.max()))
                self.over[k] += int((q > 1.0).sum())
                self.n[k] += q.size

    def line(self):
        return "  ".join(f"{k}: worst {self.worst[k]:.3f}x, {self.over[k] / max(self.n[k], 1):.2%} above 1x" for k in "pmv")


def check_update(new, old, grad, hp, step, what, acc=None):
    """new / old: (p, m, v) fp32 tensors of the ACTIVE rows after / before the update, grad: their gradient rows"""
    ref, bound = adam_ref64(old[0], grad, old[1], old[2], *hp, step)
    rs = ratios(new, ref, bound)
    if acc is not None:
        acc.add(rs)
    for k, q in zip("pmv", rs):
        worst = float(q.max()) if q.size else 0.0
        assert worst <= BAR, (what, k, f"{worst:.3g}x the bound at element {int(q.argmax())}, step {step}",
                              summarize(rs))
    return rs


# =================================================================================================
# (a) the standalone kernels on synthetic tensors
# =================================================================================================
class Strided:
    """(N, numel) rows `stride` floats apart, starting `offset` floats into their storage -- and the storage, to see that
    nothing between or around the rows moves"""

    def __init__(self, values, N, numel, stride, offset, dtype=torch.float32):
        self.store = torch.zeros(offset + N * stride + 3, dtype=dtype, device=DEV)
        self.store.copy_(torch.arange(self.store.numel(), device=DEV) % 251 + 1)          # recognisable filler in the gaps
        self.view = self.store.as_strided((N, numel), (stride, 1), offset)
        self.view.copy_(values.to(DEV).to(dtype))
        self.before = self.store.clone()

    def untouched_outside(self, rows, what):
        mask = torch.zeros_like(self.store, dtype=torch.bool)
        mask.as_strided(self.view.shape, self.view.stride(), self.view.storage_offset())[rows] = True
        assert bool(torch.equal(bits(self.store)[~mask], bits(self.before)[~mask])), f"{what}: moved outside the active rows"


class Problem:
    """one tensor of a launch: N rows of which the F rows `index` (a permutation, not contiguous) are updated"""

    def __init__(self, N, F, numel, seed, scale, pad=0, offset=0, lp=None, zero=False):
        self.N, self.F, self.numel = N, F, numel
        g = torch.Generator().manual_seed(seed)
        self.index = torch.randperm(N, generator=g)[:F].to(DEV)
        p, gr, m, v = (torch.from_numpy(x).view(N, numel) for x in draw_inputs(N * numel, seed, scale))
        if zero:                                     # g = 0, m = v = 0: with wd = 0 the update is exactly zero
            gr, m, v = torch.zeros_like(gr), torch.zeros_like(m), torch.zeros_like(v)
        stride = numel + pad
        self.p, self.m, self.v = (Strided(x, N, numel, stride, offset) for x in (p, m, v))
        self.g = Strided(gr[:F], F, numel, numel + pad, offset)
        self.lp = None if lp is None else Strided(p, N, numel, stride, 0, dtype=lp)
        self.lp_dtype = lp

    def tensor(self):
        t = K.AdamTensor(self.p.view.data_ptr(), self.m.view.data_ptr(), self.v.view.data_ptr(), self.g.view.data_ptr(),
                         self.p.view.stride(0), self.g.view.stride(0), self.numel)
        if self.lp is not None:
            t.param_lp, t.lp_dtype = self.lp.view.data_ptr(), ops._TORCH_DT[self.lp_dtype]
        return t

    def check(self, hp, step, what, acc=None):
        idx = self.index
        old = tuple(x.before.as_strided(x.view.shape, x.view.stride(), x.view.storage_offset())[idx] for x in (self.p, self.m, self.v))
        new = tuple(x.view[idx] for x in (self.p, self.m, self.v))
        check_update(new, old, self.g.view, hp, step, what, acc)
        for x, n in ((self.p, "param"), (self.m, "exp_avg"), (self.v, "exp_avg_sq")):
            x.untouched_outside(idx, f"{what} {n}")
        assert same_bits(self.g.store, self.g.before), f"{what}: the gradient was written"
        if self.lp is not None:
            assert same_bits(self.lp.view[idx], new[0].to(self.lp_dtype)), f"{what}: 16-bit copy != RNE cast of the new master"
            self.lp.untouched_outside(idx, f"{what} 16-bit copy")
        return old, new


def launch_multi(problems, hp, step, step_dev=None, advance_step=0, advance_offset=None):
    F = problems[0].F
    arr = (K.AdamTensor * len(problems))(*[q.tensor() for q in problems])
    assert all(q.F == F and torch.equal(q.index, problems[0].index) for q in problems)
    K.check(K.lib().ngm_adam_sparse_multi(arr, len(problems), ops._ptr(problems[0].index), F, int(step), ops._ptr(step_dev),
                                          *hp, int(advance_step), ops._ptr(advance_offset), ops._stream()),
            "ngm_adam_sparse_multi")


def shared_index(problems):
    for q in problems[1:]:
        q.index = problems[0].index
    return problems


SITE1_NUMEL = (1, 3, 4, 5, 1023, 1024, 1025, 131072, 64 * 256 + 5)      # the last: the 64-block grid cap, loop runs twice


@pytest.mark.parametrize("hyper", list(HYPER))
def test_site1_adam_sparse(hyper):
    """k_adam_sparse: every size at every step, non-zero moments, a permuted subset of the rows"""
    hp, acc = HYPER[hyper], Acc()
    for si, (step, scale) in enumerate(zip(STEPS, SCALES)):
        for ni, numel in enumerate(SITE1_NUMEL):
            N, F = (3, 2) if numel > 100000 else (7, 4)
            q = Problem(N, F, numel, seed=100 * si + ni, scale=scale)
            ops.adam_sparse_(q.p.view, q.m.view, q.v.view, q.g.view, q.index, step, lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3],
                             weight_decay=hp[4])
            torch.cuda.synchronize()
            q.check(hp, step, f"site 1 numel={numel} step={step}", acc)
    print(f"\nadam site 1 (k_adam_sparse) [{hyper}]  {acc.line()}")


# site 2 layouts: (numel, row pad, base offset in floats).  The launcher's grid is min((numel / 4 + 255) / 256 + 1,
# max(16, ceil(1024 / F))) workgroups of 256 threads: F = 64 -> 16 workgroups, the float4 loop runs twice from 16 Ki floats
# up; F = 1 -> 1024 workgroups, twice from 1 Mi floats up.  A row stride not divisible by 4 and a base one float off
# 16-byte alignment take the scalar path.
SITE2_LAYOUTS = [(n, 0, 0) for n in (1, 3, 4, 5, 1023, 1024, 1025, 131072)] + [(1024, 3, 0), (1024, 0, 1), (131072, 1, 0)]
TWICE = {64: 16 * 256 * 4 + 1024, 1: 1024 * 256 * 4 + 4096}


@pytest.mark.parametrize("lp", [None, "float16", "bfloat16"])
@pytest.mark.parametrize("F", [1, 64])
@pytest.mark.parametrize("hyper", list(HYPER))
def test_site2_adam_multi(hyper, F, lp):
    """k_adam_multi, one tensor per launch: float4 and scalar path, every size, both grid regimes, with / without a 16-bit copy"""
    hp, acc = HYPER[hyper], Acc()
    N = F + 3
    layouts = SITE2_LAYOUTS + [(TWICE[F], 0, 0)]
    for li, (numel, pad, off) in enumerate(layouts):
        si = li % len(STEPS)
        step, scale = STEPS[si], SCALES[si]
        q = Problem(N, F, numel, seed=7000 + 10 * li + F, scale=scale, pad=pad, offset=off, lp=LP[lp])
        launch_multi([q], hp, step)
        torch.cuda.synchronize()
        q.check(hp, step, f"site 2 numel={numel} pad={pad} offset={off} F={F} step={step}", acc)
    print(f"\nadam site 2 (k_adam_multi) [{hyper}, F={F}, lp={lp}]  {acc.line()}")


@pytest.mark.parametrize("hyper", list(HYPER))
def test_site2_every_step_both_paths(hyper):
    """k_adam_multi at every step of STEPS on one aligned (float4) and one unaligned (scalar) tensor"""
    hp, acc = HYPER[hyper], Acc()
    for si, (step, scale) in enumerate(zip(STEPS, SCALES)):
        for pad in (0, 1):
            q = Problem(9, 5, 2048, seed=300 + 2 * si + pad, scale=scale, pad=pad, lp=torch.bfloat16)
            launch_multi([q], hp, step)
            torch.cuda.synchronize()
            q.check(hp, step, f"site 2 step={step} pad={pad}", acc)
    print(f"\nadam site 2 (k_adam_multi) every step [{hyper}]  {acc.line()}")


@pytest.mark.parametrize("lp", [None, "bfloat16"])
def test_site2_several_tensors_one_launch(lp):
    """tensors of different numel and alignment in one launch (the grid is sized for the largest: the workgroups beyond a
    small tensor's end must leave it alone)"""
    hp, acc, step = HYPER["far"], Acc(), 7
    specs = [(5, 0, 0), (131072, 0, 0), (1024, 3, 0), (4, 0, 0), (1025, 0, 0), (4096, 0, 1), (1, 0, 0)]
    qs = shared_index([Problem(12, 8, n, seed=900 + i, scale=1.0, pad=pad, offset=off, lp=LP[lp])
                       for i, (n, pad, off) in enumerate(specs)])
    launch_multi(qs, hp, step)
    torch.cuda.synchronize()
    for q, s in zip(qs, specs):
        q.check(hp, step, f"site 2 multi {s}", acc)
    print(f"\nadam site 2 (k_adam_multi) 7 tensors in one launch [lp={lp}]  {acc.line()}")


@pytest.mark.parametrize("site", [1, 2])
def test_zero_gradient_zero_moments_leave_the_parameter(site):
    """g = 0, m = v = 0, wd = 0: 0 / (0 + eps) -- the parameter keeps its bits and stays finite"""
    hp = HYPER["no_decay"]
    for numel, pad in ((1025, 0), (4096, 0), (4096, 1)):
        q = Problem(6, 4, numel, seed=40 + pad, scale=1.0, pad=pad, zero=True)
        if site == 1:
            ops.adam_sparse_(q.p.view, q.m.view, q.v.view, q.g.view, q.index, 3, lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3],
                             weight_decay=hp[4])
        else:
            launch_multi([q], hp, 3)
        torch.cuda.synchronize()
        assert same_bits(q.p.store, q.p.before), (site, numel, pad)
        assert bool(torch.isfinite(q.p.view).all() and torch.isfinite(q.m.view).all() and torch.isfinite(q.v.view).all())
        q.check(hp, 3, f"site {site} zero gradient")


@pytest.mark.parametrize("mode", ["step", "step_and_offset", "offset_only"])
def test_site2_device_step_advances_once_per_launch(mode):
    """advance_step_dev = 1: the launch reads *step_dev as ITS step and the last workgroup to finish increments it (the
    header: "the kernel does ++*step_dev ... once every block has finished").  Five launches back to back on one stream,
    each on tensors of its own (different grids), nothing in between: launch k = 0..4 is the reference at step s0 + k and
    the counter ends at s0 + 5; advance_philox_offset_dev likewise.  offset_only: the step stays, the offset advances."""
    hp, s0, o0, acc = HYPER["shipped"], 3, 2 ** 40 + 17, Acc()
    step_dev = torch.tensor([s0], dtype=torch.int64, device=DEV)
    off_dev = torch.tensor([o0], dtype=torch.int64, device=DEV)
    shapes = [(4, 3, 1024), (70, 64, 5), (3, 1, 131072), (9, 6, 1025), (5, 2, 16384)]
    qs = [Problem(N, F, numel, seed=60 + k, scale=1.0) for k, (N, F, numel) in enumerate(shapes)]
    for q in qs:
        launch_multi([q], hp, 999, step_dev=step_dev, advance_step=int(mode != "offset_only"),
                     advance_offset=None if mode == "step" else off_dev)
    torch.cuda.synchronize()
    for k, q in enumerate(qs):
        q.check(hp, s0 + (0 if mode == "offset_only" else k), f"site 2 advance launch {k}", acc)
    assert int(step_dev) == (s0 if mode == "offset_only" else s0 + 5)
    assert int(off_dev) == (o0 if mode == "step" else o0 + 5)
    print(f"\nadam site 2 (k_adam_multi) device step, 5 launches [{mode}]  {acc.line()}")


# =================================================================================================
# (b) the fused sites, teacher-forced through the renderer
# =================================================================================================
M1 = dict(encoding="fourier", dim_enc=64, num_layers=2)
HASH = dict(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
EXACT = dict(hash_grad_atomics="exact")
N_ITER = 6


def plan_bwd(F, P, unit):
    """ngm_api.hip plan_bwd restated: backward workgroups per field for F launched rows of P samples each; `unit` = samples a
    workgroup's range is a multiple of (128; the hash network's 8-wave backward: 256)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    b = (ncu + F - 1) // F
    per = max(((P + b - 1) // b + unit - 1) // unit * unit, unit)
    return (P + per - 1) // per


def hash_chunks(F, P, levels=16):
    """ngm_launch_hash_grad's rule restated: sample chunks per (field, level)"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    units = F * levels
    return max(1, min((2 * ncu + units - 1) // units, (P + 4095) // 4096, 8))


def launches():
    out = {}
    n = C.c_int64()
    for k in ("grad_reduce", "adam", "hash_grad", "hash_reduce"):
        K.check(K.lib().ngm_profile_read(K.KERNEL_IDS[k], None, C.byref(n)), "ngm_profile_read")
        out[k] = int(n.value)
    return out


def active_sets(NF, F, n_iter, seed):
    """n_iter selections of F of the NF fields, each in a random order: the first one or two fields are trained in the
    first iteration, left out of the next two and trained again in the last; the others come and go at random"""
    g = torch.Generator().manual_seed(seed)
    must = list(range(min(2, NF - F, F)))
    others = [i for i in range(NF) if i not in must]
    sets = []
    for it in range(n_iter):
        if it in (0, n_iter - 1):
            sel = must + [others[j] for j in torch.randperm(len(others), generator=g).tolist()[:F - len(must)]]
        elif it in (1, 2):
            sel = [others[j] for j in torch.randperm(len(others), generator=g).tolist()[:F]]
        else:
            sel = torch.randperm(NF, generator=g).tolist()[:F]
        sel = [sel[j] for j in torch.randperm(F, generator=g).tolist()]
        assert len(set(sel)) == F
        sets.append(torch.tensor(sel, dtype=torch.int64))
    return sets


class Scene:
    """NF posed fields with rays of their own; every iteration trains the F of them it is told to"""

    def __init__(self, fkw, ckw, NF, R, n_c=8, n_g=16, seed=0, sd=None):
        self.fkw, self.NF, self.R, self.S = fkw, NF, R, n_c + n_g
        self.ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, **ckw)
        self.pos, self.quat, self.t = synth_target(NF, R, seed=seed)
        fs = O.FieldSpec(**{k: v for k, v in fkw.items() if k != "weight_dtype"})
        params = O.init_params(fs, NF, seed=seed, sigma=3.0) if fkw["encoding"] != "triplane" else O.init_params(fs, NF, seed=seed)
        params[f"_linears.{fkw['num_layers']}.weight"] *= 2.0
        g = torch.Generator().manual_seed(77 + seed)
        self.u_c = torch.rand(NF, R, n_c, generator=g)
        self.u_g = torch.rand(NF, R, n_g, generator=g)
        self.r = make_renderer(fkw, self.ckw, NF, params)
        if sd is not None:
            with torch.no_grad():
                self.r._model.all_fields_params["_neus_sd"].copy_(sd.to(DEV))
        self.r.set_field_poses(self.pos.to(DEV), self.quat.to(DEV))

    def target(self, sel, count=None):
        tg = make_target({k: v[sel] for k, v in self.t.items()}, sel)
        uc, ug = self.u_c[sel].to(DEV).contiguous(), self.u_g[sel].to(DEV).contiguous()
        if count is None:
            return tg, uc, ug
        d = {k: getattr(tg, k).clone() for k in Rr.Target._fields}        # rows >= count as the device sampler pads them
        for k, v in d.items():
            if k == "field_ids":
                v[count:] = -1
            elif v.dtype == torch.bool:
                v[count:] = False
            else:
                v[count:] = 0
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        return Rr.DeviceTarget(**d, count=cnt, subset_observed=None, subset_random=None, offsets=None, frame_cids=None,
                               u_xy=None, world_size=1), uc, ug

    def state(self):
        r, s = self.r, {}
        for k, v in r._model.all_fields_params.items():
            s["param", k] = v.clone()
        for k, st in r._optim_state.items():
            s["exp_avg", k], s["exp_avg_sq", k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        if r._model.lp_fields_params is not None:
            for k, v in r._model.lp_fields_params.items():
                if v.dtype != torch.float32:
                    s["lp", k] = v.clone()
        return s


def teacher_forced(sc, F, expect, label, counts=None, n_iter=N_ITER, seed=0):
    """The seven steps of the module docstring, n_iter times.  expect(launch counts of the updating call) asserts the site;
    counts: the active count of each iteration's padded DeviceTarget (None: plain targets)."""
    r = sc.r
    # what the case configured (gpu_common.make_renderer's defaults are the shipped set); the renderer fixes the betas
    hp = (sc.ckw.get("learning_rate", 1e-3), 0.9, 0.999, sc.ckw.get("adam_eps", 1e-15), sc.ckw.get("adam_weight_decay", 1e-5))
    sets = active_sets(sc.NF, F, n_iter, seed)
    seen = torch.zeros(sc.NF, dtype=torch.int64)
    acc = {}
    L = K.lib()
    K.check(L.ngm_profile_enable(1), "ngm_profile_enable")
    try:
        for it, sel in enumerate(sets):
            n = F if counts is None else counts[it % len(counts)]
            tgt, uc, ug = sc.target(sel, None if counts is None else n)
            rows = sel[:n].to(DEV)
            before = sc.state()                                                              # 1
            res = r.optimization_iteration(tgt, uc, ug, update=False)                        # 2
            kept = res["grads"]
            grads = {k: v.clone() for k, v in kept.items()}
            step0 = int(r._step_dev)
            K.check(L.ngm_profile_reset(), "ngm_profile_reset")
            r.optimization_iteration(tgt, uc, ug, update=True)                               # 3
            torch.cuda.synchronize()
            expect(launches())
            for k in kept:                                                                   # 4
                assert same_bits(kept[k][:n], grads[k][:n]), (label, it, k, "the updating call wrote another gradient")
            step = int(r._step_dev)
            assert step == step0 + 1 == r._step == it + 1, (step, step0, r._step, it)
            after = sc.state()
            # constants (the hash shifts) have a slot in the gradient / optimizer dicts but no gradient: never updated
            trained = [k for k in grads if ("exp_avg", k) in before and k not in K.NO_GRAD_PARAMS]
            assert trained, "no trained tensor?"
            for k in trained:                                                                # 5
                new = tuple(after[w, k][rows].reshape(n, -1) for w in ("param", "exp_avg", "exp_avg_sq"))
                old = tuple(before[w, k][rows].reshape(n, -1) for w in ("param", "exp_avg", "exp_avg_sq"))
                if it > 0 and k != "_neus_sd":
                    back = (seen[sel[:n]] > 0).to(DEV)
                    assert not bool(back.any()) or bool((old[1][back] != 0).any()), (label, k, "no moments to continue from")
                check_update(new, old, grads[k][:n].reshape(n, -1), hp, step, f"{label} it={it} {k}", acc.setdefault(k, Acc()))
                if ("lp", k) in after:                                                       # 7
                    assert same_bits(after["lp", k][rows], after["param", k][rows].to(after["lp", k].dtype)), \
                        (label, it, k, "16-bit copy != RNE cast of the new master")
            idle = torch.ones(sc.NF, dtype=torch.bool, device=DEV)
            idle[rows] = False
            for key in before:                                                               # 6
                if key[1] in trained:
                    assert same_bits(after[key][idle], before[key][idle]), (label, it, key, "an inactive row moved")
                else:
                    assert same_bits(after[key], before[key]), (label, it, key, "an untrained tensor moved")
            seen[sel[:n]] += 1
    finally:
        L.ngm_profile_enable(0)
    assert int((seen == 0).sum()) < sc.NF and bool((seen > 1).any()), "no row was trained twice"
    total = Acc()
    for k, a in acc.items():
        for o in "pmv":
            total.worst[o] = max(total.worst[o], a.worst[o])
            total.over[o] += a.over[o]
            total.n[o] += a.n[o]
    print(f"\nadam fused [{label}] {n_iter} iterations  {total.line()}")
    for k, a in acc.items():
        print(f"    {k:34s} {a.line()}")
    return acc


def mlp_site(F, P, want):
    """sites 3 / 4 for the MLP tensors: one k_grad_reduce launch, no plain Adam launch, and the workgroups per field"""
    bpf = plan_bwd(F, P, 128)
    assert (bpf > 8) == (want == 3), (F, P, bpf)

    def expect(n):
        assert n["grad_reduce"] == 1 and n["adam"] == 0 and n["hash_grad"] == 0 and n["hash_reduce"] == 0, n
    return expect, bpf


# (network, NF, F launched, R): workgroups per field on 256 CUs in the comment
MLP_CASES = {
    "site4_fourier_F32": (M1, 40, 32, 24),                       # 32 x 576 samples: 5 workgroups per field
    "site3_fourier_F2_12": (M1, 5, 2, 64),                        # 2 x 1536: 12 -- quarters of 3: k_grad_reduce's last tail loop
    "site3_fourier_F2_24": (M1, 5, 2, 128),                       # 2 x 3072: 24 -- the 16-wide tail loop AND the last one
    "site3_fourier_F1_38": (M1, 4, 1, 200),                       # 1 x 4800: 38 -- the eight-load prefetch, then the last tail
    "site4_concat_F32": ({**M1, "skip_mode": "concat"}, 36, 32, 24),
    "site3_concat_F2_24": ({**M1, "skip_mode": "concat"}, 5, 2, 128),
}


def _mlp_case(name, counts=None, ckw=None, weight_dtype=None):
    fkw, NF, F, R = MLP_CASES[name]
    if weight_dtype:
        fkw = {**fkw, "weight_dtype": weight_dtype}
    sc = Scene(fkw, ckw or {}, NF, R, seed=len(name))
    site = int(name[4])
    expect, bpf = mlp_site(F, R * sc.S, site)
    if site == 3 and torch.cuda.get_device_properties(0).multi_processor_count == 256:
        assert bpf == int(name.rsplit("_", 1)[1]), bpf
        assert bpf % 16 != 0
    label = f"{name}: site {site}, {'k_grad_reduce' if site == 3 else 'k_grad_reduce_flat'}" \
            f"{'<COUNTED>' if counts else ''}, {bpf} workgroups per field" + (f", {weight_dtype}" if weight_dtype else "")
    return teacher_forced(sc, F, expect, label, counts=counts, seed=len(name))


@pytest.mark.parametrize("name", list(MLP_CASES))
def test_fused_mlp_sites_3_and_4(name):
    _mlp_case(name)


def _hash_case(NF, F, R, counts=None, ckw=None, weight_dtype=None, seed=0):
    fkw = {**HASH, "weight_dtype": weight_dtype} if weight_dtype else HASH
    sc = Scene(fkw, {**EXACT, **(ckw or {})}, NF, R, seed=seed)
    chunks = hash_chunks(F, R * sc.S)
    bpf = plan_bwd(F, R * sc.S, 256)

    def expect(n):
        # the tables' update: inside k_hash_grad (one chunk, no k_hash_reduce launch) or in k_hash_reduce; never a plain Adam
        # launch (aligned tables); the MLP tensors: grad_reduce_one riding in the k_hash_grad launch, no k_grad_reduce launch
        assert n["hash_grad"] == 1 and n["adam"] == 0 and n["grad_reduce"] == 0, n
        assert n["hash_reduce"] == (0 if chunks == 1 else 1), (n, chunks)
    site = 5 if chunks == 1 else 6
    label = f"hash F={F} R={R}: site {site} ({'k_hash_grad epilogue' if site == 5 else f'k_hash_reduce, {chunks} chunks'})" \
            f" + site 4 riding in k_hash_grad ({bpf} workgroups per field)" + (", counted" if counts else "") \
            + (f", {weight_dtype}" if weight_dtype else "")
    return site, teacher_forced(sc, F, expect, label, counts=counts, seed=seed)


# one chunk: 32 fields x 16 levels fill the 512 workgroup slots; one field with <= 4096 samples.  Several: 2 fields x 12288 samples
@pytest.mark.parametrize("NF,F,R,site", [(36, 32, 512, 5), (4, 1, 128, 5), (5, 2, 512, 6)])
def test_fused_hash_sites_5_and_6(NF, F, R, site):
    got, acc = _hash_case(NF, F, R, seed=F)
    if torch.cuda.get_device_properties(0).multi_processor_count == 256 or (F, R) == (1, 128):
        assert got == site
    assert "_encoding.lattice_values" in acc and "_linears.0.weight" in acc and "_linears.1.bias" in acc


@pytest.mark.parametrize("name", ["site4_fourier_F32", "site3_fourier_F2_24"])
def test_fused_counted_mlp(name):
    F = MLP_CASES[name][2]
    _mlp_case(name, counts=[1, max(F // 2, 1), F])


@pytest.mark.parametrize("NF,F,R", [(36, 32, 512), (5, 2, 512)])
def test_fused_counted_hash(NF, F, R):
    _hash_case(NF, F, R, counts=[1, max(F // 2, 1), F], seed=10 + F)


def test_fused_triplane_planes_site2():
    """the feature planes: gradient from the fixed-point scatter, then k_adam_multi (site 2) from the renderer"""
    fkw = dict(encoding="triplane", resolution=16, num_components=32, tri_mode="sum", num_layers=1)
    NF, F, R = 6, 4, 33
    sc = Scene(fkw, {}, NF, R, n_c=6, n_g=10, seed=3)

    def expect(n):
        assert n["adam"] >= 1, n
    acc = teacher_forced(sc, F, expect, "triplane: site 2 (k_adam_multi) on plane_coef, MLP through k_grad_reduce", seed=3)
    assert "_encoding.plane_coef" in acc and acc["_encoding.plane_coef"].n["p"] > 0


def test_fused_neus_sd_site2():
    """geometry mode neus: `_neus_sd` is a one-float tensor per field updated by k_adam_multi (site 2, scalar path)"""
    NF, F, R = 6, 4, 40
    sd = torch.tensor([0.4, 0.8, -1.5, 1.1, 0.6, -0.9])
    sc = Scene(M1, dict(geometry_mode="neus", geometry_factor=5.0), NF, R, n_c=10, n_g=6, seed=4, sd=sd)
    assert sc.r._neus_fused()

    def expect(n):
        assert n["adam"] >= 1, n
    acc = teacher_forced(sc, F, expect, "neus: site 2 (k_adam_multi) on _neus_sd, MLP through k_grad_reduce", seed=4)
    assert "_neus_sd" in acc and acc["_neus_sd"].n["p"] == N_ITER * F


@pytest.mark.parametrize("dt", ["float16", "bfloat16"])
@pytest.mark.parametrize("net", ["fourier", "hash"])
def test_fused_reduced_precision_storage(net, dt):
    if net == "fourier":
        _mlp_case("site4_fourier_F32", weight_dtype=dt)
    else:
        _hash_case(5, 2, 512, weight_dtype=dt, seed=21)


@pytest.mark.parametrize("net", ["fourier", "hash"])
def test_fused_other_hyper_parameters(net):
    """learning rate, eps and weight decay away from their defaults (the renderer fixes the betas)"""
    ckw = dict(learning_rate=3e-2, adam_eps=1e-8, adam_weight_decay=1e-2)
    if net == "fourier":
        _mlp_case("site3_fourier_F2_24", ckw=ckw)
    else:
        _hash_case(4, 1, 128, ckw=ckw, seed=31)
