"""The counted training step: optimization_iteration / capture_iteration on a DeviceTarget as it is (launched at the
capacity Fcap, every kernel reads the number of active rows from device memory) and capture_training (sampler + step as
one graph per iteration).  Checked bitwise where the launch plan is the same (full capacity = the plain path; padding
content is never read; nothing outside the active rows moves; padding rows = fully masked rows), and to the project's
HIP-vs-oracle bars where it is not (against the materialised path, against the oracle)."""
import importlib.util
import json
import os
import socket
import sys
import time
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402

pytestmark = pytest.mark.gpu

# First act of the module: without the counted step a padded batch must never be launched (row -1 of the parameters would be
# indexed); every test below depends on these two.
assert hasattr(Rr.NeuralGraphRenderer, "capture_training"), "NeuralGraphRenderer.capture_training is missing"
if not os.path.exists(K.LIB_PATH):       # a fresh checkout: build on demand, as the CPU modules' fixtures do (collection must not fail)
    from neural_graph_mapping_amd import build as _build
    _build.build(verbose=False)
assert hasattr(K.lib(), "ngm_render_fwd_counted"), "the library does not export ngm_render_fwd_counted"

import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from gpu_common import (DEV, NRGBD, close, compare_losses, grad_close, hash_grad_close, kink_free_draws, make_renderer,  # noqa: E402
                        make_target, synth_target)
from neural_graph_mapping_amd import distributed as D  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from oracle import ngm_oracle as O  # noqa: E402
from test_gpu_safety import guard_bands  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M1 = dict(encoding="fourier", dim_enc=64, num_layers=2)
HASH = dict(encoding="permuto", num_layers=1, nr_levels=16, log2_hashmap_size=12, coarsest_scale=1.0, finest_scale=1e-4)
NETS = {"m1": M1, "hash": HASH}
# Configurations that reach the guards the two flagship networks do not: (field kwargs, config kwargs, Fcap, R, n_c, n_g)
#   skip_concat   Fourier + skip concat: k_stash_bwd's ray clip, k_field_bwd (32-sample tiles, recompute)
#   nerf_add      NeRF encoding + skip add: k_stash_bwd, k_field_bwd<NEED_COS>
#   narrow        Fourier 32 x 1 x 32: the 16-sample-tile kernels (k_field_bwd16s / k_field_bwd16 with mlp_matmul f32)
#   density       geometry mode density: k_stash_bwd in front of k_field_bwd_b3<FC = false>
#   hash_float    hash_grad_atomics float: the fp32-atomics instance of k_hash_grad
#   hash_f32      hash network, fp32 MFMA: k_stash_bwd + k_field_bwd16 + k_hash_grad
#   many_blocks   Fcap = 2 with R * S = 3072 samples per field: more than 8 backward blocks per field -> k_grad_reduce
OTHER = {
    "skip_concat": ({**M1, "skip_mode": "concat"}, {}, 5, 24, 8, 16),
    "nerf_add": (dict(encoding="nerf", num_octaves=8, num_layers=1, skip_mode="add"), {}, 5, 24, 8, 8),
    "narrow": (dict(encoding="fourier", dim_enc=32, num_layers=1), {}, 5, 24, 8, 16),
    "narrow_f32": (dict(encoding="fourier", dim_enc=32, num_layers=1), dict(mlp_matmul="f32"), 5, 24, 8, 16),
    "density": (M1, dict(geometry_mode="density", geometry_factor=5.0), 5, 24, 8, 16),
    "hash_float": (HASH, dict(hash_grad_atomics="float"), 5, 24, 8, 16),
    "hash_f32": (HASH, dict(mlp_matmul="f32"), 5, 24, 8, 16),
    "many_blocks": (M1, {}, 2, 128, 8, 16),
}
FIELDS = Rr.Target._fields
LOSS_KEYS = ("combined", "termination", "photometric_l1", "depth_huber", "freespace", "tsdf")
REPORT = {}          # figures the tests measured; profiles/r08_device_iteration.json quotes them


def _report(key, value):
    """keep a measured figure; with NGM_DEVICE_ITERATION_REPORT=<file.json> set, also merge it into that file"""
    REPORT[key] = value
    path = os.environ.get("NGM_DEVICE_ITERATION_REPORT")
    if not path:
        return
    old = {}
    if os.path.exists(path):
        try:
            old = json.load(open(path))
        except ValueError:
            old = {}
    old.update(REPORT)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1, sort_keys=True)


class Batch:
    """Fcap rows of synthetic rays on Fcap distinct fields of a map of N (ids neither 0 nor N - 1, in no particular order),
    explicit jitter draws, and renderers that all start from the same parameters"""

    def __init__(self, fkw, Fcap, R, n_c=8, n_g=16, seed=0, ckw=None, extra_fields=6):
        self.fkw, self.Fcap, self.R, self.n_c, self.n_g = fkw, Fcap, R, n_c, n_g
        self.ckw = dict(num_samples_coarse=n_c, num_samples_depth_guided=n_g, termination_weight=0.3, **(ckw or {}))
        self.N = N = Fcap + extra_fields
        g = torch.Generator().manual_seed(500 + seed)
        self.ids = 1 + torch.randperm(N - 2, generator=g)[:Fcap]
        self.pos, self.quat, self.t = synth_target(Fcap, R, seed=seed)
        self.pos_all = 0.5 * torch.randn(N, 3, generator=g)
        self.quat_all = torch.nn.functional.normalize(torch.randn(N, 4, generator=g), dim=-1)
        self.pos_all[self.ids], self.quat_all[self.ids] = self.pos, self.quat
        self.fs = O.FieldSpec(**{k: v for k, v in fkw.items() if k != "weight_dtype"})
        self.params = O.init_params(self.fs, N, seed=seed, sigma=3.0)
        self.params[f"_linears.{fkw['num_layers']}.weight"] *= 2.0
        self.u_c = torch.rand(Fcap, R, n_c, generator=g)
        self.u_g = torch.rand(Fcap, R, n_g, generator=g) if n_g else None

    def renderer(self):
        r = make_renderer(self.fkw, self.ckw, self.N, self.params)
        r.set_field_poses(self.pos_all.to(DEV), self.quat_all.to(DEV))
        return r

    def draws(self, n=None):
        sl = slice(None) if n is None else slice(0, n)
        return self.u_c[sl].to(DEV).contiguous(), (None if self.u_g is None else self.u_g[sl].to(DEV).contiguous())

    def target(self, n=None, t=None):
        """the plain Target of the first n rows (all: None)"""
        t = self.t if t is None else t
        tg = make_target(t, self.ids)
        return tg if n is None else Rr.Target(*(getattr(tg, k)[:n].contiguous() for k in FIELDS))

    def padded(self, n, hostile=False, t=None):
        """DeviceTarget with count n: rows >= n as the sampler pads them (field_ids -1, masks 0, zeros), or hostile"""
        tg = self.target(t=t)
        d = {k: getattr(tg, k).clone() for k in FIELDS}
        g = torch.Generator().manual_seed(9)
        for k, v in d.items():
            if k == "field_ids":
                v[n:] = -1
                if hostile:            # valid ids of OTHER fields (0 and N - 1 among them) and out-of-range ids, alternating
                    others = [i for i in range(self.N) if i not in self.ids[:n].tolist()]
                    bad = [0, self.N - 1, self.N + 1000, -7, 2 ** 40] + others
                    v[n:] = torch.tensor([bad[i % len(bad)] for i in range(self.Fcap - n)], dtype=torch.int64)
            elif v.dtype == torch.bool:
                v[n:] = bool(hostile)
            elif v.dtype.is_floating_point:
                v[n:] = 0
                if hostile and self.Fcap > n:
                    fill = torch.tensor([float("nan"), float("inf"), -float("inf"), 1e30])
                    idx = torch.randint(0, 4, tuple(v[n:].shape), generator=g)
                    v[n:] = fill[idx].to(DEV)
            else:
                v[n:] = 0
                if hostile and self.Fcap > n:
                    v[n:] = torch.randint(-2 ** 40, 2 ** 40, tuple(v[n:].shape), generator=g).to(DEV)
        cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
        return Rr.DeviceTarget(**d, count=cnt, subset_observed=None, subset_random=None, offsets=None, frame_cids=None,
                               u_xy=None, world_size=1)

    def hostile_draws(self, n):
        uc, ug = self.draws()
        uc, ug = uc.clone(), (None if ug is None else ug.clone())
        uc[n:] = float("nan")
        if ug is not None:
            ug[n:] = float("inf")
        return uc, ug


def state(r):
    s = {}
    for k, v in r._model.all_fields_params.items():
        s["param " + k] = v.clone()
    for k, st in r._optim_state.items():
        s["exp_avg " + k], s["exp_avg_sq " + k] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    if r._model.lp_fields_params is not None:
        for k, v in r._model.lp_fields_params.items():
            s["lp " + k] = v.clone()
    return s


def assert_state_equal(a, b, rows=None, what=""):
    assert a.keys() == b.keys()
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert torch.equal(x, y), (what, k)


def losses_of(res):
    return {k: res[k].clone() for k in LOSS_KEYS}


def assert_losses_equal(a, b):
    for k in LOSS_KEYS:
        assert torch.equal(a[k], b[k]) or (bool(torch.isnan(a[k])) and bool(torch.isnan(b[k]))), (k, a[k], b[k])


# ------------------------------------------------------------------------------------------------ 1. full capacity
@pytest.mark.parametrize("net", ["m1", "hash"])
def test_full_capacity_is_the_plain_path_bitwise(net):
    b = Batch(NETS[net], 4, 40, seed=1)
    ra, rb = b.renderer(), b.renderer()
    uc, ug = b.draws()
    plain = ra.optimization_iteration(b.target(), uc, ug, update=False)
    counted = rb.optimization_iteration(b.padded(b.Fcap), uc, ug, update=False)
    assert_losses_equal(losses_of(plain), losses_of(counted))
    for k in plain["grads"]:
        assert torch.equal(plain["grads"][k], counted["grads"][k]), k
    assert torch.equal(plain["prediction"].rgbds, counted["prediction"].rgbds)
    for _ in range(2):
        la = ra.optimization_iteration(b.target(), uc, ug, update=True)
        lb = rb.optimization_iteration(b.padded(b.Fcap), uc, ug, update=True)
        assert_losses_equal(losses_of(la), losses_of(lb))
    assert_state_equal(state(ra), state(rb), what="full capacity")
    assert ra._step == rb._step == 2 and int(ra._step_dev) == int(rb._step_dev) == 2


# ------------------------------------------------------------------------------------------------ 2. padding is never read
@pytest.mark.parametrize("count", ["one", "half", "all_but_one"])
@pytest.mark.parametrize("net", ["m1", "hash"])
def test_padding_is_never_read(net, count):
    b = Batch(NETS[net], 6, 24, seed=2)
    n = dict(one=1, half=b.Fcap // 2, all_but_one=b.Fcap - 1)[count]
    ra, rb = b.renderer(), b.renderer()
    uc, ug = b.draws()
    huc, hug = b.hostile_draws(n)
    clean = ra.optimization_iteration(b.padded(n), uc, ug, update=False)
    hostile = rb.optimization_iteration(b.padded(n, hostile=True), huc, hug, update=False)
    assert_losses_equal(losses_of(clean), losses_of(hostile))
    assert all(bool(torch.isfinite(clean[k])) for k in LOSS_KEYS)
    for k in clean["grads"]:
        assert torch.equal(clean["grads"][k][:n], hostile["grads"][k][:n]), k
        assert bool(torch.isfinite(hostile["grads"][k][:n]).all()), k
    assert torch.equal(clean["prediction"].rgbds[:n], hostile["prediction"].rgbds[:n])
    for _ in range(2):
        la = ra.optimization_iteration(b.padded(n), uc, ug, update=True)
        lb = rb.optimization_iteration(b.padded(n, hostile=True), huc, hug, update=True)
        assert_losses_equal(losses_of(la), losses_of(lb))
    sa, sb = state(ra), state(rb)
    assert_state_equal(sa, sb, what="hostile padding")
    assert all(bool(torch.isfinite(v.float()).all()) for v in sb.values())


# ------------------------------------------------------------------------------------------------ 3. nothing else moves
@pytest.mark.parametrize("net", ["m1", "hash", "m1_bf16"])
def test_nothing_else_moves(net):
    fkw = {**M1, "weight_dtype": "bfloat16"} if net == "m1_bf16" else NETS[net]
    b = Batch(fkw, 5, 24, seed=3)
    n = 2
    SENT = -12345.5
    with guard_bands() as bands:
        r = b.renderer()
        w = r._workspace(b.Fcap, b.R)
        w["grads"], w["gs"], w["gflat"] = ops.alloc_grads(r._fc, b.Fcap, DEV)
        for k in ("rgbds", "color_vars", "depth_vars", "term_probs"):
            w[k].fill_(SENT)
        for v in w["grads"].values():
            v.fill_(SENT)
        before = state(r)
        uc, ug = b.hostile_draws(n)
        out = r.optimization_iteration(b.padded(n, hostile=True), uc, ug, update=True)
        bands.check()
    after = state(r)
    active = b.ids[:n].to(DEV)
    others = torch.tensor([i for i in range(b.N) if i not in b.ids[:n].tolist()], device=DEV)
    assert 0 in others.tolist() and b.N - 1 in others.tolist()       # what a wrapped -1 / a zero would hit
    assert_state_equal(before, after, rows=others, what="rows outside field_ids[:count]")
    changed = [k for k in before if not torch.equal(before[k][active], after[k][active])]
    assert any(k.startswith("param ") for k in changed) and any(k.startswith("exp_avg ") for k in changed)
    if net == "m1_bf16":
        assert any(k.startswith("lp ") for k in changed)
    p = out["prediction"]
    for name, v in (("rgbds", p.rgbds), ("color_vars", p.color_vars), ("depth_vars", p.depth_vars), ("term_probs", p.term_probs)):
        assert bool((v[n:] == SENT).all()), name
        assert not bool((v[:n] == SENT).any()), name
    for k, v in w["grads"].items():
        if k in K.NO_GRAD_PARAMS:
            continue
        assert bool((v[n:] == SENT).all()), k
        assert not bool((v[:n] == SENT).all()), k


# ------------------------------------------------------------------------------------------------ 2 + 3, the other kernels
@pytest.mark.parametrize("cfg", sorted(OTHER))
def test_other_kernels_never_read_padding_and_move_nothing_else(cfg):
    """Items 2 and 3 on the configurations of OTHER: with 0 < count < Fcap, hostile padding (field ids of other fields and
    out of range, NaN / inf everywhere) changes nothing observable, and an update moves no row outside field_ids[:count].
    hash_float: fp32 LDS atomics are not reproducible run to run, so its table gradient is held to the project's run-to-run
    bar for that mode (1e-5 of max, tests/test_gpu_parity.py) instead of bitwise, and its trained state is not compared."""
    fkw, ckw, Fcap, R, n_c, n_g = OTHER[cfg]
    b = Batch(fkw, Fcap, R, n_c, n_g, seed=8, ckw=ckw)
    n = 1 if Fcap == 2 else 3
    ra, rb = b.renderer(), b.renderer()
    uc, ug = b.draws()
    huc, hug = b.hostile_draws(n)
    clean = ra.optimization_iteration(b.padded(n), uc, ug, update=False)
    hostile = rb.optimization_iteration(b.padded(n, hostile=True), huc, hug, update=False)
    if cfg == "many_blocks":
        assert K.lib().ngm_debug_last_bwd_variant() == 3
    assert_losses_equal(losses_of(clean), losses_of(hostile))
    assert bool(torch.isfinite(clean["tsdf"])) and bool(torch.isfinite(clean["freespace"]))
    floaty = cfg == "hash_float"
    for k in clean["grads"]:
        if k in K.NO_GRAD_PARAMS:
            continue
        assert bool(torch.isfinite(hostile["grads"][k][:n]).all()), k
        if floaty and k == "_encoding.lattice_values":
            grad_close(hostile["grads"][k][:n], clean["grads"][k][:n], 1e-5, "float atomics, clean vs hostile padding")
        else:
            assert torch.equal(clean["grads"][k][:n], hostile["grads"][k][:n]), k
    assert torch.equal(clean["prediction"].rgbds[:n], hostile["prediction"].rgbds[:n])
    before = state(rb)
    ra.optimization_iteration(b.padded(n), uc, ug, update=True)
    rb.optimization_iteration(b.padded(n, hostile=True), huc, hug, update=True)
    sa, sb = state(ra), state(rb)
    if not floaty:
        assert_state_equal(sa, sb, what="hostile padding, " + cfg)
    assert all(bool(torch.isfinite(v.float()).all()) for v in sb.values())
    active = b.ids[:n].to(DEV)
    others = torch.tensor([i for i in range(b.N) if i not in b.ids[:n].tolist()], device=DEV)
    assert_state_equal(before, sb, rows=others, what="rows outside field_ids[:count], " + cfg)
    assert any(not torch.equal(before[k][active], sb[k][active]) for k in before if k.startswith("param "))


# ------------------------------------------------------------------------------------------------ 4. padding = masked rows
@pytest.mark.parametrize("net", ["m1", "hash"])
def test_padding_rows_equal_fully_masked_rows(net):
    """Same launch plan, same partial order: a padding row and a real row that no loss term sees (masks 0, gt 0) both add
    exactly +0 to every sum, so the losses and the gradient rows < n are bitwise equal."""
    b = Batch(NETS[net], 5, 24, seed=4)
    n = 3
    t = {k: v.clone() for k, v in b.t.items()}
    t["depth_mask"][n:] = False
    t["term_mask"][n:] = False
    t["gt"][n:] = 0.0
    t["rgbds"][n:] = 0.0
    ra, rb = b.renderer(), b.renderer()
    uc, ug = b.draws()
    masked = ra.optimization_iteration(b.target(t=t), uc, ug, update=False)
    counted = rb.optimization_iteration(b.padded(n, t=t), uc, ug, update=False)
    assert_losses_equal(losses_of(masked), losses_of(counted))
    for k in masked["grads"]:
        assert torch.equal(masked["grads"][k][:n], counted["grads"][k][:n]), k


# ------------------------------------------------------------------------------------------------ 5. materialised + oracle
@pytest.mark.parametrize("net", ["m1", "hash"])
def test_agrees_with_the_materialised_path_and_the_oracle(net):
    """Different launch plans (F = count vs F = Fcap): fp32 sums are reordered, so this is held to the project's
    HIP-vs-oracle bars (compare_losses / grad_close defaults), not bitwise; both runs are also held to the oracle.
    M1: 3 active rows of a capacity of 32, 100 rays x 24 samples -- forward and backward plans differ (backward, F = 3: 19
    workgroups per field of 128 samples, F = 32: 7 of 384), so the per-field gradient sums are reordered as well as the loss
    sums.  Hash: 3 of 5 rows x 24 rays, where both backward plans are 3 workgroups per field -- on the 32 x 100 shape the
    PLAIN (materialised) path misses the hash network's own oracle bar for table level 4 (0.0174 of the level's max against
    6e-3 on this draw; the bars were measured on other statistics), which says nothing about the counted step; its padded-vs-
    materialised comparison on that shape is test_padded_vs_materialised_where_the_plans_differ below."""
    fkw = NETS[net]
    b = Batch(fkw, 32, 100, seed=5) if net == "m1" else Batch(fkw, 5, 24, seed=5)
    n = 3
    rs = O.RenderSpec(num_samples_coarse=b.n_c, num_samples_depth_guided=b.n_g, termination_weight=0.3)
    sub = {k: v[:n] for k, v in b.t.items()}
    pr = {k: v[b.ids[:n]] for k, v in b.params.items()}
    u_c, u_g, sub = kink_free_draws(sub, b.pos[:n], b.quat[:n], pr, b.fs, rs, b.u_c[:n], b.u_g[:n])
    b.u_c[:n], b.u_g[:n] = u_c, u_g
    for k in sub:
        b.t[k] = torch.cat([sub[k], b.t[k][n:]])
    po = {k: v.clone().requires_grad_(k != "_encoding.random_shift_per_level") for k, v in pr.items()}
    pred = O.render_ijs(sub["ijs"], sub["c2ws"], NRGBD, b.pos[:n], b.quat[:n], po, b.fs, rs, sub["near"], sub["far"], sub["gt"], u_c, u_g)
    ra, rb = b.renderer(), b.renderer()
    mat = ra.optimization_iteration(b.target(n), *b.draws(n), update=False)
    cnt = rb.optimization_iteration(b.padded(n, hostile=True), *b.hostile_draws(n), update=False)
    tol = dict(rtol=2e-3, atol=1e-5) if net == "hash" else dict(rtol=3e-4, atol=1e-6)
    loss, _ = compare_losses(mat, pred, sub, rs, **tol)
    compare_losses(cnt, pred, sub, rs, **tol)
    loss["combined"].backward()
    worst = 0.0
    for k in LOSS_KEYS:
        close(cnt[k], mat[k], rtol=3e-4, atol=1e-6)
    for k in po:
        if po[k].grad is None:
            continue
        for label, res in (("materialised", mat), ("counted", cnt)):
            try:
                if net == "hash":
                    hash_grad_close(res["grads"][k][:n], po[k].grad, k)
                else:
                    grad_close(res["grads"][k][:n], po[k].grad, name=k)
            except AssertionError as err:
                raise AssertionError(f"{label} run against the oracle: {err}") from None
        grad_close(cnt["grads"][k][:n], mat["grads"][k], name="padded vs materialised " + k)
        scale = mat["grads"][k].abs().max().clamp_min(1e-12)
        worst = max(worst, float((cnt["grads"][k][:n] - mat["grads"][k]).abs().max() / scale))
    print(f"padded vs materialised, {net}, Fcap {b.Fcap} x {b.R} rays: worst gradient difference {worst:.3e} of max")
    _report(f"padded_vs_materialised_worst_grad_frac_of_max_{net}_{b.Fcap}x{b.R}", worst)


def test_padded_vs_materialised_where_the_plans_differ():
    """Hash network, 3 active rows of a capacity of 32, 100 rays x 24 samples: backward plan F = 3: 10 workgroups per field of
    256 samples, F = 32: 5 of 512.  Counted against materialised, same rows and draws, to grad_close's default bar and
    compare_losses' tolerances; the worst gradient difference is recorded."""
    b = Batch(HASH, 32, 100, seed=5)
    n = 3
    ra, rb = b.renderer(), b.renderer()
    mat = ra.optimization_iteration(b.target(n), *b.draws(n), update=False)
    cnt = rb.optimization_iteration(b.padded(n, hostile=True), *b.hostile_draws(n), update=False)
    for k in LOSS_KEYS:
        close(cnt[k], mat[k], rtol=3e-4, atol=1e-6)
    worst = 0.0
    for k, v in mat["grads"].items():
        if k in K.NO_GRAD_PARAMS:
            continue
        grad_close(cnt["grads"][k][:n], v, name="padded vs materialised, plans differ, " + k)
        worst = max(worst, float((cnt["grads"][k][:n] - v).abs().max() / v.abs().max().clamp_min(1e-12)))
    print(f"padded vs materialised, hash, Fcap 32 x 100 rays: worst gradient difference {worst:.3e} of max")
    _report("padded_vs_materialised_worst_grad_frac_of_max_hash_32x100", worst)


# ------------------------------------------------------------------------------------------------ 6. ragged / small shapes
RAGGED = [  # Fcap, count, R, n_c, n_g
    (3, 2, 7, 3, 2),       # R * S = 35: fields start mid-tile, the tile after the last active field is half unwritten
    (4, 3, 5, 4, 4),       # R < 8
    (1, 0, 9, 4, 4), (1, 1, 9, 4, 4),
    (32, 1, 12, 8, 16),
    (5, 4, 33, 3, 0),
]


@pytest.mark.parametrize("net", ["m1", "m1_half", "m1_bf16", "hash"])
@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_and_small_shapes(net, shape):
    """The workspace (activation stash included) is pre-filled once with zeros and once with NaN bit patterns: the forward of
    a padding row writes none of it, so a backward that read a sample beyond the last active field's would differ (or turn
    NaN).  Bitwise equal, finite, and within the bars of the materialised path."""
    Fcap, n, R, n_c, n_g = shape
    fkw = {**M1, "weight_dtype": "bfloat16"} if net == "m1_bf16" else NETS.get(net, M1)
    ckw = dict(activation_stash="half") if net == "m1_half" else {}
    b = Batch(fkw, Fcap, R, n_c, n_g, seed=6, ckw=ckw)
    runs = []
    for fill in (0x00, 0xFF):
        r = b.renderer()
        r._workspace(Fcap, R)["ws"].fill_(fill)
        uc, ug = b.hostile_draws(n)
        res = r.optimization_iteration(b.padded(n, hostile=True), uc, ug, update=False)
        rec = dict(loss=losses_of(res), grads={k: v[:n].clone() for k, v in res["grads"].items()})
        r._workspace(Fcap, R)["ws"].fill_(fill)
        r.optimization_iteration(b.padded(n, hostile=True), uc, ug, update=True)
        rec["state"] = state(r)
        runs.append(rec)
    assert_losses_equal(runs[0]["loss"], runs[1]["loss"])
    for k in runs[0]["grads"]:
        assert torch.equal(runs[0]["grads"][k], runs[1]["grads"][k]), k
        assert bool(torch.isfinite(runs[1]["grads"][k]).all()), k
    assert_state_equal(runs[0]["state"], runs[1]["state"], what="workspace fill")
    assert all(bool(torch.isfinite(v.float()).all()) for v in runs[1]["state"].values())
    if n == 0:
        return
    rm = b.renderer()
    mat = rm.optimization_iteration(b.target(n), *b.draws(n), update=False)
    for k in LOSS_KEYS:
        close(runs[1]["loss"][k], mat[k], rtol=3e-4, atol=1e-6, equal_nan=True)
    for k, v in mat["grads"].items():
        if k not in K.NO_GRAD_PARAMS:
            grad_close(runs[1]["grads"][k], v, name="ragged padded vs materialised " + k)


# ------------------------------------------------------------------------------------------------ 7. count == 0
@pytest.mark.parametrize("net", ["m1", "hash", "m1_separate"])
def test_count_zero_is_an_idle_iteration(net):
    b = Batch(NETS.get(net, M1), 4, 16, seed=7)
    ra, rb = b.renderer(), b.renderer()
    if net == "m1_separate":
        K.lib().ngm_debug_disable_fused_comp(1)        # the bookkeeping of k_stash_bwd's block 0 instead of the fused backward's
    try:
        before = state(ra)
        step0 = ra._step
        got = ra.optimization_iteration(b.padded(0, hostile=True), *b.hostile_draws(0), update=True)
        torch.cuda.synchronize()
    finally:
        K.lib().ngm_debug_disable_fused_comp(0)
    want = rb._idle_iteration(True)
    for k in LOSS_KEYS:
        torch.testing.assert_close(got[k].cpu(), want[k].cpu(), rtol=0, atol=0, equal_nan=True)
    assert bool(torch.isnan(got["combined"]))
    assert_state_equal(before, state(ra), what="count 0")
    assert ra._step == step0 + 1 == rb._step
    assert int(ra._step_dev) == step0 + 1 == int(rb._step_dev)      # one device counter: Adam step and Philox jitter offset
    # and the next iteration is an ordinary one on the advanced counters
    nxt = ra.optimization_iteration(b.padded(2), *b.draws(), update=True)
    assert bool(torch.isfinite(nxt["combined"])) and int(ra._step_dev) == step0 + 2


# ------------------------------------------------------------------------------------------------ 8. one graph, no sync
class PartScene:
    """map + keyframe store as tests/test_gpu_target_device.Scene; the fields of `hidden` sit behind every camera, so the
    sampler drops them whenever it draws them: the count varies from iteration to iteration"""

    def __init__(self, num_fields, num_frames, hidden, H=48, W=64, seed=0):
        g = torch.Generator().manual_seed(seed)
        pos = torch.rand(num_fields, 3, generator=g) * torch.tensor([8.0, 6.0, 5.0]) - torch.tensor([4.0, 3.0, 7.0])
        hidden = torch.as_tensor(hidden)
        pos[hidden, 2] = -pos[hidden, 2] + 4.0
        c2w = torch.eye(4).repeat(num_frames, 1, 1)
        c2w[:, :3, 3] = torch.rand(num_frames, 3, generator=g) * 4.0 - 2.0
        rgbd = torch.rand(num_frames, H, W, 4, generator=g)
        rgbd[..., 3] = 2.0 + 8.0 * rgbd[..., 3]
        quat = torch.zeros(num_fields, 4)
        quat[:, 0] = 1.0
        self.positions, self.quat = pos.to(DEV), quat.to(DEV)
        self.c2w, self.rgbd = c2w.to(DEV), rgbd.to(DEV).contiguous()
        self.f2s = torch.arange(num_frames).to(DEV)
        self.cam = Rr.Camera(W, H, 0.8 * W, 0.8 * W, W / 2 - 0.5, H / 2 - 0.5, pixel_center=0.0)
        self.num_fields = num_fields

    def renderer(self, fkw, seed=0):
        fs = O.FieldSpec(**fkw)
        params = O.init_params(fs, self.num_fields, seed=seed, sigma=3.0)
        r = make_renderer(fkw, dict(num_samples_coarse=4, num_samples_depth_guided=4, field_radius=1.0), self.num_fields, params)
        r.set_field_poses(self.positions, self.quat)
        return r

    def args(self, cur, T, R):
        return (cur, self.c2w, self.rgbd, self.f2s, T, R)


@pytest.mark.parametrize("net", ["m1", "hash"])
def test_capture_training_one_graph_serves_every_count(net):
    N, T, R, SEED, NIT = 40, 12, 32, 5, 20
    sc = PartScene(N, 12, hidden=list(range(0, N, 2)), seed=1)
    cur = torch.arange(0, N, 3, device=DEV)
    ra, rb = sc.renderer(NETS[net]), sc.renderer(NETS[net])
    start = state(ra)
    step = ra.capture_training(*sc.args(cur, T, R), seed=SEED, camera=sc.cam)
    assert isinstance(step.graph, torch.cuda.CUDAGraph) and isinstance(step.target, Rr.DeviceTarget)
    assert_state_equal(start, state(ra), what="capture_training trains nothing by itself")
    assert int(ra._target_iter_dev) == 0 and ra._step == 0
    counts, la = [], None
    for _ in range(NIT):
        la = step()
        counts.append(int(step.target.count))
    lb = None
    for i in range(NIT):
        t = rb.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=SEED, iteration=i)
        assert int(t.count) == counts[i]
        lb = rb.optimization_iteration(t, seed=SEED)
    torch.cuda.synchronize()
    assert len(set(counts)) > 1 and max(counts) > 0, counts          # one graph demonstrably served several active counts
    assert_losses_equal(losses_of(la), losses_of(lb))
    assert_state_equal(state(ra), state(rb), what="20 replays vs 20 eager counted iterations")
    assert int(ra._target_iter_dev) == NIT and ra._step == NIT == int(ra._step_dev)
    changed = [k for k, v in state(ra).items() if not torch.equal(v, start[k])]
    assert changed, "nothing was trained"
    # the graph reads its inputs in place: a different tensor at replay is refused on the host
    ra._global_map_dict["positions"] = ra._global_map_dict["positions"].clone()
    with pytest.raises(RuntimeError, match="capture again"):
        step()


# ------------------------------------------------------------------------------------------------ 9. training quality
def _example():
    spec = importlib.util.spec_from_file_location("fit_synthetic", os.path.join(ROOT, "examples", "fit_synthetic.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_training_quality_on_the_example_scene():
    """capture_training against the materialised loop on examples/fit_synthetic.py: identical targets and jitter, only the
    summation order differs.  The device loop's PSNR may fall short of the materialised loop's by no more than the spread
    of the materialised loop over three jitter seeds, measured here."""
    mod = _example()
    iters = 200
    mats = [mod.main(iters=iters, device=str(DEV), quiet=True, loop="materialize", jitter_seed=s)[1] for s in (0, 1, 2)]
    spread = max(mats) - min(mats)
    losses, dev_psnr, derr = mod.main(iters=iters, device=str(DEV), quiet=True, loop="device", jitter_seed=0)
    print(f"PSNR after {iters} iterations: capture_training {dev_psnr:.3f} dB, materialised (jitter seeds 0, 1, 2) "
          f"{mats[0]:.3f} / {mats[1]:.3f} / {mats[2]:.3f} dB, spread {spread:.3f} dB")
    _report("psnr_db", dict(capture_training=dev_psnr, materialised=mats, spread=spread, iters=iters))
    assert losses[-1] < 0.25 * losses[0], losses
    assert dev_psnr >= mats[0] - spread, (dev_psnr, mats, spread)


# ------------------------------------------------------------------------------------------------ 10. two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


TWO = dict(N=24, T=6, R=16, SEED=11, NIT=8)


def _two_scene():
    # rank 1 owns the odd ids: all of them hidden except two, so that most draws leave rank 1 without a field
    N = TWO["N"]
    hidden = [i for i in range(1, N, 2) if i not in (5, 13)]
    return PartScene(N, 10, hidden=hidden, seed=3), torch.arange(0, N, 2, device=DEV)[:6].contiguous()


def _two_worker(rank, world, port, out, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    torch.cuda.set_device(0)
    D.init_from_env(backend="gloo")
    sc, cur = _two_scene()
    r = sc.renderer(M1)
    r.process_group = dist.group.WORLD
    if mode == "peer":
        r.peer_exchange = D.PeerExchange(dist.group.WORLD, timeout_s=20.0)
    step = r.capture_training(*sc.args(cur, TWO["T"], TWO["R"]), seed=TWO["SEED"], camera=sc.cam, world_size=world, rank=rank)
    counts, losses = [], []
    for _ in range(TWO["NIT"]):
        res = step()
        counts.append(int(step.target.count))
        losses.append({k: res[k].cpu().clone() for k in LOSS_KEYS})
    torch.cuda.synchronize()
    graphs = step.graph
    rec = dict(counts=counts, losses=losses, state={k: v.cpu() for k, v in state(r).items()}, step_dev=int(r._step_dev),
               it_dev=int(r._target_iter_dev), one_graph=isinstance(graphs, torch.cuda.CUDAGraph),
               two_graphs=isinstance(graphs, tuple) and len(graphs) == 2,
               status=r.peer_exchange.status() if mode == "peer" else 0)
    torch.save(rec, os.path.join(out, f"two_{mode}{rank}.pt"))
    dist.barrier()
    if mode == "peer":
        r.peer_exchange.close()
    dist.destroy_process_group()


def _two_emulated():
    """The same sharded run in one process, on the PLAIN path: each rank's target is materialised (active rows come first, so
    a ray keeps its row and with it its Philox jitter), a rank with rows runs the un-counted forward / backward at F = count,
    a rank without rows is an idle iteration, and the exchange's sum 0 + v_0 + v_1 goes into both -- a reference that runs
    none of the counted kernels.  (It cannot be the unsharded run: the jitter of a ray is keyed by its row in the rank's own
    batch -- jitter() in csrc/ngm_device.h --, so a sharded run draws other jitter than the unsharded one.)"""
    sc, cur = _two_scene()
    rs = [sc.renderer(M1) for _ in range(2)]
    counts, losses = [[], []], [[], []]
    for i in range(TWO["NIT"]):
        ctx, sums = [None, None], [None, None]
        for k, r in enumerate(rs):
            t = r.sample_target_mv_device(*sc.args(cur, TWO["T"], TWO["R"]), camera=sc.cam, seed=TWO["SEED"], iteration=i,
                                          world_size=2, rank=k)
            n = int(t.count)
            counts[k].append(n)
            if n > 0:
                r.process_group = "emulated"                  # not None: the forward reduces its sums instead of deferring
                ctx[k] = r._iteration_forward(t.materialize(), None, None, TWO["SEED"], advance=True)
                sums[k] = ctx[k]["w"]["sums"].clone()
            else:
                sums[k] = torch.zeros(16, device=DEV)
        tot = torch.zeros(16, device=DEV) + sums[0]
        tot = tot + sums[1]
        for k, r in enumerate(rs):
            if ctx[k] is not None:
                ctx[k]["w"]["sums"].copy_(tot)
                res = r._iteration_backward(ctx[k], True)
            else:
                r.process_group = None
                r._idle_iteration(True)                       # the counters of an idle rank; its loss is the global one
                rc = r._rc_train
                res = D.loss_values_from_sums(tot, rc.w_termination, rc.w_photometric, rc.w_depth, rc.w_freespace, rc.w_tsdf,
                                              "l1", "huber")
            losses[k].append({q: res[q].cpu().clone() for q in LOSS_KEYS})
    return counts, losses, [{k: v.cpu() for k, v in state(r).items()} for r in rs]


@pytest.mark.parametrize("mode", ["peer", "gloo"])
def test_two_ranks_capture_training(tmp_path, mode):
    """Each rank captures capture_training(world_size=2, rank=r) -- with `peer_exchange` one graph, with gloo the two-graph
    form -- and replays it; rank 1 owns almost only hidden fields, so its count is 0 in some iterations and it still enters
    every exchange (nobody hangs: the spawn joins).  Held, to the bars of item 5, against a one-process emulation of the same
    sharded run on the plain (materialised) path, which runs none of the counted kernels; the union of the ranks' own fields is
    the trained map."""
    world = 2
    ctxm = mp.spawn(_two_worker, args=(world, _free_port(), str(tmp_path), mode), nprocs=world, join=False)
    deadline = time.monotonic() + 240.0                 # the ranks under a time limit: never wait on a hung exchange
    while not ctxm.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctxm.processes:
                p.kill()
            raise AssertionError("a rank did not finish within its time limit")
    counts, losses, states = _two_emulated()
    N = TWO["N"]
    for rank in range(world):
        res = torch.load(os.path.join(tmp_path, f"two_{mode}{rank}.pt"))
        assert res["one_graph"] if mode == "peer" else res["two_graphs"]
        assert res["status"] == 0
        assert res["counts"] == counts[rank]
        assert res["step_dev"] == TWO["NIT"] == res["it_dev"]
        for i in range(TWO["NIT"]):
            for k in LOSS_KEYS:
                close(res["losses"][i][k], losses[rank][i][k], rtol=3e-4, atol=1e-6, equal_nan=True)
        own = torch.arange(rank, N, world)
        other = torch.arange(1 - rank, N, world)
        for k, v in res["state"].items():
            if k.startswith("param ") and v.is_floating_point():
                grad_close(v[own].float(), states[rank][k][own].float(), name=f"two ranks ({mode}) {k}")
            # a rank never touches the other rank's fields
            assert torch.equal(v[other], states[rank][k][other]), k
    r0, r1 = (torch.load(os.path.join(tmp_path, f"two_{mode}{r}.pt")) for r in range(world))
    assert 0 in r1["counts"] and max(r0["counts"]) > 0, (r0["counts"], r1["counts"])
    zero_it = r1["counts"].index(0)
    for k in LOSS_KEYS:       # the idle rank reports the global loss of that iteration, as rank 0 does
        torch.testing.assert_close(r1["losses"][zero_it][k], r0["losses"][zero_it][k], rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 11. unsupported
@pytest.mark.parametrize("cfg", ["neus", "triplane"])
def test_unsupported_configurations_fall_back_or_raise(cfg):
    if cfg == "neus":
        fkw, ckw = M1, dict(geometry_mode="neus", geometry_factor=5.0)
    else:
        fkw, ckw = dict(encoding="triplane", num_layers=1, resolution=16, num_components=32), {}
    N, T, R = 12, 6, 16
    sc = PartScene(N, 8, hidden=[1, 4, 7], seed=2)
    cur = torch.arange(0, N, 2, device=DEV)

    def renderer(params=None):
        r = make_renderer(fkw, dict(num_samples_coarse=4, num_samples_depth_guided=4, field_radius=1.0, **ckw), N, params)
        if params is None:
            from test_gpu_safety import _perturb
            _perturb(r, seed=4)
        r.set_field_poses(sc.positions, sc.quat)
        return r
    ra = renderer()
    rb = renderer({k: v.clone() for k, v in ra._model.all_fields_params.items()})
    assert ra.counted_step_unsupported() is not None
    ta = ra.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=1, iteration=0)
    tb = rb.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=1, iteration=0)
    with pytest.warns(RuntimeWarning, match="synchronises"):
        la = ra.optimization_iteration(ta, seed=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                      # one-time: the second call does not warn again
        la = ra.optimization_iteration(ta, seed=2)
    for _ in range(2):
        lb = rb.optimization_iteration(tb.materialize(), seed=2)
    assert_losses_equal({k: la[k] for k in LOSS_KEYS}, {k: lb[k] for k in LOSS_KEYS})
    assert_state_equal(state(ra), state(rb), what="warned fallback vs materialize()")
    with pytest.raises(RuntimeError, match="counted step"):
        ra.capture_training(*sc.args(cur, T, R), camera=sc.cam)
    with pytest.raises(RuntimeError, match="counted step"):
        ra.capture_iteration(ta)
    # under capture the fallback would synchronise: it raises before anything is launched
    y = torch.zeros(1, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y.add_(1.0)
        with pytest.raises(RuntimeError, match="cannot be captured"):
            ra.optimization_iteration(ta, seed=2)


# ------------------------------------------------------------------------------------------------ 12. capture_iteration(DeviceTarget)
def _small_scene():
    """TWO's sizes, the smallest of this module: 24 fields (the even ids hidden), T = 6 -> a capacity of 6 rows of 16 rays;
    every third field is current, so hidden fields are among the observed draws and padded rows exist"""
    return PartScene(24, 12, hidden=list(range(0, 24, 2)), seed=1), torch.arange(0, 24, 3, device=DEV)


@pytest.mark.parametrize("net", ["m1", "hash"])
def test_capture_iteration_on_a_device_target(net):
    """A DeviceTarget is captured as the counted step: 4 replays after the warm-up's two real updates are, bit for bit, six
    eager counted iterations on the same target."""
    T, R, SEED = TWO["T"], TWO["R"], 3
    sc, cur = _small_scene()
    ra, rb = sc.renderer(NETS[net]), sc.renderer(NETS[net])
    ta = ra.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=SEED, iteration=0)
    tb = rb.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=SEED, iteration=0)
    assert ta.ijs.shape[0] == 6 and 0 < int(ta.count) < 6, int(ta.count)
    replay = ra.capture_iteration(ta, seed=SEED)
    assert isinstance(replay.graph, torch.cuda.CUDAGraph)
    assert ra._step == 2
    la = lb = None
    for _ in range(4):
        la = replay()
    for _ in range(2 + 4):
        lb = rb.optimization_iteration(tb, seed=SEED)
    torch.cuda.synchronize()
    assert_losses_equal(losses_of(la), losses_of(lb))
    assert_state_equal(state(ra), state(rb), what="2 warm-up updates + 4 replays vs 6 eager counted iterations")
    assert ra._step == int(ra._step_dev) == 6 and rb._step == int(rb._step_dev) == 6


# ------------------------------------------------------------------------------------------------ 13. a refused capture
class _RefusedGraph:
    def __init__(self, *a, **kw):
        raise RuntimeError("refused for the test")


def _refused_worker(rank, store, out, net):
    """One rank with a gloo group (so that both functions take their two-graph form) whose graph objects cannot be
    constructed: a Python exception inside the functions' `try`, before any stream begins to capture."""
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", store=dist.FileStore(store, 1), rank=0, world_size=1)
    T, R, SEED = TWO["T"], TWO["R"], 3
    sc, cur = _small_scene()

    def renderer():
        r = sc.renderer(NETS[net])
        r.process_group = dist.group.WORLD
        return r
    real = torch.cuda.CUDAGraph
    torch.cuda.CUDAGraph = _RefusedGraph
    try:
        # capture_iteration(Target): the warm-up's two real updates stay, then plain launches
        ra, rb = renderer(), renderer()
        t = ra.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=SEED, iteration=0).materialize()
        assert t.ijs.shape[0] > 0
        with pytest.warns(RuntimeWarning, match="graph capture refused"):
            step = ra.capture_iteration(t, seed=SEED)
        assert step.graph is None and "refused for the test" in step.capture_error
        assert ra._step == 2 == int(ra._step_dev)
        la = lb = None
        for _ in range(3):
            la = step()
        for _ in range(2 + 3):
            lb = rb.optimization_iteration(t, seed=SEED)
        torch.cuda.synchronize()
        assert_losses_equal(losses_of(la), losses_of(lb))
        assert_state_equal(state(ra), state(rb), what="capture_iteration, refused: 2 + 3 plain iterations")
        assert ra._step == 5 == int(ra._step_dev)
        # capture_training: nothing trained by the warm-up, the iteration counter put back, then sampler + step per call
        ra, rb = renderer(), renderer()
        start = state(ra)
        with pytest.warns(RuntimeWarning, match="graph capture refused"):
            step = ra.capture_training(*sc.args(cur, T, R), seed=SEED, camera=sc.cam)
        assert step.graph is None and "refused for the test" in step.capture_error
        assert step.target is None
        assert ra._step == 0 and int(ra._target_iter_dev) == 0
        assert_state_equal(start, state(ra), what="capture_training, refused, trains nothing by itself")
        for i in range(3):
            la = step()
            assert isinstance(step.target, Rr.DeviceTarget)
            lb = rb.optimization_iteration(rb.sample_target_mv_device(*sc.args(cur, T, R), camera=sc.cam, seed=SEED, iteration=i),
                                           seed=SEED)
        torch.cuda.synchronize()
        assert_losses_equal(losses_of(la), losses_of(lb))
        assert_state_equal(state(ra), state(rb), what="capture_training, refused: 3 plain sampler + step calls")
        assert ra._step == 3 == int(ra._step_dev) and int(ra._target_iter_dev) == 3
    finally:
        torch.cuda.CUDAGraph = real
    with open(os.path.join(out, f"refused_{net}.ok"), "w") as fh:
        fh.write("ok")
    dist.destroy_process_group()


@pytest.mark.parametrize("net", ["m1", "hash"])
def test_refused_capture_falls_back_to_plain_launches(tmp_path, net):
    """capture_iteration and capture_training when the runtime refuses the two-graph capture: a RuntimeWarning, `.graph is
    None`, the message in `.capture_error`, `_step` as the warm-up left it, and calls that are plain iterations bit for bit
    (the assertions are the child's: _refused_worker)."""
    ctxm = mp.spawn(_refused_worker, args=(str(tmp_path / "store"), str(tmp_path), net), nprocs=1, join=False)
    deadline = time.monotonic() + 120.0
    while not ctxm.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctxm.processes:
                p.kill()
            raise AssertionError("the child did not finish within its time limit")
    assert os.path.exists(os.path.join(tmp_path, f"refused_{net}.ok"))
