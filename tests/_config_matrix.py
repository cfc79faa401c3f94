"""The table behind tests/test_gpu_config_matrix.py and tests/test_config_matrix_cpu.py: field configurations that
`check_field_cfg` (csrc/ngm_api.hip) lets through -- and a few it must not --, each with the outcome expected on the five
surfaces of the library, per `mlp_matmul` mode.  Plain data: no torch, no GPU.

Surfaces
  points    ops.field_eval under no_grad                   (ngm_field_eval_fwd -> k_field_points_fwd)
  autograd  ops.field_eval forward + backward              (... -> ngm_field_eval_bwd_stash / ngm_field_eval_bwd)
  step      the renderer's fused training step             (ngm_render_fwd + ngm_render_bwd[_adam])
  render    the fused render forward without gradients     (ngm_render_fwd -> k_render_fwd)
  knn       ops.field_eval_knn                             (ngm_field_eval_knn -> k_knn_eval)

Outcomes, per mode ("f32", "auto"; "bf16x3" where the entry is about the explicit mode)
  REFUSE            NgmError, code NGM_E_UNSUPPORTED, nothing observable changed
  fwd(mm)           runs; the library reports arithmetic `mm` ("f32" | "bf16x3") for that surface (ngm_debug_last_matmul)
  bwd(v_stash, v)   autograd: ngm_debug_last_bwd_variant with the activation stash allowed, and with
                    ops.FIELD_EVAL_STASH_MAX_BYTES = 0
  step(mm, v, fc)   fused step: arithmetic of the forward, backward variant, ngm_debug_last_comp_fused

Both halves are checked against the library without a GPU (tests/test_config_matrix_cpu.py): the forward columns -- shape,
arithmetic, refusal -- against plan_fwd through ngm_debug_plan_fwd, the backward ones against plan_mlp_bwd through
ngm_debug_plan_bwd (both csrc/ngm_api.hip), with TI / TH = ceil(dim / 16) and MI / MH = ceil(dim / 32):
  forward shape <MI,MH,L>     NGM_FWD_SHAPES (csrc/ngm_launch.h), shared by the three forward launchers: <2,2,2> <2,2,1> <1,1,1>
                              <1,1,2> <2,2,3>; bf16x3 only where ngm_fwd_split_takes: <2,2,L<=2>, Fourier / none, skip no (points /
                              knn: a preference; fused forward: `auto` resolves to it, explicit `bf16x3` elsewhere is refused by
                              the plan)
  variant 3  k_field_bwd_b3   stash kind 1 (TI = TH = 4, skip no, Fourier / NeRF / none, L <= 2) and mode != f32
  variant 5  k_hash_mlp_bwd   hash, L = 1, 17..32 features, <= 32 hidden units, mode != f32, fused step only
  variant 2  k_field_bwd16s   stash kind 1 and mode f32, fused step only
  variant 1  k_field_bwd16    (TI,TH,L) in {(4,4,1) (4,4,2) (2,2,1) (2,2,2) (3,3,1)}, skip no, not triplane
  variant 0  k_field_bwd      everything else at L <= 2
No backward kernel takes L = 3; nothing takes L = 4 or L = 3 at <= 32 units (refused by check_field_cfg itself).

The storage axis (tests/test_gpu_storage_matrix.py): STORAGE = 16-bit `weight_dtype`s; `storage16(entry, surface, mode)` is the
outcome with the weights stored in 16 bits.  Storage is no input of either plan (ngm_debug_plan_fwd / ngm_debug_plan_bwd take
none), so it is the entry's own outcome -- same arithmetic, backward variant and comp_fused, same NGM_E_UNSUPPORTED where fp32
refuses -- and what runs must equal the run on fp32 storage of the same (16-bit-representable) weights bit for bit.  One
exception: the triplane planes exist in fp32 only -- REFUSE_STORAGE: NotImplementedError from NeuralFieldSet, NGM_E_INVALID
("triplane encoding needs fp32 planes", check_params) at the ops level, on every surface, before any plan is made."""

REFUSE = "refuse"
REFUSE_STORAGE = "refuse-storage"       # 16-bit storage of an encoding that has fp32 tensors only: NGM_E_INVALID, nothing launched
STORAGE = ("bfloat16", "float16")
SURFACES = ("points", "autograd", "step", "render", "knn")
STEP_SHAPES = ((3, 37, 5, 2), (2, 33, 1, 1))            # (F, R, n_c, n_g) of the fused surfaces
FORWARD_SHAPES = ("<1,1,1>", "<1,1,2>", "<2,2,1>", "<2,2,2>", "<2,2,3>")
BWD_VARIANTS = (0, 1, 2, 3, 5)


def fwd(mm):
    return ("fwd", mm)


def bwd(with_stash, without):
    return ("bwd", with_stash, without)


def step(mm, variant, comp_fused):
    return ("step", mm, variant, comp_fused)


def runs(outcome):
    return outcome not in (REFUSE, REFUSE_STORAGE)


def _both(o):
    return dict(f32=o, auto=o)


def _entry(name, fkw, shape, points, autograd, step, render, knn, geometry="nrgbd", seed=0, bars=None):
    """bars: {surface: {tensor: bar}} -- a gradient bar other than the suite's, derived beside the entry (never from a kernel)"""
    return dict(name=name, fkw=fkw, shape=shape, geometry=geometry, seed=seed, bars=bars or {},
                points=points, autograd=autograd, step=step, render=render, knn=knn)


def _fourier(D, L, H=None, **kw):
    d = dict(encoding="fourier", dim_enc=D, num_layers=L, **kw)
    if H is not None:
        d["dim_hidden"] = H
    return d


def _hash(levels, L, log2=12, short=True):
    d = dict(encoding="permuto", num_layers=L, nr_levels=levels, log2_hashmap_size=log2, coarsest_scale=1.0, finest_scale=1e-4)
    if short:                       # every level coarse (scale >= 0.08) under hash_grad_close(sigmas=...): the strict bars
        d["finest_scale"] = 0.1
    return d


ALL_REFUSE = _both(REFUSE)
ALL_F32 = _both(fwd("f32"))
SPLIT = dict(f32=fwd("f32"), auto=fwd("bf16x3"))       # <2,2,L<=2>, Fourier / none, skip no

ENTRIES = [
    # ---------------------------------------------------------------------------------------------- depth, 64 -> 64 Fourier
    _entry("fourier64_L1", _fourier(64, 1), "<2,2,1>", SPLIT,
           dict(f32=bwd(1, 1), auto=bwd(3, 1)), dict(f32=step("f32", 2, 0), auto=step("bf16x3", 3, 1)), SPLIT, SPLIT),
    _entry("fourier64_L2", _fourier(64, 2), "<2,2,2>", dict(SPLIT, bf16x3=fwd("bf16x3")),
           dict(f32=bwd(1, 1), auto=bwd(3, 1)),
           dict(f32=step("f32", 2, 0), auto=step("bf16x3", 3, 1), bf16x3=step("bf16x3", 3, 1)),
           dict(SPLIT, bf16x3=fwd("bf16x3")), dict(SPLIT, bf16x3=fwd("bf16x3"))),
    # three hidden layers: forward only, fp32 MFMA whatever the mode asks for; the explicit split is refused by the fused forward
    _entry("fourier64_L3", _fourier(64, 3), "<2,2,3>", dict(ALL_F32, bf16x3=fwd("f32")), ALL_REFUSE,
           dict(ALL_REFUSE, bf16x3=REFUSE), dict(ALL_F32, bf16x3=REFUSE), dict(ALL_F32, bf16x3=fwd("f32"))),
    _entry("fourier64_L4", _fourier(64, 4), None, ALL_REFUSE, ALL_REFUSE, ALL_REFUSE, ALL_REFUSE, ALL_REFUSE),
    _entry("nerf10_L3", dict(encoding="nerf", num_octaves=10, num_layers=3), "<2,2,3>", ALL_F32, ALL_REFUSE, ALL_REFUSE, ALL_F32,
           ALL_F32),
    _entry("triplane64_L3", dict(encoding="triplane", num_components=64, resolution=16, tri_mode="sum", num_layers=3), "<2,2,3>",
           ALL_F32, ALL_REFUSE, ALL_REFUSE, ALL_F32, ALL_F32),
    _entry("fourier64_add_L3", _fourier(64, 3, skip_mode="add"), "<2,2,3>", ALL_F32, ALL_REFUSE, ALL_REFUSE, ALL_F32, ALL_F32),
    _entry("fourier64_concat_L3", _fourier(64, 3, skip_mode="concat"), "<2,2,3>", ALL_F32, ALL_REFUSE, ALL_REFUSE, ALL_F32,
           ALL_F32),
    _entry("fourier64_neus_L3", _fourier(64, 3), "<2,2,3>", ALL_F32, ALL_REFUSE, ALL_REFUSE, ALL_F32, ALL_F32, geometry="neus"),
    _entry("fourier32_L3", _fourier(32, 3), None, ALL_REFUSE, ALL_REFUSE, ALL_REFUSE, ALL_REFUSE, ALL_REFUSE),
    # ---------------------------------------------------------------------------------------------- widths, L = 1 and L = 2
    # one 16-tile: (TI,TH) = (1,1) has no k_field_bwd16 instance
    _entry("nerf2_12to16_L1", dict(encoding="nerf", num_octaves=2, num_layers=1, dim_hidden=16), "<1,1,1>", ALL_F32,
           _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("nerf2_12to16_L2", dict(encoding="nerf", num_octaves=2, num_layers=2, dim_hidden=16), "<1,1,2>", ALL_F32,
           _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("none_3to32_L1", dict(encoding="none", dim_enc=3, num_layers=1, dim_hidden=32), "<1,1,1>", ALL_F32,
           _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("none_3to32_L2", dict(encoding="none", dim_enc=3, num_layers=2, dim_hidden=32), "<1,1,2>", ALL_F32,
           _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    # 20 -> 32 and 32 -> 17 are both (TI,TH) = (2,2): k_field_bwd16<2,2,L>
    _entry("fourier_20to32_L1", _fourier(20, 1, 32), "<1,1,1>", ALL_F32, _both(bwd(1, 1)), _both(step("f32", 1, 0)), ALL_F32,
           ALL_F32),
    _entry("fourier_20to32_L2", _fourier(20, 2, 32), "<1,1,2>", ALL_F32, _both(bwd(1, 1)), _both(step("f32", 1, 0)), ALL_F32,
           ALL_F32),
    _entry("fourier_32to17_L1", _fourier(32, 1, 17), "<1,1,1>", ALL_F32, _both(bwd(1, 1)), _both(step("f32", 1, 0)), ALL_F32,
           ALL_F32),
    _entry("fourier_32to17_L2", _fourier(32, 2, 17), "<1,1,2>", ALL_F32, _both(bwd(1, 1)), _both(step("f32", 1, 0)), ALL_F32,
           ALL_F32),
    # 33 -> 48 and 48 -> 48 are both (3,3): k_field_bwd16<3,3,1> at L = 1, k_field_bwd at L = 2; the forward is the split's shape
    _entry("fourier_33to48_L1", _fourier(33, 1, 48), "<2,2,1>", SPLIT, _both(bwd(1, 1)),
           dict(f32=step("f32", 1, 0), auto=step("bf16x3", 1, 0)), SPLIT, SPLIT),
    _entry("fourier_33to48_L2", _fourier(33, 2, 48), "<2,2,2>", SPLIT, _both(bwd(0, 0)),
           dict(f32=step("f32", 0, 0), auto=step("bf16x3", 0, 0)), SPLIT, SPLIT),
    _entry("fourier_48to48_L1", _fourier(48, 1, 48), "<2,2,1>", SPLIT, _both(bwd(1, 1)),
           dict(f32=step("f32", 1, 0), auto=step("bf16x3", 1, 0)), SPLIT, SPLIT),
    _entry("fourier_48to48_L2", _fourier(48, 2, 48), "<2,2,2>", SPLIT, _both(bwd(0, 0)),
           dict(f32=step("f32", 0, 0), auto=step("bf16x3", 0, 0)), SPLIT, SPLIT),
    # 40 -> 64 is (3,4): mixed 16-tile classes inside one 32-pad class, no 16-sample-tile instance, no stash
    _entry("fourier_40to64_L1", _fourier(40, 1, 64), "<2,2,1>", SPLIT, _both(bwd(0, 0)),
           dict(f32=step("f32", 0, 0), auto=step("bf16x3", 0, 0)), SPLIT, SPLIT),
    _entry("fourier_40to64_L2", _fourier(40, 2, 64), "<2,2,2>", SPLIT, _both(bwd(0, 0)),
           dict(f32=step("f32", 0, 0), auto=step("bf16x3", 0, 0)), SPLIT, SPLIT),
    # 64 -> 49 and 61 -> 64 are (4,4): the stash kernels, with zero-padded rows / columns
    _entry("fourier_64to49_L1", _fourier(64, 1, 49), "<2,2,1>", SPLIT, dict(f32=bwd(1, 1), auto=bwd(3, 1)),
           dict(f32=step("f32", 2, 0), auto=step("bf16x3", 3, 1)), SPLIT, SPLIT),
    _entry("fourier_64to49_L2", _fourier(64, 2, 49), "<2,2,2>", SPLIT, dict(f32=bwd(1, 1), auto=bwd(3, 1)),
           dict(f32=step("f32", 2, 0), auto=step("bf16x3", 3, 1)), SPLIT, SPLIT),
    _entry("fourier_61to64_L1", _fourier(61, 1, 64), "<2,2,1>", SPLIT, dict(f32=bwd(1, 1), auto=bwd(3, 1)),
           dict(f32=step("f32", 2, 0), auto=step("bf16x3", 3, 1)), SPLIT, SPLIT),
    _entry("fourier_61to64_L2", _fourier(61, 2, 64), "<2,2,2>", SPLIT, dict(f32=bwd(1, 1), auto=bwd(3, 1)),
           dict(f32=step("f32", 2, 0), auto=step("bf16x3", 3, 1)), SPLIT, SPLIT),
    # ---------------------------------------------------------------------------------------------- hash ladders
    # <= 8 levels: one 16-tile, k_field_bwd<1,1,1> (k_hash_mlp_bwd needs dim_enc > 16)
    _entry("hash1_L1", _hash(1, 1), "<1,1,1>", ALL_F32, _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("hash4_T8_L1", _hash(4, 1, log2=8), "<1,1,1>", ALL_F32, _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("hash8_L1", _hash(8, 1), "<1,1,1>", ALL_F32, _both(bwd(0, 0)), _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    # 9 and 16 levels: (2,2); the fused step writes the encoding stash and runs k_hash_mlp_bwd with the compositing backward inside
    _entry("hash9_T8_L1", _hash(9, 1, log2=8), "<1,1,1>", ALL_F32, _both(bwd(1, 1)),
           dict(f32=step("f32", 1, 0), auto=step("f32", 5, 1)), ALL_F32, ALL_F32),
    # Default ladder (finest scale 1e-4) against the fp64 oracle in the point evaluation: 257 points per field and a random
    # d_out average nothing, and the fp32 position error (~1e-7, x 1e4 at the finest level) reaches the first layer's weight
    # gradient whole.  HASH_BARS["first_weight"] = 4e-3 was measured against the fp32 oracle, which shares that error.  The fp32
    # oracle against the fp64 oracle on this problem: 5.35e-3 (L = 1) and 4.97e-3 (L = 2) -> bar 4 x = 2.1e-2 / 2.0e-2
    # (derived; every other tensor, and the fused step's averaged gradients, stay on HASH_BARS).
    _entry("hash16_L1", _hash(16, 1, short=False), "<1,1,1>", ALL_F32, _both(bwd(1, 1)),
           dict(f32=step("f32", 1, 0), auto=step("f32", 5, 1)), ALL_F32, ALL_F32,
           bars=dict(autograd={"_linears.0.weight": 2.1e-2})),
    # two hidden layers: the stash is written, k_hash_mlp_bwd declines (L == 1), k_field_bwd16<2,2,2> reads it behind k_stash_bwd
    _entry("hash16_L2", _hash(16, 2, short=False), "<1,1,2>", ALL_F32, _both(bwd(1, 1)),
           dict(f32=step("f32", 1, 0), auto=step("f32", 1, 0)), ALL_F32, ALL_F32,
           bars=dict(autograd={"_linears.0.weight": 2.0e-2})),
    # ---------------------------------------------------------------------------------------------- skip connections, L = 2
    _entry("fourier_20to32_add_L2", _fourier(20, 2, 32, skip_mode="add"), "<1,1,2>", ALL_F32, _both(bwd(0, 0)),
           _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("fourier_20to32_concat_L2", _fourier(20, 2, 32, skip_mode="concat"), "<1,1,2>", ALL_F32, _both(bwd(0, 0)),
           _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("fourier_40to64_add_L2", _fourier(40, 2, 64, skip_mode="add"), "<2,2,2>", ALL_F32, _both(bwd(0, 0)),
           _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    _entry("fourier_40to64_concat_L2", _fourier(40, 2, 64, skip_mode="concat"), "<2,2,2>", ALL_F32, _both(bwd(0, 0)),
           _both(step("f32", 0, 0)), ALL_F32, ALL_F32),
    # ---------------------------------------------------------------------------------------------- explicit bf16x3 outside its shape
    _entry("fourier64_add_L2", _fourier(64, 2, skip_mode="add"), "<2,2,2>", dict(ALL_F32, bf16x3=fwd("f32")), _both(bwd(0, 0)),
           dict(_both(step("f32", 0, 0)), bf16x3=REFUSE), dict(ALL_F32, bf16x3=REFUSE), dict(ALL_F32, bf16x3=fwd("f32"))),
    _entry("fourier32_L2", _fourier(32, 2), "<1,1,2>", dict(ALL_F32, bf16x3=fwd("f32")), _both(bwd(1, 1)),
           dict(_both(step("f32", 1, 0)), bf16x3=REFUSE), dict(ALL_F32, bf16x3=REFUSE), dict(ALL_F32, bf16x3=fwd("f32"))),
]

BY_NAME = {e["name"]: e for e in ENTRIES}
NAMES = [e["name"] for e in ENTRIES]


def modes(entry, surface):
    return list(entry[surface])


def storage16(entry, surface, mode):
    """outcome of (entry, surface, mode) with the weights stored as either of STORAGE: see the module docstring"""
    if entry["fkw"]["encoding"] == "triplane":
        return REFUSE_STORAGE
    return entry[surface][mode]


def is_hash(entry):
    return entry["fkw"]["encoding"] == "permuto"


def hash_sigmas(entry):
    """the levels' scales (positional_encodings.py:50: geomspace), None for the default 16-level ladder hash_grad_close knows"""
    import numpy as np
    f = entry["fkw"]
    if f["nr_levels"] == 16 and f["finest_scale"] == 1e-4:
        return None
    return np.geomspace(f["coarsest_scale"], f["finest_scale"], num=f["nr_levels"])


def support_matrix():
    """rows of the README's support matrix: (entry, shape, {surface: 'runs' | 'refuses' | 'mixed'}) for mode auto"""
    rows = []
    for e in ENTRIES:
        rows.append((e["name"], e["shape"] or "-", {s: ("runs" if runs(e[s]["auto"]) else "refuses") for s in SURFACES}))
    return rows
