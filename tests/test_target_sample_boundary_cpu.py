"""The refusals of the device sampler at the C boundary (include/ngm_hip.h ngm_target_sample_mv, ngm_target_sample_mv_live
and their *_workspace planners): a table of malformed records goes through both entry points by ctypes, and every row pins
the returned status and the whole ngm_last_error() text.  Every refusal comes before anything is launched, so the non-NULL
pointers are arbitrary non-zero integers and no row passes all the checks.  No GPU."""
import ctypes as C
import os

import pytest

PTR = 0x1000                         # a non-NULL pointer that is never dereferenced
MAX_DRAW = 2048
OK, INVALID, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def _records(capi, live):
    """A record set that passes every check of the entry point (never sent as it is): 12 fields, 5 current (the live
    maximum), T = 8 -> 4 observed + 4 random (live maxima: 4 and 8), one rank, capacity 8, 6 keyframes of 48 x 64."""
    def pointers(rec):
        for name, tp in rec._fields_:
            if tp is capi.f32p:
                setattr(rec, name, C.cast(PTR, tp))
            elif tp is C.c_void_p:
                setattr(rec, name, PTR)
        return rec
    kf, s, out, lv = (pointers(T()) for T in (capi.Keyframes, capi.TargetSample, capi.TargetOut, capi.TargetLive))
    kf.num_frames, kf.height, kf.width, kf.fx, kf.fy = 6, 48, 64, 1.0, 1.0
    s.num_current, s.num_fields, s.num_observed, s.num_random = 5, 12, 4, 8 if live else 4
    s.num_rays, s.capacity, s.world_size, s.rank, s.radius, s.seed, s.iteration = 16, 8, 1, 0, 1.0, 0, 0
    lv.num_train_fields = 8
    return dict(kf=kf, s=s, out=out, live=lv)


def _call(capi, live, edits):
    """Apply `edits` ({"s.num_rays": 0, "out": None, "ws": None, "ws_short": 1, ...}) to the good records and call."""
    L = capi.lib()
    r = _records(capi, live)
    ws, short = PTR, 0
    for key, val in edits.items():
        if key == "ws":
            ws = val
        elif key == "ws_short":
            short = val
        elif "." in key:
            rec, field = key.split(".")
            setattr(r[rec], field, val)                          # None: NULL
        else:
            r[key] = val
    s, kf = r["s"], r["kf"]
    plan = (L.ngm_target_sample_mv_grow_workspace if live == "grow" else L.ngm_target_sample_mv_live_workspace if live
            else L.ngm_target_sample_mv_workspace)
    need = plan(kf.num_frames if kf is not None else 1, s.num_current if s is not None else 1,
                s.num_fields if s is not None else 1, min(max(s.capacity, 0), MAX_DRAW) if s is not None else 0)
    need = max(need, 1)
    ref = lambda x: None if x is None else C.byref(x)
    if live == "grow":                                           # the live records over reserved rows + the device field count
        rc = L.ngm_target_sample_mv_grow(ref(kf), ref(s), ref(r["live"]), r.get("num_fields_dev", PTR), ref(r["out"]), ws, need - short, None)
    elif live:
        rc = L.ngm_target_sample_mv_live(ref(kf), ref(s), ref(r["live"]), ref(r["out"]), ws, need - short, None)
    else:
        rc = L.ngm_target_sample_mv(ref(kf), ref(s), ref(r["out"]), ws, need - short, None)
    return rc, L.ngm_last_error().decode()


S, LV, GR = "ngm_target_sample_mv: ", "ngm_target_sample_mv_live: ", "ngm_target_sample_mv_grow: "
NULL_ARRAY = "NULL array (iteration < 0 needs iteration_dev)"
BIG = dict([("s.num_fields", 5000), ("s.num_current", 3000)])

# (id, live, edits, status, message) -- the messages are the library's, written out
ROWS = [
    # ---- ngm_target_sample_mv ----
    ("kf_null", False, {"kf": None}, INVALID, "target sampler: NULL keyframe argument"),
    ("kf_null_c2ws", False, {"kf.c2ws": None}, INVALID, "target sampler: NULL keyframe argument"),
    ("kf_empty", False, {"kf.num_frames": 0}, INVALID, "target sampler: empty keyframe set"),
    ("s_null", False, {"s": None}, INVALID, S + "NULL argument"),
    ("out_null", False, {"out": None}, INVALID, S + "NULL argument"),
    ("num_current_negative", False, {"s.num_current": -1}, INVALID, S + "bad sizes (num_rays >= 1, 0 <= rank < world_size)"),
    ("num_rays_0", False, {"s.num_rays": 0}, INVALID, S + "bad sizes (num_rays >= 1, 0 <= rank < world_size)"),
    ("rank_ge_world", False, {"s.rank": 1}, INVALID, S + "bad sizes (num_rays >= 1, 0 <= rank < world_size)"),
    ("observed_gt_current", False, {"s.num_observed": 6}, INVALID,
     S + "num_observed <= num_current and num_random <= num_fields - num_observed"),
    ("random_gt_rest", False, {"s.num_random": 9}, INVALID,
     S + "num_observed <= num_current and num_random <= num_fields - num_observed"),
    ("max_draw", False, dict(BIG, **{"s.num_observed": 1000, "s.num_random": 1049, "s.capacity": 2049}), UNSUPPORTED,
     S + "more than NGM_TARGET_MAX_DRAW fields drawn"),
    ("capacity_wrong", False, {"s.capacity": 7}, INVALID,
     S + "capacity must be min(num_observed + num_random, fields of this rank)"),
    ("capacity_not_sharded", False, {"s.world_size": 2}, INVALID,                 # rank 0 of 2 owns 6 of the 12 fields
     S + "capacity must be min(num_observed + num_random, fields of this rank)"),
    ("null_current_field_ids", False, {"s.current_field_ids": None}, INVALID, S + NULL_ARRAY),
    ("null_field_positions", False, {"s.field_positions": None}, INVALID, S + NULL_ARRAY),
    ("null_count", False, {"s.count": None}, INVALID, S + NULL_ARRAY),
    ("null_field_ids", False, {"s.field_ids": None}, INVALID, S + NULL_ARRAY),
    ("null_subset_observed", False, {"s.subset_observed": None}, INVALID, S + NULL_ARRAY),
    ("null_subset_random", False, {"s.subset_random": None}, INVALID, S + NULL_ARRAY),
    ("null_offsets", False, {"s.offsets": None}, INVALID, S + NULL_ARRAY),
    ("null_frame_cids", False, {"s.frame_cids": None}, INVALID, S + NULL_ARRAY),
    ("null_u_xy", False, {"s.u_xy": None}, INVALID, S + NULL_ARRAY),
    ("iteration_dev_needed", False, {"s.iteration": -1, "s.iteration_dev": None}, INVALID, S + NULL_ARRAY),
    ("null_out_ijs", False, {"out.ijs": None}, INVALID, S + "NULL output array"),
    ("null_out_term_mask", False, {"out.term_mask": None}, INVALID, S + "NULL output array"),
    ("rows_past_int32", False, {"s.num_rays": 1 << 28}, UNSUPPORTED, S + "capacity x num_rays >= 2^31"),
    ("ws_null", False, {"ws": None}, WORKSPACE, S + "workspace too small"),
    ("ws_one_byte_short", False, {"ws_short": 1}, WORKSPACE, S + "workspace too small"),
    # two rules at once: the earlier check answers
    ("order_sizes_before_counts", False, {"s.num_rays": 0, "s.num_observed": 6}, INVALID,
     S + "bad sizes (num_rays >= 1, 0 <= rank < world_size)"),
    ("order_capacity_before_arrays", False, {"s.capacity": 7, "s.count": None}, INVALID,
     S + "capacity must be min(num_observed + num_random, fields of this rank)"),
    ("order_outputs_before_workspace", False, {"out.gt": None, "ws": None}, INVALID, S + "NULL output array"),
    # ---- ngm_target_sample_mv_live ----
    ("kf_null", True, {"kf": None}, INVALID, "target sampler: NULL keyframe argument"),
    ("kf_empty", True, {"kf.height": 0}, INVALID, "target sampler: empty keyframe set"),
    ("s_null", True, {"s": None}, INVALID, LV + "NULL argument"),
    ("out_null", True, {"out": None}, INVALID, LV + "NULL argument"),
    ("live_null", True, {"live": None}, INVALID, LV + "NULL argument"),
    ("max_current_0", True, {"s.num_current": 0, "s.num_observed": 0}, INVALID,
     LV + "bad sizes (max_current >= 1, num_rays >= 1, 0 <= rank < world_size)"),
    ("num_rays_0", True, {"s.num_rays": 0}, INVALID,
     LV + "bad sizes (max_current >= 1, num_rays >= 1, 0 <= rank < world_size)"),
    ("rank_ge_world", True, {"s.rank": 1}, INVALID,
     LV + "bad sizes (max_current >= 1, num_rays >= 1, 0 <= rank < world_size)"),
    ("num_train_fields_negative", True, {"live.num_train_fields": -1}, INVALID,
     LV + "bad sizes (max_current >= 1, num_rays >= 1, 0 <= rank < world_size)"),
    ("max_current_gt_fields", True, {"s.num_current": 13}, INVALID, LV + "max_current > num_fields"),
    ("observed_gt_current", True, {"s.num_observed": 6}, INVALID,
     LV + "num_observed / num_random must be their maxima min(T / 2, max_current) / min(T, num_fields)"),
    ("observed_below_maximum", True, {"s.num_observed": 3}, INVALID,
     LV + "num_observed / num_random must be their maxima min(T / 2, max_current) / min(T, num_fields)"),
    ("random_below_maximum", True, {"s.num_random": 4}, INVALID,                  # the static call's n_rand
     LV + "num_observed / num_random must be their maxima min(T / 2, max_current) / min(T, num_fields)"),
    ("random_gt_rest", True, {"s.num_random": 9}, INVALID,
     LV + "num_observed / num_random must be their maxima min(T / 2, max_current) / min(T, num_fields)"),
    ("max_draw", True, {"s.num_fields": 5000, "s.num_current": 2000, "live.num_train_fields": 3000, "s.num_observed": 1500,
                        "s.num_random": 3000, "s.capacity": 2048}, UNSUPPORTED, LV + "more than NGM_TARGET_MAX_DRAW fields drawn"),
    ("capacity_wrong", True, {"s.capacity": 7}, INVALID, LV + "capacity must be min(min(T, num_fields), fields of this rank)"),
    ("null_live_num_current", True, {"live.num_current": None}, INVALID, LV + "NULL device count"),
    ("null_live_num_frames", True, {"live.num_frames": None}, INVALID, LV + "NULL device count"),
    ("null_live_num_observed", True, {"live.num_observed": None}, INVALID, LV + "NULL device count"),
    ("null_live_num_random", True, {"live.num_random": None}, INVALID, LV + "NULL device count"),
    ("null_current_field_ids", True, {"s.current_field_ids": None}, INVALID, LV + NULL_ARRAY),
    ("null_field_positions", True, {"s.field_positions": None}, INVALID, LV + NULL_ARRAY),
    ("null_count", True, {"s.count": None}, INVALID, LV + NULL_ARRAY),
    ("null_field_ids", True, {"s.field_ids": None}, INVALID, LV + NULL_ARRAY),
    ("null_subset_observed", True, {"s.subset_observed": None}, INVALID, LV + NULL_ARRAY),
    ("null_subset_random", True, {"s.subset_random": None}, INVALID, LV + NULL_ARRAY),
    ("null_offsets", True, {"s.offsets": None}, INVALID, LV + NULL_ARRAY),
    ("null_frame_cids", True, {"s.frame_cids": None}, INVALID, LV + NULL_ARRAY),
    ("null_u_xy", True, {"s.u_xy": None}, INVALID, LV + NULL_ARRAY),
    ("iteration_dev_needed", True, {"s.iteration": -1, "s.iteration_dev": None}, INVALID, LV + NULL_ARRAY),
    ("null_out_rgbds", True, {"out.rgbds": None}, INVALID, LV + "NULL output array"),
    ("null_out_rgb_mask", True, {"out.rgb_mask": None}, INVALID, LV + "NULL output array"),
    ("rows_past_int32", True, {"s.num_rays": 1 << 28}, UNSUPPORTED, LV + "capacity x num_rays >= 2^31"),
    ("ws_null", True, {"ws": None}, WORKSPACE, LV + "workspace too small"),
    ("ws_one_byte_short", True, {"ws_short": 1}, WORKSPACE, LV + "workspace too small"),
    ("order_fields_before_maxima", True, {"s.num_current": 13, "s.num_observed": 3}, INVALID, LV + "max_current > num_fields"),
    ("order_capacity_before_counts", True, {"s.capacity": 7, "live.num_frames": None}, INVALID,
     LV + "capacity must be min(min(T, num_fields), fields of this rank)"),
    ("order_counts_before_arrays", True, {"live.num_current": None, "s.count": None}, INVALID, LV + "NULL device count"),
    ("order_outputs_before_workspace", True, {"out.far": None, "ws_short": 1}, INVALID, LV + "NULL output array"),
    # ---- ngm_target_sample_mv_grow: the live entry point's checks behind its own ----
    ("num_fields_dev_null", "grow", {"num_fields_dev": None}, INVALID, GR + "NULL num_fields_dev"),
    ("ws_null", "grow", {"ws": None}, WORKSPACE, GR + "workspace too small"),
    ("ws_one_byte_short", "grow", {"ws_short": 1}, WORKSPACE, GR + "workspace too small"),
    ("order_outputs_before_workspace", "grow", {"out.far": None, "ws_short": 1}, INVALID, GR + "NULL output array"),
]


@pytest.mark.parametrize("live,edits,status,message", [r[1:] for r in ROWS],
                         ids=[("grow-" if r[1] == "grow" else "live-" if r[1] else "static-") + r[0] for r in ROWS])
def test_sampler_refuses_before_any_launch(capi, live, edits, status, message):
    rc, err = _call(capi, live, edits)
    assert (rc, err) == (status, message)


def test_empty_subsets_may_be_null(capi):
    """subset_observed / subset_random are needed only for a non-zero size: with 0 observed (static: 0 current fields and a
    NULL current_field_ids too) the call goes on to the next refusal, here the workspace"""
    rc, err = _call(capi, False, {"s.num_current": 0, "s.current_field_ids": None, "s.num_observed": 0, "s.num_random": 8,
                                  "s.subset_observed": None, "ws": None})
    assert (rc, err) == (WORKSPACE, S + "workspace too small")
    # live: T = 1 -> no observed field; current_field_ids is needed whatever the counts
    base = {"live.num_train_fields": 1, "s.num_observed": 0, "s.num_random": 1, "s.capacity": 1, "s.subset_observed": None}
    assert _call(capi, True, dict(base, ws=None)) == (WORKSPACE, LV + "workspace too small")
    assert _call(capi, True, dict(base, **{"s.current_field_ids": None})) == (INVALID, LV + NULL_ARRAY)


def test_workspace_planners_refuse_with_minus_one(capi):
    L = capi.lib()
    for fn in (L.ngm_target_sample_mv_workspace, L.ngm_target_sample_mv_live_workspace):
        assert fn(6, 5, 12, 8) > 0
        assert fn(0, 5, 12, 8) == -1                       # no frame
        assert fn(6, -1, 12, 8) == -1                      # negative number of current fields
        assert fn(6, 5, -1, 8) == -1                       # negative number of fields
        assert fn(6, 5, 12, -1) == -1 and fn(6, 5, 12, MAX_DRAW + 1) == -1          # capacity outside [0, NGM_TARGET_MAX_DRAW]
        assert fn(6, 5, 12, 0) > 0 and fn(6, 5, 12, MAX_DRAW) > 0
    # the same layout behind both
    assert L.ngm_target_sample_mv_workspace(6, 5, 12, 8) == L.ngm_target_sample_mv_live_workspace(6, 5, 12, 8)
    # the one difference: no current field is a size of the static sampler, not a maximum of the live one
    assert L.ngm_target_sample_mv_workspace(6, 0, 12, 8) > 0
    assert L.ngm_target_sample_mv_live_workspace(6, 0, 12, 8) == -1
