"""CPU-side checks of the live training iteration's boundary (include/ngm_hip.h ngm_target_sample_mv_live,
ngm_target_observed_fields, ngm_field_counts_add): symbols, struct layouts, argument validation before any launch, the host
restatement of the observed-field test against the reference's recorded result (G26) and against numpy.argsort, the
KeyframeStore bookkeeping against the reference's restated, and the margin condition every scene of
tests/test_gpu_live_iteration.py is chosen by.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngm_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _live_scenes as S  # noqa: E402
import _target_live_host as LH  # noqa: E402

NEW = ("ngm_target_sample_mv_live_workspace", "ngm_target_sample_mv_live", "ngm_target_observed_fields_workspace",
       "ngm_target_observed_fields", "ngm_field_counts_add")


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


def test_symbols_declared_and_exported_abi_unchanged(capi):
    head = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    L = capi.lib()
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", src), n
        assert n in capi.EXPORTED and hasattr(L, n), n
    assert int(re.search(r"#define\s+NGM_ABI_VERSION\s+(\d+)", head).group(1)) == 11 == L.ngm_abi_version()
    assert int(re.search(r"#define\s+NGM_OBSERVED_MAX_POINTS\s+(\d+)", src).group(1)) == capi.NGM_OBSERVED_MAX_POINTS
    # the planners size the workspaces without a device; bad sizes give -1
    W = L.ngm_target_sample_mv_live_workspace
    assert W(16, 40, 40, 12) == L.ngm_target_sample_mv_workspace(16, 40, 40, 12) > 0
    assert W(16, 0, 40, 12) == -1 and W(0, 40, 40, 12) == -1 and W(16, 40, 40, capi.NGM_TARGET_MAX_DRAW + 1) == -1
    assert L.ngm_target_observed_fields_workspace(480, 640) >= 480 * 640 * 8
    assert L.ngm_target_observed_fields_workspace(0, 640) == -1 and L.ngm_target_observed_fields_workspace(65536, 65536) == -1


def test_struct_layouts_match_header(capi, tmp_path):
    live = ("num_current", "num_frames", "num_observed", "num_random", "num_train_fields")
    obs = [f[0] for f in capi.ObservedFields._fields_ if f[0] != "reserved0"]
    fmt = " ".join(["%zu"] * (2 + len(live) + len(obs)))
    args = ",".join(["sizeof(ngm_target_live)"] + [f"offsetof(ngm_target_live,{f})" for f in live] +
                    ["sizeof(ngm_observed_fields)"] + [f"offsetof(ngm_observed_fields,{f})" for f in obs])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngm_hip.h"\n'
                   f'int main(){{printf("{fmt}\\n",{args});return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    TL, OF = capi.TargetLive, capi.ObservedFields
    assert sizes == ([C.sizeof(TL)] + [getattr(TL, f).offset for f in live] + [C.sizeof(OF)] + [getattr(OF, f).offset for f in obs])


def test_ops_registered_with_fake_shapes(capi):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from neural_graph_mapping_amd import ops
    op = torch.ops.ngm355.target_sample_mv_live
    with FakeTensorMode(allow_non_fake_inputs=True):
        dev = "cuda"
        out = op(torch.zeros(40, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                 torch.zeros(16, 4, 4, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(20, 24, 32, 4, device=dev),
                 torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(40, 3, device=dev), None, [1.0, 1.0, 0.0, 0.0], 1.0,
                 40, 12, 32, 0, 0, 3, 1)
        shapes = {k: tuple(v.shape) for k, v in zip(ops.TARGET_SAMPLE_MV_LIVE_OUT, out)}
        assert shapes["ijs"] == (12, 32, 2) and shapes["subset_observed"] == (6,) and shapes["subset_random"] == (12,)
        assert shapes["num_observed"] == (1,) and shapes["num_random"] == (1,)
        px, used = torch.ops.ngm355.target_observed_fields(
            torch.zeros(24, 32, 4, device=dev), torch.zeros(4, 4, device=dev), torch.zeros(70, 3, device=dev), None, None,
            torch.zeros(70, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), [1.0, 1.0, 0.0, 0.0],
            0.35, 70, 64, 0, 0)
        assert tuple(px.shape) == (64,) and px.dtype == torch.int64 and used.dtype == torch.int32


def test_live_plan(capi):
    P, Q = capi.target_sample_mv_live_plan, capi.target_sample_mv_plan
    assert P(40, 40, 12, 32) == (6, 12, 12)
    assert P(3, 40, 12, 32) == (3, 12, 12)
    assert P(40, 40, 12, 32, world_size=3, rank=2) == (6, 12, 12) and P(10, 10, 12, 8, world_size=3, rank=2) == (6, 10, 3)
    for N, T, W in ((40, 12, 1), (40, 12, 3), (10, 32, 2), (7, 7, 2)):
        for rank in range(W):
            for n in range(0, N + 1):                     # the capacity does not depend on the number of current fields
                assert Q(n, N, T, 8, W, rank)[2] == P(N, N, T, 8, W, rank)[2]
    with pytest.raises(ValueError, match="max_current"):
        P(0, 40, 12, 32)
    with pytest.raises(ValueError, match="max_current"):
        P(41, 40, 12, 32)


def test_validators_raise_before_launch(capi):
    from neural_graph_mapping_amd import ops
    i32 = lambda: torch.zeros(1, dtype=torch.int32)
    good = dict(current_field_ids=torch.zeros(12, dtype=torch.int64), current_count=i32(), c2ws=torch.zeros(6, 4, 4), num_frames=i32(),
                rgbd_store=torch.zeros(8, 24, 32, 4), frame_to_store=torch.zeros(6, dtype=torch.int64),
                field_positions=torch.zeros(12, 3))

    def call(**kw):
        a = dict(good)
        rest = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, radius=1.0, num_fields=12, num_train_fields=8, num_rays_per_field=16, iteration=0)
        for k in list(kw):
            (a if k in a else rest)[k] = kw[k]
        return ops.target_sample_mv_live(**a, **rest)
    with pytest.raises(TypeError, match="current_count"):
        call(current_count=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(TypeError, match="num_frames"):
        call(num_frames=3)
    with pytest.raises(TypeError, match="current_field_ids"):
        call(current_field_ids=torch.zeros(12, dtype=torch.int32))
    with pytest.raises(ValueError, match="max_current"):
        call(current_field_ids=torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_current"):
        call(current_field_ids=torch.zeros(13, dtype=torch.int64))
    with pytest.raises(ValueError, match="frame_to_store"):                    # capacity mismatch: poses for 6 frames, slots for 5
        call(frame_to_store=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="iteration_dev"):
        call(iteration=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # valid input, but no device tensors
        call()

    ogood = dict(rgbd=torch.zeros(24, 32, 4), c2w=torch.eye(4), field_positions=torch.zeros(12, 3))

    def obs(**kw):
        a = dict(ogood)
        rest = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, radius=0.35, num_fields=12, num_points=64, frame=0)
        for k in list(kw):
            (a if k in a else rest)[k] = kw[k]
        return ops.target_observed_fields(**a, **rest)
    with pytest.raises(TypeError, match="rgbd"):
        obs(rgbd=torch.zeros(24, 32, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match="c2w"):
        obs(c2w=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="num_points"):
        obs(num_points=0)
    with pytest.raises(ValueError, match="num_points"):
        obs(num_points=capi.NGM_OBSERVED_MAX_POINTS + 1)
    with pytest.raises(ValueError, match="subset_in"):
        obs(subset_in=torch.zeros(63, dtype=torch.int64))
    with pytest.raises(ValueError, match="ids_out"):                           # capacity mismatch: 11 slots for 12 fields
        obs(ids_out=torch.zeros(11, dtype=torch.int64))
    with pytest.raises(TypeError, match="count_out"):
        obs(count_out=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="frame_dev"):
        obs(frame=None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        obs()
    with pytest.raises(TypeError, match="int64"):
        ops.field_counts_add(torch.zeros(4, dtype=torch.int32), None, torch.zeros(12, dtype=torch.int64), 12)
    with pytest.raises(ValueError, match="training_iterations"):
        ops.field_counts_add(torch.zeros(4, dtype=torch.int64), None, torch.zeros(11, dtype=torch.int64), 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.field_counts_add(torch.zeros(4, dtype=torch.int64), None, torch.zeros(12, dtype=torch.int64), 12)


def test_renderer_signatures():
    from neural_graph_mapping_amd import renderer as Rr
    import inspect
    for fn in (Rr.NeuralGraphRenderer.sample_target_mv_device, Rr.NeuralGraphRenderer.capture_training):
        p = inspect.signature(fn).parameters
        for k in ("current_count", "num_frames"):
            assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None
    assert "min_iterations" in inspect.signature(Rr.NeuralGraphRenderer.get_field_ids).parameters


# ---------------------------------------------------------------------------------------------- host restatement
def test_k_smallest_equals_argsort():
    g = np.random.RandomState(0)
    for n, k in ((3072, 500), (768, 64), (40, 64), (1, 1), (5000, 1), (300, 299), (300, 300)):
        hi = g.randint(0, 2 ** 32, size=n, dtype=np.uint64)
        if n >= 768:
            hi[: n // 2] = hi[0]                         # equal random words: the select must go on into the index digits
        keys = (hi << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        want = np.sort(keys[np.argsort(keys, kind="stable")[:k]])
        assert np.array_equal(LH.k_smallest_radix(keys, k), want), (n, k)
    img = S.frame(24, 32, 0)
    keys, pix = LH.pixel_keys(img[..., 3], 7, 3)
    assert len(keys) == int((img[..., 3] != 0).sum()) and np.array_equal(keys & np.uint64(0xFFFFFFFF), pix.astype(np.uint64))
    px = LH.draw_pixels(img[..., 3], 64, 7, 3)
    assert np.array_equal(px, np.sort(pix[np.argsort(keys, kind="stable")[:64]]))
    assert not np.array_equal(px, LH.draw_pixels(img[..., 3], 64, 7, 4)) and not np.array_equal(px, LH.draw_pixels(img[..., 3], 64, 8, 3))


def test_host_restatement_reproduces_g26():
    """the reference's _get_observed_fields on its recorded draws (tests/golden/make_golden_observed.py)"""
    import scene
    g = np.load(os.path.join(ROOT, "tests", "golden", "g26_observed_fields.npz"))
    img = scene.sv_frame(int(g["frame_seed"])).numpy()
    cam = (scene.SV_FX, scene.SV_FY, scene.SV_CX, scene.SV_CY)
    px = g["d_pixels"].astype(np.int64)
    assert len(px) == int(g["num_points"]) == len(np.unique(px)) and (img[..., 3].reshape(-1)[px] != 0).all()
    for dt in (np.float32, np.float64):
        ids = LH.observed_from_pixels(img, g["c2w"], g["positions"], float(g["field_radius"]), px, *cam, dt=dt)
        assert np.array_equal(ids, g["o_field_ids"]), dt
    _, mb, ms = LH.observed_from_pixels(img, g["c2w"], g["positions"], float(g["field_radius"]), px, *cam, dt=np.float64, margins=True)
    assert mb >= 1e-3 and ms >= 1e-3
    assert 0 < len(g["o_field_ids"]) < len(g["positions"])


def test_margin_condition_of_the_gpu_scenes():
    """A condition on the scenes, not a tolerance: in float64, for every field, |max over the chosen points of (r^2 - d^2)|
    >= 1e-3 r^2 and every AABB comparison clears its bound by 1e-3 r -- some hundred times the float32 rounding of d^2 at
    these coordinates (<= 6 m: 36 x 2^-23 x a few operations ~ 1e-5 against r^2 ~ 0.12).  The GPU comparisons then exclude
    nothing, and float32 and float64 agree on every scene."""
    seen = []
    cases = [(n, S.observe_case(n), S.SEED, S.FRAME) for n in S.OBSERVE_CASES]
    pos = S.field_map(S.GRAPH_MAP_SEED)
    cases += [(f"graph frame {i}", dict(S.graph_frame(i), positions=pos, num_points=S.GRAPH_POINTS), S.SEED, i)
              for i in range(len(S.GRAPH_FRAMES))]
    for name, c, seed, frame in cases:
        ids, mb, ms = S.margins(c["rgbd"], c["c2w"], c["positions"], c["num_points"], seed, frame)
        assert mb >= 1e-3 and ms >= 1e-3, (name, mb, ms)
        H, W = c["rgbd"].shape[:2]
        px, ids32 = LH.observed_fields(c["rgbd"], c["c2w"], c["positions"], S.RADIUS, c["num_points"], seed, frame,
                                       *S.camera_params(H, W))
        assert np.array_equal(ids, ids32), name
        valid = int((c["rgbd"][..., 3] != 0).sum())
        assert len(px) == min(c["num_points"], valid) == len(np.unique(px)), name
        seen.append(len(ids))
    n = dict(zip([c[0] for c in cases], seen))
    assert n["all_zero"] == 0 and n["graph frame 1"] == 0 and n["48x64"] > 6
    assert all(n[f"graph frame {i}"] > 6 for i in (0, 2, 3)) and len({n[f"graph frame {i}"] for i in range(4)}) >= 3
    # the map: some fields behind the camera, some outside the points' AABB, and they are what is left out
    c = S.observe_case("48x64")
    ids, _, _ = S.margins(c["rgbd"], c["c2w"], c["positions"], 500, S.SEED, S.FRAME)
    assert not set(ids) & set(range(20)) and S.NUM_FIELDS == 70


# ---------------------------------------------------------------------------------------------- KeyframeStore
def test_keyframe_store_matches_reference_bookkeeping():
    from neural_graph_mapping_amd.keyframes import KeyframeStore
    H, W, cap = 4, 5, 4
    g = torch.Generator().manual_seed(0)
    img = lambda: torch.rand(H, W, 4, generator=g)
    pose = lambda: torch.rand(4, 4, generator=g)
    st, ref = KeyframeStore(cap, H, W, device="cpu"), LH.ReferenceKeyframes(cap)
    images = {}

    def check():
        n = st.count
        ncid, c2w = ref.frame_cid_to_ncid, ref.c_c2w
        assert int(st.num_frames) == n == len(ncid)
        assert st.frame_cid_to_ncid[:n].tolist() == list(ncid)
        for k in range(n):
            assert torch.equal(st.c_c2w[k], c2w[k]), k
            assert torch.equal(st.nc_rgbd[ncid[k]], images[ref.images[ncid[k]]]), k
        assert int(st.frame_cid_to_ncid.min()) >= 0 and int(st.frame_cid_to_ncid.max()) < cap      # padding stays in range
        assert bool(torch.isfinite(st.c_c2w).all())
    ptrs = [t.data_ptr() for t in (st.nc_rgbd, st.c_c2w, st.frame_cid_to_ncid, st.num_frames)]
    # frame 0: a current frame
    images["f0"], p0 = img(), pose()
    st.set_current(images["f0"], p0, frame_id=0)
    ref.update(current=(0, "f0", p0))
    check()
    # frames 1, 2: each becomes a keyframe
    for f in (1, 2):
        images[f"f{f}"], p = img(), pose()
        st.set_current(images[f"f{f}"], p, frame_id=f)
        st.add_keyframe(images[f"f{f}"], f)
        ref.update(current=(f, f"f{f}", p), keyframe=(f, f"f{f}", p))
        check()
    assert st.num_keyframes == 2 and st.count == 3
    # frame 3: tracking lost -- slot 0 leaves the list, the keyframes move up
    st.clear_current()
    ref.update(current=None)
    check()
    assert st.count == 2 and st.frame_cid_to_ncid[:2].tolist() == [1, 2]
    # frame 4: tracked again, another keyframe; the pose graph moves all keyframes
    images["f4"], p4 = img(), pose()
    st.set_current(images["f4"], p4, frame_id=4)
    st.add_keyframe(images["f4"], 4)
    ref.update(current=(4, "f4", p4), keyframe=(4, "f4", p4))
    check()
    moved = torch.rand(3, 4, 4, generator=g)
    st.set_keyframe_poses(moved)
    for fid, p in zip(st.frame_ids, moved):
        ref.poses[fid] = p
    images["f5"], p5 = img(), pose()
    st.set_current(images["f5"], p5, frame_id=5)
    ref.update(current=(5, "f5", p5))
    check()
    # the store is full: both raise, as the reference does
    with pytest.raises(ValueError, match="Maximum number of keyframes reached"):
        st.add_keyframe(images["f5"], 5)
    with pytest.raises(ValueError, match="Maximum number of keyframes reached"):
        ref.update(current=(5, "f5", p5), keyframe=(5, "f5", p5))
    assert ptrs == [t.data_ptr() for t in (st.nc_rgbd, st.c_c2w, st.frame_cid_to_ncid, st.num_frames)]    # all in place
    assert st.num_frames.dtype == torch.int32 and st.frame_cid_to_ncid.dtype == torch.int64
    # keyframes_only: no current-frame slot, keyframes from slot 0
    ko, rko = KeyframeStore(2, H, W, device="cpu", keyframes_only=True), LH.ReferenceKeyframes(2, keyframes_only=True)
    with pytest.raises(ValueError, match="current-frame slot"):
        ko.set_current(images["f0"], p0)
    for f in (0, 1):
        ko.add_keyframe(images[f"f{f}"], f, c2w=p0 + f)
        rko.update(keyframe=(f, f"f{f}", p0 + f))
        assert ko.frame_cid_to_ncid[:ko.count].tolist() == list(rko.frame_cid_to_ncid) and int(ko.num_frames) == f + 1
        assert all(torch.equal(ko.c_c2w[k], rko.c_c2w[k]) for k in range(ko.count))
    with pytest.raises(ValueError, match="Maximum number of keyframes reached"):
        ko.add_keyframe(images["f0"], 2, c2w=p0)
