"""-m gpu: covering a keyframe's depth with new fields (include/ngm_hip.h ngm_cover_depth; ops.cover_depth;
NeuralGraphRenderer.cover_depth / extend_map) against the fixture recorded from the real reference and the fp64 host mirror
tests/_cover_host.py, whose checker tests/test_cover_depth_cpu.py shows to reject seven single faults.  Raw C calls run with
new_positions, counts and the workspace between guard bands, the workspace pre-filled with 0xFF bytes.  Shapes: 48 x 64 and a
ragged 37 x 53 (a last wave that is partly empty), radius 1.0 and 0.25, world points on both sides of the origin on every axis.
The set of cells is exact wherever the mirror finds no decision inside its rounding band; positions are bitwise."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import DEV  # noqa: E402
import _cover_host as CH  # noqa: E402
import _growing_map_host as G  # noqa: E402
import _live_scenes as S  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import ops  # noqa: E402
from test_gpu_growing_map import SMALL, assert_states_equal, camera, dev, renderer, state  # noqa: E402
from test_gpu_image_metrics import PATTERN, Banded  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g30_cover_depth.npz")
RADII = (1.0, 0.25)


def c_cover(depth, c2w, K_, shift, radius, positions=None, field_ids=None, num_active=None, max_new=512, calls=1, stream=None,
            cell=None):
    """ngm_cover_depth through the C ABI.  depth: (H, W), or (H, W, 4) read in place with pixel_stride 4.  new_positions and
    counts between guard bands and pre-filled with the pattern, the workspace between guard bands and pre-filled with 0xFF.
    -> (new_positions (max_new, 3) float32 as the call left it, counts (4,)) per call (a list for calls > 1)"""
    L = K.lib()
    img = dev(np.asarray(depth, np.float32))
    h, w = img.shape[:2]
    stride = 1 if img.dim() == 2 else 4
    dptr = img.data_ptr() + (0 if stride == 1 else 12)
    pose, sh = dev(np.asarray(c2w, np.float32)), dev(np.asarray(shift, np.float32))
    pos = None if positions is None else dev(np.asarray(positions, np.float32).reshape(-1, 3))
    ids = None if field_ids is None else dev(np.asarray(field_ids, np.int64))
    rows = 0 if pos is None else pos.shape[0]
    na = (rows if ids is None else ids.shape[0]) if num_active is None else num_active
    wsb = L.ngm_cover_depth_workspace(h, w, na, max_new)
    assert wsb > 0
    ws = Banded(wsb, 0xFF)
    fx, fy, cx, cy = K_
    res = []
    for _ in range(calls):
        out, cnt = Banded(12 * max_new, PATTERN), Banded(16, PATTERN)
        a = K.CoverDepthArgs(dptr, pose.data_ptr(), sh.data_ptr(), None if pos is None or rows == 0 else pos.data_ptr(),
                             None if ids is None or na == 0 else ids.data_ptr(), out.ptr, cnt.ptr, stride, rows, na, h, w, max_new,
                             fx, fy, cx, cy, radius, CH.cell_of(radius) if cell is None else cell)
        st = ops._stream() if stream is None else stream.cuda_stream
        K.check(L.ngm_cover_depth(C.byref(a), ws.ptr, wsb, st), "ngm_cover_depth")
        torch.cuda.synchronize()
        out.check(), cnt.check(), ws.check()
        res.append((out.payload(torch.float32).view(max_new, 3).cpu().numpy().copy(), cnt.payload(torch.int32).cpu().numpy().copy()))
    return res[0] if calls == 1 else res


def untouched(rows):
    """rows of new_positions the call must not have written still hold the pattern"""
    return bool((np.ascontiguousarray(rows).view(np.uint8) == PATTERN).all())


def run_case(case, **kw):
    return c_cover(case["depth"], case["c2w"], case["K"], case["shift"], case["radius"], case.get("positions"), case.get("field_ids"), **kw)


def classify(case):
    return CH.classify(case["depth"], case["c2w"], case["K"], case["shift"], case["radius"], case.get("positions"), case.get("field_ids"))


def held(case, pos, cnt):
    """a status-0 result against the mirror; rows past num_new untouched"""
    n = int(cnt[0])
    CH.check(classify(case), pos[:n], cnt)
    assert untouched(pos[n:])


@pytest.fixture(scope="module")
def g30():
    return dict(np.load(FIXTURE))


def ragged(seed, radius):
    return CH.sweep_case(seed, radius, 37, 53)


# ------------------------------------------------------------------------------------------------ 1. the fixture
def test_fixture_from_the_reference(g30):
    Kx, n0, n1, r = tuple(g30["intrinsics"]), int(g30["num0"]), int(g30["num1"]), float(g30["radius"])
    calls = [(dict(depth=g30["depth0"], c2w=g30["c2w0"], K=Kx, shift=g30["shift0"], radius=r), g30["positions"][:n0]),
             (dict(depth=g30["depth1"], c2w=g30["c2w1"], K=Kx, shift=g30["shift1"], radius=r, positions=g30["positions"][:n0]),
              g30["positions"][n0:n1])]
    for case, want in calls:
        pos, cnt = run_case(case)
        _, want_counts = CH.cover_fp32(case["depth"], case["c2w"], Kx, case["shift"], r, case.get("positions"))
        assert cnt.tolist() == want_counts                                   # no pixel of the fixture is ambiguous: exact
        assert pos[:len(want)].tobytes() == want.tobytes() and untouched(pos[len(want):])
        # the op: the same rows, zeros behind them
        p2, c2 = ops.cover_depth(dev(case["depth"]), dev(case["c2w"]), dev(case["shift"]),
                                 None if "positions" not in case else dev(case["positions"]), r, *Kx, 64)
        assert c2.cpu().numpy().tolist() == want_counts and p2.shape == (64, 3)
        assert p2[:len(want)].cpu().numpy().tobytes() == want.tobytes() and not bool(p2[len(want):].any())


# ------------------------------------------------------------------------------------------------ 2. no active fields
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", [(48, 64), (37, 53)])
def test_without_active_fields_every_touched_cell_is_new(shape, radius):
    depth, c2w, Kx = CH.box_scene(53, *shape)                                # this camera sees a corner: floor and two walls
    p = CH.world_points(depth, c2w, Kx)[1]
    assert (p.min(0) < -0.2).all() and (p.max(0) > 0.2).all()                # both sides of the origin on every axis
    case = dict(depth=depth, c2w=c2w, K=Kx, shift=(np.float32([0.3, 0.7, 0.1]) * np.float32(CH.cell_of(radius))), radius=radius)
    pos, cnt = run_case(case)
    held(case, pos, cnt)
    assert cnt[2] == cnt[3] > 0
    # an empty table with a count of zero is the same call
    pos2, cnt2 = run_case(dict(case, positions=np.zeros((0, 3), np.float32)))
    assert pos2.tobytes() == pos.tobytes() and cnt2.tolist() == cnt.tolist()


# ------------------------------------------------------------------------------------------------ 3. everything covered
def test_every_point_covered_writes_nothing():
    depth, c2w, Kx = CH.box_scene(6, 37, 53)
    centres = CH.world_points(depth, c2w, Kx)[1].astype(np.float32)           # a field on every point
    for radius in RADII:
        pos, cnt = c_cover(depth, c2w, Kx, np.float32([0.2, 0.1, 0.05]), radius, centres)
        assert cnt.tolist() == [0, 0, 0, len(centres)] and untouched(pos)


# ------------------------------------------------------------------------------------------------ 4. occupied, not covering
@pytest.mark.parametrize("radius", RADII)
def test_a_cell_with_an_active_centre_is_not_emitted(radius):
    """The centre sits near one corner of cell (2, -3, 1), five pixels see points near the opposite corner, 1.5 r away: the
    points are uncovered, their cell is occupied, nothing is new (rm.py:303-311).  Without the field the cell is emitted."""
    cell, H, W = CH.cell_of(radius), 37, 53
    shift = np.float32([0.11, 0.05, 0.2]) * np.float32(cell)
    ijk = np.array([2, -3, 1])
    lo = ijk * cell - shift.astype(np.float64)
    centre = (lo + 0.12 * cell).astype(np.float32)
    target, d0 = lo + 0.88 * cell, 0.25
    Kx = (60.0, 60.0, 26.0, 18.0)
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = target + [0, 0, d0]
    depth = np.zeros((H, W), np.float32)
    for di, dj in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
        depth[18 + di, 26 + dj] = d0
    case = dict(depth=depth, c2w=c2w, K=Kx, shift=shift, radius=radius, positions=centre[None])
    cls = classify(case)
    assert cls["ambiguous_pixels"] == 0 and cls["ambiguous_centres"] == 0 and not cls["required"] and not cls["optional"]
    pos, cnt = run_case(case)
    assert cnt.tolist() == [0, 0, 5, 5] and untouched(pos)
    pos, cnt = run_case(dict(case, positions=None))
    assert cnt.tolist() == [1, 0, 5, 5] and pos[:1].tobytes() == CH.emit([ijk], shift, cell).tobytes() and untouched(pos[1:])


# ------------------------------------------------------------------------------------------------ 5. padded id lists
def test_padded_and_out_of_range_ids_are_skipped():
    case = ragged(3, 0.25)
    ids, rows = case["field_ids"], len(case["positions"])
    assert len(ids) > 4
    padded = np.full(2 * len(ids) + 3, -1, np.int64)
    padded[1:2 * len(ids):2] = ids
    padded[0], padded[2], padded[-1] = rows, rows + 7, 1 << 40
    a, b = run_case(case), run_case(dict(case, field_ids=padded))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[1][0] > 0
    held(case, *a)
    # the compacted list as a table of its own, no ids
    c = run_case(dict(case, positions=case["positions"][ids], field_ids=None))
    assert a[0].tobytes() == c[0].tobytes() and a[1].tolist() == c[1].tolist()
    # only the first num_active rows of a table count
    d = c_cover(case["depth"], case["c2w"], case["K"], case["shift"], 0.25, case["positions"], num_active=3)
    e = run_case(dict(case, positions=case["positions"][:3], field_ids=None))
    assert d[0].tobytes() == e[0].tobytes() and d[1].tolist() == e[1].tolist()


# ------------------------------------------------------------------------------------------------ 6. the depth channel in place
def test_pixel_stride_four_reads_the_depth_channel():
    case = ragged(4, 1.0)
    rgbd = np.random.default_rng(0).random((37, 53, 4)).astype(np.float32) + 9.0      # colours that would be wrong depths
    rgbd[..., 3] = case["depth"]
    a, b = run_case(case), run_case(dict(case, depth=rgbd))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tolist() == b[1].tolist() and a[1][0] > 0
    p, c = ops.cover_depth(dev(rgbd), dev(case["c2w"]), dev(case["shift"]), dev(case["positions"]), 1.0, *case["K"], 512,
                           field_ids=dev(case["field_ids"]))
    assert c.cpu().numpy().tolist() == a[1].tolist() and p[:a[1][0]].cpu().numpy().tobytes() == a[0][:a[1][0]].tobytes()


# ------------------------------------------------------------------------------------------------ 7. pixels and poses that do not count
def test_zero_and_non_finite_depths_and_a_lost_pose_are_skipped():
    case = ragged(7, 1.0)
    depth = case["depth"].copy()
    g = np.random.default_rng(1)
    for value in (np.inf, -np.inf, np.nan, 0.0, -0.0):
        depth[g.random(depth.shape) < 0.05] = value
    case = dict(case, depth=depth)
    pos, cnt = run_case(case)
    held(case, pos, cnt)
    assert cnt[3] == int((np.isfinite(depth) & (depth != 0)).sum()) < depth.size * 0.85
    lost = case["c2w"].copy()
    lost[1, 3] = np.nan
    pos, cnt = run_case(dict(case, c2w=lost))
    assert cnt.tolist() == [0, 0, 0, 0] and untouched(pos)


# ------------------------------------------------------------------------------------------------ 8. all or nothing
def test_overflow_reports_the_need_and_writes_nothing():
    case = ragged(8, 0.25)
    pos, cnt = run_case(case)
    need = int(cnt[0])
    assert need > 3
    p1, c1 = run_case(case, max_new=need - 1)
    assert c1.tolist() == [need, 1, cnt[2], cnt[3]] and untouched(p1)
    p2, c2 = run_case(case, max_new=need)
    assert c2.tolist() == cnt.tolist() and p2.tobytes() == pos[:need].tobytes()
    p3, c3 = run_case(case, max_new=1)
    assert c3.tolist() == [need, 1, cnt[2], cnt[3]] and untouched(p3)


# ------------------------------------------------------------------------------------------------ 9. repeatable
def test_calls_repeat_bit_for_bit_on_any_stream():
    case = CH.sweep_case(9, 0.25)
    (p1, c1), (p2, c2) = run_case(case, calls=2)                              # the second on the first's stale workspace
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    p3, c3 = run_case(case, stream=side)
    assert c1[0] > 8
    assert p1.tobytes() == p2.tobytes() == p3.tobytes() and c1.tolist() == c2.tolist() == c3.tolist()


# ------------------------------------------------------------------------------------------------ 10. the sweep
def test_sweep_of_box_room_scenes():
    """40 seeds at each radius: every required cell present, no forbidden one, positions bitwise, counts held.  So that the
    optional cells cannot hide a failure they must be at most 1 % of all cells over the sweep (the mirror alone decides that)."""
    required = optional = emitted = 0
    for radius in RADII:
        for seed in range(40):
            case = CH.sweep_case(seed, radius)
            cls = classify(case)
            pos, cnt = run_case(case)
            n = int(cnt[0])
            CH.check(cls, pos[:n], cnt)
            assert untouched(pos[n:])
            required, optional, emitted = required + len(cls["required"]), optional + len(cls["optional"]), emitted + n
    share = optional / (required + optional)
    print(f"cover sweep: {required} required cells, {optional} optional ({100 * share:.2f} %), {emitted} emitted")
    assert required > 2000 and share <= 0.01


# ------------------------------------------------------------------------------------------------ far from the origin
def test_far_from_the_origin():
    """beyond |index| = 2^16 the kernel tries every active field (the 27-cell search is exact only below); beyond 2^20 the
    index does not pack: status 2, nothing written"""
    case = CH.sweep_case(2, 1.0, 37, 53)
    off = np.float32([90000.0, -120000.0, 80000.0])
    c2w = case["c2w"].copy()
    c2w[:3, 3] += off
    far = dict(case, c2w=c2w, positions=case["positions"] + off)
    pos, cnt = run_case(far)
    held(far, pos, cnt)
    assert 0 < cnt[2] < cnt[3]                                               # some pixels covered, some not, out there
    c2w = case["c2w"].copy()
    c2w[0, 3] += np.float32(2.0e6)
    pos, cnt = run_case(dict(case, c2w=c2w))
    assert cnt[:2].tolist() == [0, 2] and untouched(pos)


# ------------------------------------------------------------------------------------------------ 11. / 12. extend_map
KF_ID = 500


def keyframe():
    """a new keyframe of the growing-map scene: a 10 x 12 patch of depth 3 m in front of pose(102), no depth elsewhere"""
    rgbd = S.frame(S.GRAPH_H, S.GRAPH_W, 777, zero_frac=2.0)
    rgbd[7:17, 10:22, 3] = 3.0
    return rgbd, S.pose(102)


def expected_new(positions, rgbd, c2w, shift):
    Kx = S.camera_params(S.GRAPH_H, S.GRAPH_W)
    case = dict(depth=rgbd[..., 3], c2w=c2w, K=Kx, shift=shift, radius=S.RADIUS, positions=positions)
    cls = classify(case)
    assert cls["ambiguous_pixels"] == 0 and cls["ambiguous_centres"] == 0
    return CH.cover_fp32(rgbd[..., 3], c2w, Kx, shift, S.RADIUS, positions)[0]


def test_extend_map_under_a_live_graph():
    F = G.GrowFrames(device=DEV)
    cam = camera(F.H, F.W)
    rgbd, c2w = keyframe()
    shift = np.float32([0.13, 0.21, 0.05])
    want = expected_new(F.positions[:G.START], rgbd, c2w, shift)
    num_new, cap = len(want), G.START + len(want) + 2
    assert 2 <= num_new <= 40
    r = renderer(F.positions[:G.START], SMALL, trained=True)
    r.track_training_iterations = True
    r.reserve_fields(cap)
    st = F.store()
    ids_buf = torch.full((cap,), -1, dtype=torch.int64, device=DEV)
    cnt_buf = torch.zeros(1, dtype=torch.int32, device=DEV)
    pose_buf = torch.eye(4, device=DEV)

    def observe(f):
        pose_buf.copy_(dev(F.frames[f]["c2w"]))
        r.observed_fields_device(st.nc_rgbd[0], pose_buf, num_points=S.GRAPH_POINTS, seed=S.SEED, frame=f, out=(ids_buf, cnt_buf), camera=cam)
    F.advance(st, 0)
    observe(0)
    step = r.capture_training(ids_buf, st.c_c2w, st.nc_rgbd, st.frame_cid_to_ncid, G.T, G.R, seed=G.SEED, camera=cam,
                              current_count=cnt_buf, num_frames=st.num_frames)
    for _ in range(3):
        step()
    before = state(r, True)
    # the keyframe arrives: the store takes it, the map is extended from the store's slot, read in place
    st.add_keyframe(dev(rgbd), KF_ID, c2w=dev(c2w))
    slot = st.slot_of(KF_ID)
    new_ids = r.extend_map(st.nc_rgbd[slot], KF_ID, dev(c2w), store=st, shift=dev(shift), camera=cam)
    assert new_ids == range(G.START, G.START + num_new)
    md, rs = r._global_map_dict, r._reserved
    assert md["num"] == G.START + num_new == int(rs["num_fields_dev"])
    assert md["positions"][G.START:].cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(md["orientations"][G.START:].cpu(), torch.tensor([1.0, 0, 0, 0]).repeat(num_new, 1))
    assert md["kf_ids"][G.START:].tolist() == [KF_ID] * num_new and r._anchor["slot"][G.START:md["num"]].tolist() == [slot] * num_new
    assert r._anchor["slot"][:G.START].tolist() == [-1] * G.START and r._anchor["slot"][md["num"]:].tolist() == [-1] * 2
    proto = r._model._prototype_field.state_dict()
    after = state(r, True)
    for k, v in after.items():
        assert torch.equal(v[:G.START], before[k]), k                         # the fields that were there: not a bit moved
        if k.startswith("exp_avg"):
            assert not bool(v[G.START:].any()), k
        if k.startswith("param "):
            assert torch.equal(v[G.START:], proto[k[6:]].to(v.device).expand_as(v[G.START:])), k
    assert not bool(md["training_iterations"][G.START:].any())
    # the same graph goes on and trains the new fields
    graph = step.graph
    F.advance(st, 2)
    observe(2)
    for _ in range(20):
        step()
    assert step.graph is graph
    ti = md["training_iterations"]
    assert int(ti[G.START:md["num"]].max()) >= 1, ti[G.START:].tolist()
    # a keyframe that needs more fields than the reservation has left: refused, not a bit changes, the graph replays
    torch.cuda.synchronize()
    full = state(r, True)
    extra = {k: v.clone() for k, v in (("kf", r._anchor["kf_ids"]), ("slot", r._anchor["slot"]), ("nfd", rs["num_fields_dev"]), ("ti", ti))}
    st.add_keyframe(dev(F.frames[3]["rgbd"]), 3, c2w=dev(F.frames[3]["c2w"]))
    with pytest.raises(ValueError, match=r"new fields needed but 2 reserved rows are free"):
        r.extend_map(st.nc_rgbd[st.slot_of(3)], 3, dev(F.frames[3]["c2w"]), store=st, camera=cam)
    assert_states_equal(state(r, True), full, "a refused extend_map")
    for k, v in (("kf", r._anchor["kf_ids"]), ("slot", r._anchor["slot"]), ("nfd", rs["num_fields_dev"]), ("ti", ti)):
        assert torch.equal(v, extra[k]), k
    assert r._global_map_dict["num"] == G.START + num_new
    with pytest.raises(ValueError, match="not a keyframe"):
        r.extend_map(dev(rgbd), 12345, dev(c2w), store=st, camera=cam)
    step()
    # nothing to add: an empty range, nothing touched (the keyframe's own fields now cover it; same shift: its cells are occupied)
    assert r.extend_map(dev(rgbd), KF_ID, dev(c2w), store=st, shift=dev(shift), camera=cam) == range(md["num"], md["num"])


def test_extend_map_without_a_reservation_gives_the_same_fields():
    F = G.GrowFrames(device=DEV)
    cam = camera(F.H, F.W)
    rgbd, c2w = keyframe()
    shift = np.float32([0.13, 0.21, 0.05])
    want = expected_new(F.positions[:G.START], rgbd, c2w, shift)
    r = renderer(F.positions[:G.START], SMALL, trained=True)
    st = F.store()
    st.add_keyframe(dev(rgbd), KF_ID, c2w=dev(c2w))
    before = state(r, True)
    new_ids = r.extend_map(dev(rgbd[..., 3].copy()), KF_ID, dev(c2w), store=st, shift=dev(shift), camera=cam)
    n = G.START + len(want)
    assert new_ids == range(G.START, n) and r._global_map_dict["num"] == n
    assert r._global_map_dict["positions"][G.START:].cpu().numpy().tobytes() == want.tobytes()
    assert r._global_map_dict["kf_ids"].tolist() == [-1] * G.START + [KF_ID] * len(want)
    after = state(r, True)
    for k, v in after.items():
        assert v.shape[0] == n and torch.equal(v[:G.START], before[k]), k
    # the draw of the shift is the reference's: torch's generator, on the device, uniform in [0, cell)
    gen = torch.Generator(device=DEV).manual_seed(4)
    cell = ops.cover_cell(S.RADIUS)
    drawn = torch.empty(3, device=DEV).uniform_(0.0, cell, generator=gen)
    gen.manual_seed(4)
    p_a, c_a = r.cover_depth(dev(rgbd), dev(c2w), generator=gen, camera=cam, max_new=64)
    p_b, c_b = r.cover_depth(dev(rgbd), dev(c2w), shift=drawn, camera=cam, max_new=64)
    assert torch.equal(p_a, p_b) and torch.equal(c_a, c_b) and int(c_a[1]) == 0
    # active_field_ids: only those fields cover and occupy
    ids = torch.arange(0, n, 2, device=DEV)
    p_c, c_c = r.cover_depth(dev(rgbd), dev(c2w), active_field_ids=ids, shift=drawn, camera=cam, max_new=64)
    case = dict(depth=rgbd[..., 3], c2w=c2w, K=S.camera_params(S.GRAPH_H, S.GRAPH_W), shift=drawn.cpu().numpy(), radius=S.RADIUS,
                positions=r._global_map_dict["positions"].cpu().numpy(), field_ids=ids.cpu().numpy())
    CH.check(classify(case), p_c[:int(c_c[0])].cpu().numpy(), c_c.cpu().numpy())
