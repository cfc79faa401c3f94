"""Fields anchored to keyframes on the GPU (include/ngm_hip.h ngm_fields_repose; NeuralGraphRenderer.anchor_fields /
remove_keyframe / repose_fields; KeyframeStore.remove_keyframe): the kernel through the C ABI against the float64 restatement
of the reference (tests/_repose_host.py) with the float32 restatement's own error as the yardstick, the "not touched" rules
bit for bit, guard bands, the device field count, advance_prev, determinism -- and one captured training graph that keeps
replaying across a loop closure and across the release and reuse of a keyframe slot."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gpu_common import DEV  # noqa: E402
import _growing_map_host as G  # noqa: E402
import _live_scenes as S  # noqa: E402
import _repose_host as RH  # noqa: E402
from neural_graph_mapping_amd import _capi as K  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from test_gpu_growing_map import LOSS_KEYS, M1, assert_losses_equal, camera, dev, identity_quat, renderer  # noqa: E402

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
CAP, START, T, R = G.CAPACITY, G.START, G.T, G.R


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def repose_call(pos, quat, anchor, prev, new, num_fields=None, num_fields_dev=None, advance=0):
    """ngm_fields_repose through the C ABI on device tensors, in place"""
    a = K.FieldsReposeArgs(C.cast(pos.data_ptr(), K.f32p), C.cast(quat.data_ptr(), K.f32p), anchor.data_ptr(),
                           C.cast(prev.data_ptr(), K.f32p), C.cast(new.data_ptr(), K.f32p),
                           None if num_fields_dev is None else num_fields_dev.data_ptr(),
                           pos.shape[0] if num_fields is None else num_fields, prev.shape[0], advance, 0)
    K.check(K.lib().ngm_fields_repose(C.byref(a), torch.cuda.current_stream().cuda_stream), "ngm_fields_repose")


def make_case(F, NP, seed=0):
    """F fields over NP keyframe poses (numpy float32).  With 7 poses: 0 leaves a rotation by pi about x, 1 lands on a
    rotation by pi about y, 2 carries a translation of magnitude 50, 3 has a NaN in its new pose, 4 does not move (bitwise
    equal rows), 5 lands on a rotation by pi about z, 6 gets a small correction.  With one pose: a general pose that lands
    on a rotation by pi about y.  Anchors repeat; from 4 fields on one is -1 and two are out of range; quaternions are not
    unit."""
    rng = np.random.default_rng(1000 * F + NP + seed)
    rr = lambda: RH.rot(rng.normal(size=3), rng.uniform(0.2, 2.9))
    tt = lambda s=3.0: rng.uniform(-s, s, 3)
    if NP == 1:
        prev, new = [RH.pose(rr(), tt())], [RH.pose(RH.rot(1, np.pi), tt())]
    else:
        t50 = rng.normal(size=3)
        t50 *= 50.0 / np.linalg.norm(t50)
        prev = [RH.pose(RH.rot(0, np.pi), tt()), RH.pose(rr(), tt()), RH.pose(rr(), t50), RH.pose(rr(), tt()), RH.pose(rr(), tt()),
                RH.pose(rr(), tt()), RH.pose(rr(), tt())]
        new = [RH.pose(rr(), tt()), RH.pose(RH.rot(1, np.pi), tt()), RH.pose(rr(), t50 + tt(0.5)), RH.pose(rr(), tt()), prev[4].copy(),
               RH.pose(RH.rot(2, np.pi), tt()), RH.pose(RH.rot(rng.normal(size=3), 0.02) @ prev[6][:3, :3], prev[6][:3, 3] + tt(0.05))]
        new[3][1, 2] = np.nan
    prev, new = np.stack(prev).astype(np.float32), np.stack(new).astype(np.float32)
    anchor = (np.arange(F) % NP).astype(np.int32)             # every pose is used as soon as F >= NP, anchors repeat beyond
    rng.shuffle(anchor)
    if F >= 4:
        anchor[1], anchor[2], anchor[F - 1] = -1, NP, NP + 1000
    pos = rng.uniform(-4, 4, (F, 3)).astype(np.float32)
    if NP > 2:
        pos[anchor == 2] += prev[2, :3, 3]                    # the fields of the far keyframe stand near it
    quat = rng.normal(size=(F, 4))
    quat *= (rng.uniform(0.5, 2.0, (F, 1)) / np.linalg.norm(quat, axis=-1, keepdims=True))
    return pos, quat.astype(np.float32), anchor, prev, new


def check_against_fp64(got_pos, got_quat, pos, quat, anchor, prev, new, num=None, what=""):
    """The bar: the kernel's worst error in positions, and in quaternions up to sign, against the float64 restatement is at
    most 4 x the worst error of the float32 restatement on the same inputs (the margin tests/test_gpu_adam.py gives a
    different association order); every row the rules leave alone is bit for bit the input."""
    p64, q64, touched = RH.repose(pos, quat, anchor, prev, new, np.float64, num)
    p32, q32, _ = RH.repose(pos, quat, anchor, prev, new, np.float32, num)
    ref_p, ref_q = RH.errors(p32[touched], q32[touched], p64[touched], q64[touched])
    got_p, got_q = RH.errors(got_pos[touched], got_quat[touched], p64[touched], q64[touched])
    print(f"{what}: {int(touched.sum())} of {len(anchor)} rows moved; kernel {got_p:.3e} / {got_q:.3e}, "
          f"float32 restatement {ref_p:.3e} / {ref_q:.3e}")
    assert np.array_equal(bits(got_pos[~touched]), bits(pos[~touched])), what
    assert np.array_equal(bits(got_quat[~touched]), bits(quat[~touched])), what
    assert np.isfinite(got_pos).all() and np.isfinite(got_quat).all()
    assert got_p <= 4 * ref_p and got_q <= 4 * ref_q, (what, got_p, ref_p, got_q, ref_q)
    return touched


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("NP", [1, 7])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 200])
def test_kernel_against_fp64_restatement(F, NP):
    pos, quat, anchor, prev, new = make_case(F, NP)
    d = [dev(x) for x in (pos, quat, anchor, prev, new)]
    repose_call(*d)
    torch.cuda.synchronize()
    touched = check_against_fp64(d[0].cpu().numpy(), d[1].cpu().numpy(), pos, quat, anchor, prev, new, what=f"F={F} NP={NP}")
    assert torch.equal(d[3].cpu(), torch.from_numpy(prev)) and np.array_equal(bits(d[4].cpu().numpy()), bits(new))   # advance_prev = 0
    if F >= 63:
        assert touched.any() and not touched.all()
        if NP == 7:
            assert not touched[np.isin(anchor, (3, 4))].any() and touched[np.isin(anchor, (0, 1, 2, 5, 6))].all()
            moved = np.abs(d[0].cpu().numpy() - pos).max(-1)
            assert (moved[np.isin(anchor, (0, 1, 2, 5))] > 1e-3).all()


def test_kernel_against_reference_fixture():
    """G25, from the real reference in float32: the bound of tests/test_repose_cpu.py (64 eps32 M), and the 4 x bar"""
    g = np.load(os.path.join(HERE, "golden", "g25_repose.npz"))
    pos, quat, prev, new = g["positions"], g["orientations"], g["prev_kf2ws"], g["new_kf2ws"]
    anchor = g["kf_ids"].astype(np.int32)
    d = [dev(x) for x in (pos, quat, anchor, prev, new)]
    repose_call(*d)
    got_p, got_q = d[0].cpu().numpy(), d[1].cpu().numpy()
    touched = check_against_fp64(got_p, got_q, pos, quat, anchor, prev, new, what="G25")
    m_pos = max(1.0, float(np.abs(pos).max()), float(np.abs(prev[:, :3, 3]).max()), float(np.abs(new[:, :3, 3]).max()))
    m_quat = float(np.linalg.norm(quat, axis=-1).max())
    ep, eq = RH.errors(got_p[touched], got_q[touched], g["out_positions"][touched], g["out_orientations"][touched])
    print(f"G25 against the reference: {ep:.3e} / {eq:.3e} (bounds {64 * EPS32 * m_pos:.3e} / {64 * EPS32 * m_quat:.3e})")
    assert ep <= 64 * EPS32 * m_pos and eq <= 64 * EPS32 * m_quat


def test_guard_bands():
    """4 KiB bands around all five buffers and the device count: 65 of 70 rows in force, prev advanced"""
    from test_gpu_safety import guard_bands
    pos, quat, anchor, prev, new = make_case(70, 7)

    def banded(a):
        t = torch.zeros(tuple(a.shape), dtype=torch.from_numpy(a).dtype, device=DEV)
        t.copy_(torch.from_numpy(a))
        return t
    with guard_bands() as bands:
        d = [banded(x) for x in (pos, quat, anchor, prev, new)]
        nfd = torch.zeros(1, dtype=torch.int32, device=DEV)
        nfd.fill_(65)
        repose_call(*d, num_fields_dev=nfd, advance=1)
        repose_call(*d[:3], d[3][:1], d[4][:1], advance=1)               # one pose: every other anchor is out of range
        torch.cuda.synchronize()
        n = bands.check()
    assert n >= 6
    check_against_fp64(d[0].cpu().numpy(), d[1].cpu().numpy(), pos, quat, anchor, prev, new, num=65, what="banded")


def test_device_field_count_bounds_the_rows():
    pos, quat, anchor, prev, new = make_case(65, 7)
    for count, want in ((40, 40), (0, 0), (-3, 0), (65, 65), (900, 65)):
        d = [dev(x) for x in (pos, quat, anchor, prev, new)]
        nfd = torch.tensor([count], dtype=torch.int32, device=DEV)
        repose_call(*d, num_fields_dev=nfd)
        got_p, got_q = d[0].cpu().numpy(), d[1].cpu().numpy()
        assert np.array_equal(bits(got_p[want:]), bits(pos[want:])) and np.array_equal(bits(got_q[want:]), bits(quat[want:])), count
        h = [dev(x) for x in (pos, quat, anchor, prev, new)]
        repose_call(*h, num_fields=want)                                    # the host count gives the same bits
        assert torch.equal(d[0], h[0]) and torch.equal(d[1], h[1])
        check_against_fp64(got_p, got_q, pos, quat, anchor, prev, new, num=want, what=f"count {count}")


def test_advance_prev_and_determinism():
    pos, quat, anchor, prev, new = make_case(200, 7)
    d = [dev(x) for x in (pos, quat, anchor, prev, new)]
    e = [t.clone() for t in d]
    repose_call(*d, advance=1)
    repose_call(*e, advance=1)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(d[:2], e[:2]))    # two calls, cloned inputs
    # prev := new for every finite row; the row of the lost pose keeps the pose its fields still stand at
    got_prev = d[3].cpu().numpy()
    assert np.array_equal(bits(got_prev[[0, 1, 2, 4, 5, 6]]), bits(new[[0, 1, 2, 4, 5, 6]])) and np.array_equal(bits(got_prev[3]), bits(prev[3]))
    once = [t.clone() for t in d[:2]]
    repose_call(*d, advance=1)                                              # the same new poses again: not one bit changes
    assert torch.equal(d[0].view(torch.int32), once[0].view(torch.int32)) and torch.equal(d[1].view(torch.int32), once[1].view(torch.int32))
    # without the advance the second call moves the fields again
    f = [dev(x) for x in (pos, quat, anchor, prev, new)]
    repose_call(*f, advance=0)
    assert torch.equal(f[0], once[0]) and torch.equal(f[3].cpu(), torch.from_numpy(prev))
    repose_call(*f, advance=0)
    touched = RH.touched_rows(anchor, prev, new)
    again = (f[0] != once[0]).any(-1).cpu().numpy()
    assert again[touched].all() and not again[~touched].any()


# ------------------------------------------------------------------------------------------------ 2. under the live graph
class LiveRun:
    """Renderer A: reserved at CAP with START fields, anchored, ONE capture_training graph.  Renderer B: its unreserved twin
    on the eager sampler and iteration (the twins of tests/test_gpu_growing_map.py over G.GrowFrames)."""

    def __init__(self, store_capacity=6):
        self.F = F = G.GrowFrames(device=DEV)
        self.cam = camera(F.H, F.W)
        self.ra = renderer(F.positions[:START], M1, None, trained=True)
        self.rb = renderer(F.positions[:START], M1, None, trained=True)
        self.ra.reserve_fields(CAP)
        self.st = F.store(store_capacity)
        self.ids_buf = torch.full((CAP,), -1, dtype=torch.int64, device=DEV)
        self.cnt_buf = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.pose_buf = torch.eye(4, device=DEV)
        self.step, self.it, self.graphs, self.trained, self.targets = None, 0, [], [], []
        self.ra.anchor_fields(self.st, [1000 + (i % 2) for i in range(START)])

    def frame(self, f, advance=True, iterations=G.PER_FRAME):
        F, st, ra, rb = self.F, self.st, self.ra, self.rb
        if advance:
            F.advance(st, f)
        self.pose_buf.copy_(dev(F.frames[f]["c2w"]))
        ra.observed_fields_device(st.nc_rgbd[0], self.pose_buf, num_points=S.GRAPH_POINTS, seed=S.SEED, frame=f,
                                  out=(self.ids_buf, self.cnt_buf), camera=self.cam)
        if self.step is None:
            self.step = ra.capture_training(self.ids_buf, st.c_c2w, st.nc_rgbd, st.frame_cid_to_ncid, T, R, seed=G.SEED, camera=self.cam,
                                            current_count=self.cnt_buf, num_frames=st.num_frames)
            assert isinstance(self.step.graph, torch.cuda.CUDAGraph)
        n, m = int(self.cnt_buf), st.count
        cur = self.ids_buf[:n].clone()
        c2w, f2s = st.c_c2w[:m].clone(), st.frame_cid_to_ncid[:m].clone()
        for _ in range(iterations):
            la = self.step()
            self.graphs.append(self.step.graph)
            k = int(self.step.target.count)
            self.trained.append(self.step.target.field_ids[:k].cpu().clone())
            self.targets.append((m, f2s.cpu(), self.step.target.frame_cids[:k].cpu().clone()))
            la = {q: la[q].clone() for q in LOSS_KEYS}
            t = rb.sample_target_mv_device(cur, c2w, st.nc_rgbd, f2s, T, R, camera=self.cam, seed=G.SEED, iteration=self.it)
            assert int(t.count) == k and torch.equal(t.field_ids[:k], self.step.target.field_ids[:k]), (f, self.it)
            lb = rb.optimization_iteration(t, seed=G.SEED)
            assert_losses_equal(la, lb, (f, self.it))                       # bitwise, NaN matching NaN
            self.it += 1

    def snapshot(self):
        ra, st = self.ra, self.st
        rs = ra._reserved
        return [x.detach().cpu().numpy().copy() for x in (rs["positions"], rs["orientations"], ra._anchor["slot"], st.slot_c2w_prev,
                                                          st.slot_c2w)]

    def give_b_the_poses_of_a(self):
        md = self.ra._global_map_dict
        self.rb.set_field_poses(md["positions"].clone(), md["orientations"].clone())


def rigid(seed, angle, shift):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(RH.pose(RH.rot(rng.normal(size=3), angle), rng.uniform(-shift, shift, 3)).astype(np.float32)).to(DEV)


def test_one_graph_across_a_loop_closure():
    run = LiveRun()
    ra, st = run.ra, run.st
    for f in range(3):                                       # three frames under the one capture (a keyframe joins at frame 1)
        run.frame(f)
        if f == 1:
            ra.anchor_fields(st, [1] * 10, field_ids=list(range(20, 30)))
    # the loop closure: every keyframe pose is perturbed rigidly, the map follows on the device
    D = rigid(7, 0.04, 0.05)
    slots = [st.slot_of(f) for f in st.frame_ids]
    st.set_keyframe_poses(D @ st.slot_c2w[slots])
    pos, quat, anchor, prev, new = run.snapshot()
    ptrs = (ra._reserved["positions"].data_ptr(), ra._reserved["orientations"].data_ptr())
    ra.repose_fields(st)
    torch.cuda.synchronize()
    got = run.snapshot()
    assert ptrs == (ra._reserved["positions"].data_ptr(), ra._reserved["orientations"].data_ptr())
    touched = check_against_fp64(got[0], got[1], pos, quat, anchor, prev, new, num=START, what="loop closure")
    assert touched[:START].all() and not touched[START:].any()             # rows past the count are unanchored and untouched
    assert np.array_equal(bits(got[3]), bits(new))                          # the store's previous table advanced
    assert not np.array_equal(got[1][:START], quat[:START])                 # orientations moved too
    run.give_b_the_poses_of_a()
    run.frame(3)                                             # the same graph keeps replaying: no "capture again"
    run.frame(3, advance=False)
    assert len(run.graphs) == 25 and all(g is run.step.graph for g in run.graphs)
    assert sum(len(t) for t in run.trained[15:]) > 0                        # fields were trained after the closure
    ra.repose_fields(st)                                     # nothing moved since: not one bit changes
    torch.cuda.synchronize()
    again = run.snapshot()
    assert np.array_equal(bits(again[0]), bits(got[0])) and np.array_equal(bits(again[1]), bits(got[1]))


def test_keyframe_release_under_the_live_graph():
    run = LiveRun(store_capacity=4)                          # slots 1..3: full after frame 1
    ra, st = run.ra, run.st
    run.frame(0, iterations=2)
    run.frame(1, iterations=2)
    assert st.frame_ids == [1000, 1001, 1] and st._free == []
    released = st.slot_of(1001)
    ra.remove_keyframe(st, 1001)                             # its fields go to 1000: no later keyframe existed, 1000 is the closest earlier
    assert st.frame_ids == [1000, 1] and st._free == [released] and st.count == 3
    assert ra._global_map_dict["kf_ids"].tolist() == [1000] * START
    assert ra._anchor["slot"][:START].tolist() == [st.slot_of(1000)] * START
    # keyframe 1000 moves, keyframe 1 does not: the rewired fields move by their NEW anchor's delta, in the same update
    D = rigid(9, 0.05, 0.08)
    st.set_keyframe_poses(torch.stack((D @ st.slot_c2w[st.slot_of(1000)], st.slot_c2w[st.slot_of(1)])))
    pos, quat, anchor, prev, new = run.snapshot()
    ra.repose_fields(st)
    torch.cuda.synchronize()
    got = run.snapshot()
    touched = check_against_fp64(got[0], got[1], pos, quat, anchor, prev, new, num=START, what="rewired")
    assert touched[:START].all()
    was_1001 = np.arange(START) % 2 == 1
    want = (D.cpu().numpy().astype(np.float64) @ np.concatenate((pos[:START], np.ones((START, 1))), -1).T).T[:, :3]
    assert np.abs(got[0][:START][was_1001] - want[was_1001]).max() < 1e-4 and np.abs(got[0][:START] - pos[:START]).max() > 1e-3
    run.give_b_the_poses_of_a()
    before = len(run.targets)
    for _ in range(4):                                       # 20 iterations: the targets never name the released slot
        run.frame(1, advance=False)
    assert len(run.targets) - before == 20
    for m, f2s, cids in run.targets[before:]:
        assert m == 3 and released not in f2s.tolist()
        assert cids.numel() == 0 or (int(cids.min()) >= 0 and int(cids.max()) < m and released not in f2s[cids.long()].tolist())
    assert sum(c.numel() for _, _, c in run.targets[before:]) > 0
    # the slot is reused by a new keyframe: the graph still replays
    run.frame(3, iterations=3)                               # F.advance adds frame 3 as a keyframe
    assert st.slot_of(3) == released and st.frame_ids == [1000, 3, 1] and st.count == 4
    assert all(g is run.step.graph for g in run.graphs)
    assert released in run.targets[-1][1].tolist()
