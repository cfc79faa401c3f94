"""CPU-side checks of fields anchored to keyframes (include/ngm_hip.h ngm_fields_repose; KeyframeStore.remove_keyframe;
NeuralGraphRenderer.anchor_fields / remove_keyframe / repose_fields): the host restatement against a fixture from the real
reference, symbols and the struct layout, the store's bookkeeping with release against the reference's restated, the
rewiring rule and the anchors' bookkeeping on CPU tensors, and the refusals of the new op.  No GPU."""
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
import _repose_host as RH  # noqa: E402
from neural_graph_mapping_amd import models as M  # noqa: E402
from neural_graph_mapping_amd import renderer as Rr  # noqa: E402
from neural_graph_mapping_amd.keyframes import KeyframeStore  # noqa: E402

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def capi():
    from neural_graph_mapping_amd import _capi, build
    if not os.path.exists(_capi.LIB_PATH):
        build.build(verbose=False)
    return _capi


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_reference_fixture():
    """G25 (tests/golden/make_golden_repose.py): the real _absolute_map_dict_to_relative / _relative_map_dict_to_absolute in
    float32.  Bound: each of the two affine maps sums three products and a translation of magnitude <= M per coordinate (4
    roundings on terms <= 3 M), the inverse's entries carry a few roundings of their own: 64 eps32 M covers both maps with
    room for torch's LU inverse against the adjugate; for quaternions M is the largest field-quaternion norm."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g25_repose.npz"))
    pos, quat, kf, prev, new = g["positions"], g["orientations"], g["kf_ids"], g["prev_kf2ws"], g["new_kf2ws"]
    m_pos = max(1.0, float(np.abs(pos).max()), float(np.abs(prev[:, :3, 3]).max()), float(np.abs(new[:, :3, 3]).max()))
    m_quat = float(np.linalg.norm(quat, axis=-1).max())
    assert m_quat > 1.5                                                     # the non-unit quaternion is there
    for dt in (np.float32, np.float64):
        rp, rq = RH.absolute_to_relative(pos, quat, kf, prev, dt)
        assert rp.dtype == dt and rq.dtype == dt
        ep, eq = RH.errors(rp, rq, g["rel_positions"], g["rel_orientations"])
        print(f"{dt.__name__} relative: {ep:.3e} / {eq:.3e}")
        assert ep <= 64 * EPS32 * m_pos and eq <= 64 * EPS32 * m_quat
        op, oq = RH.relative_to_absolute(rp, rq, kf, new, dt)
        ep, eq = RH.errors(op, oq, g["out_positions"], g["out_orientations"])
        print(f"{dt.__name__} absolute: {ep:.3e} / {eq:.3e} (bounds {64 * EPS32 * m_pos:.3e} / {64 * EPS32 * m_quat:.3e})")
        assert ep <= 64 * EPS32 * m_pos and eq <= 64 * EPS32 * m_quat
    # the three rules: keyframe 4 did not move -- its fields come back bit for bit, everything else moved
    p, q, touched = RH.repose(pos, quat, kf, prev, new, np.float32)
    assert touched.tolist() == [k != 4 for k in kf]
    assert np.array_equal(p[~touched].view(np.uint32), pos[~touched].view(np.uint32))
    assert np.array_equal(q[~touched].view(np.uint32), quat[~touched].view(np.uint32))
    anchor = kf.copy()
    anchor[0], anchor[1] = -1, 5                                             # unanchored, out of range
    bad = new.copy()
    bad[2, 1, 3] = np.nan                                                    # a lost pose
    _, _, t2 = RH.repose(pos, quat, anchor, prev, bad, np.float32, num=10)
    assert t2.tolist() == [i >= 2 and i < 10 and kf[i] not in (2, 4) for i in range(12)]


def test_matrix_to_quaternion_at_pi_and_inverse():
    """a rotation by pi about each axis: the quaternion is exact to rounding (the trace-only formula divides by ~0 there);
    the adjugate inverse against numpy's on a non-orthonormal affine matrix"""
    for ax in range(3):
        want = np.zeros(4)
        want[1 + ax] = 1.0
        for dt in (np.float32, np.float64):
            q = RH.matrix_to_quaternion(RH.rot(ax, np.pi)[None], dt)[0]
            assert np.abs(np.minimum(np.abs(q - want), np.abs(q + want))).max() <= 4 * np.finfo(dt).eps
    rng = np.random.default_rng(0)
    T = np.tile(np.eye(4), (6, 1, 1))
    T[:, :3, :] = rng.normal(size=(6, 3, 4))
    assert np.abs(RH.affine_inverse(T) - np.linalg.inv(T)).max() < 1e-9
    q = RH.matrix_to_quaternion(np.stack([RH.rot(rng.normal(size=3), a) for a in (0.1, 1.0, 2.0, 3.0)]))
    assert np.allclose(np.linalg.norm(q, axis=-1), 1.0) and (q[:, 0] >= 0).all()


# ------------------------------------------------------------------------------------------------ ABI
def test_symbol_declared_and_exported_abi_unchanged(capi):
    head = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    L = capi.lib()
    assert re.search(r"\bngm_fields_repose\s*\(", src)
    assert "ngm_fields_repose" in capi.EXPORTED and hasattr(L, "ngm_fields_repose")
    assert int(re.search(r"#define\s+NGM_ABI_VERSION\s+(\d+)", head).group(1)) == 11 == L.ngm_abi_version()
    for rule in ("BITWISE EQUAL", "non-finite", "at or beyond the field count"):     # the three stricter rules are stated
        assert rule in head, rule
    # argument validation happens before any launch (no device here)
    assert L.ngm_fields_repose(None, None) == capi.NGM_E_INVALID and b"NULL" in L.ngm_last_error()
    a = capi.FieldsReposeArgs(8, 8, 8, 8, 8, None, -1, 3, 1, 0)
    assert L.ngm_fields_repose(C.byref(a), None) == capi.NGM_E_INVALID and b">= 0" in L.ngm_last_error()
    a.num_fields, a.num_poses = 4, -2
    assert L.ngm_fields_repose(C.byref(a), None) == capi.NGM_E_INVALID and b">= 0" in L.ngm_last_error()
    for missing in ("positions", "orientations", "anchor_slot", "prev_poses", "new_poses"):
        a = capi.FieldsReposeArgs(8, 8, 8, 8, 8, None, 4, 3, 1, 0)
        setattr(a, missing, None)
        assert L.ngm_fields_repose(C.byref(a), None) == capi.NGM_E_INVALID and b"NULL array" in L.ngm_last_error(), missing
    a = capi.FieldsReposeArgs(None, None, None, None, None, None, 0, 0, 1, 0)       # an empty map, no keyframes: nothing to do
    assert L.ngm_fields_repose(C.byref(a), None) == capi.NGM_OK


def test_struct_layout_matches_header(capi, tmp_path):
    fa = [f[0] for f in capi.FieldsReposeArgs._fields_]
    fmt = " ".join(["%zu"] * (1 + len(fa)))
    args = ",".join(["sizeof(ngm_fields_repose_args)"] + [f"offsetof(ngm_fields_repose_args,{f})" for f in fa])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ngm_hip.h"\n'
                   f'int main(){{printf("{fmt}\\n",{args});return 0;}}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    FA = capi.FieldsReposeArgs
    assert sizes == [C.sizeof(FA)] + [getattr(FA, f).offset for f in fa]


def test_op_registered_and_refuses_cpu_tensors(capi):
    from neural_graph_mapping_amd import ops
    assert hasattr(torch.ops.ngm355, "fields_repose_")
    schema = str(torch.ops.ngm355.fields_repose_.default._schema)
    assert "Tensor(a0!) positions" in schema and "Tensor(a1!) orientations" in schema       # declared as mutating
    pos, quat, anchor = torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(5, dtype=torch.int32)
    prev, new = torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fields_repose_(pos, quat, anchor, prev, new)
    with pytest.raises(TypeError, match="anchor_slot must be an int32"):
        ops.fields_repose_(pos, quat, anchor.long(), prev, new)
    with pytest.raises(ValueError, match="orientations"):
        ops.fields_repose_(pos, quat[:4], anchor, prev, new)
    with pytest.raises(ValueError, match="differ"):
        ops.fields_repose_(pos, quat, anchor, prev, new[:1])
    with pytest.raises(ValueError, match="num_fields"):
        ops.fields_repose_(pos, quat, anchor, prev, new, num_fields=6)
    with pytest.raises(TypeError, match="one-element int32"):
        ops.fields_repose_(pos, quat, anchor, prev, new, num_fields_dev=torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ KeyframeStore with release
H, W = 4, 5


class StorePair:
    """a KeyframeStore on CPU tensors and the reference bookkeeping, driven together"""

    def __init__(self, cap, keyframes_only=False):
        self.g = torch.Generator().manual_seed(cap)
        self.st, self.ref = KeyframeStore(cap, H, W, device="cpu", keyframes_only=keyframes_only), RH.ReferenceKeyframesRelease(cap, keyframes_only)
        self.cap, self.images, self.ko = cap, {}, keyframes_only
        self.ptrs = self.addresses()

    def addresses(self):
        st = self.st
        return [t.data_ptr() for t in (st.nc_rgbd, st.c_c2w, st.frame_cid_to_ncid, st.num_frames, st.slot_c2w, st.slot_c2w_prev)]

    def keyframe(self, f):
        img, p = torch.rand(H, W, 4, generator=self.g), torch.rand(4, 4, generator=self.g)
        self.images[f] = img
        if self.ko:
            self.st.add_keyframe(img, f, c2w=p)
            self.ref.update(keyframe=(f, f, p))
        else:
            self.st.set_current(img, p, frame_id=f)
            self.st.add_keyframe(img, f)
            self.ref.update(current=(f, f, p), keyframe=(f, f, p))
        self.check()
        return p

    def remove(self, f):
        self.st.remove_keyframe(f)
        self.ref.remove(f)
        self.ref.lists()
        self.check()

    def check(self):
        st, ref = self.st, self.ref
        n, ncid, c2w = st.count, ref.frame_cid_to_ncid, ref.c_c2w
        assert int(st.num_frames) == n == len(ncid)
        assert st.frame_cid_to_ncid[:n].tolist() == list(ncid)
        off = int(st.has_current)
        assert st.frame_ids == [int(f) for f in ref.frame_id[ncid[off:]]]                 # ascending slot order
        assert st.num_keyframes == n - off
        for k in range(n):
            assert torch.equal(st.c_c2w[k], c2w[k]), k
            assert torch.equal(st.nc_rgbd[ncid[k]], self.images[ref.images[ncid[k]]]), k
        for f in st.frame_ids:
            s = st.slot_of(f)
            assert int(ref.frame_id[s]) == f and torch.equal(st.slot_c2w[s], ref.poses[f])
        assert sorted(st._free) == sorted(ref.free) and st._free == ref.free                # the slot, not the frame id, is freed
        assert int(st.frame_cid_to_ncid.min()) >= 0 and int(st.frame_cid_to_ncid.max()) < self.cap      # padding stays in range
        assert bool(torch.isfinite(st.c_c2w).all()) and bool(torch.isfinite(st.slot_c2w).all())
        assert self.addresses() == self.ptrs                                              # everything in place


def test_store_remove_middle_newest_and_add_after():
    sp = StorePair(8)
    poses = {f: sp.keyframe(f) for f in (10, 20, 30, 40)}                    # slots 1..4
    assert [sp.st.slot_of(f) for f in (10, 20, 30, 40)] == [1, 2, 3, 4]
    assert all(torch.equal(sp.st.slot_c2w_prev[sp.st.slot_of(f)], poses[f]) for f in poses)   # prev row = the pose at insertion
    sp.remove(20)                                                            # a middle keyframe
    assert sp.st.frame_ids == [10, 30, 40] and sp.st.frame_cid_to_ncid[:4].tolist() == [0, 1, 3, 4] and sp.st.count == 4
    sp.remove(40)                                                            # the newest
    assert sp.st.frame_ids == [10, 30] and sp.st.count == 3
    sp.keyframe(50)                                                          # the next NEVER-USED slot, not a released one
    assert sp.st.slot_of(50) == 5 and sp.st.frame_ids == [10, 30, 50]
    with pytest.raises(ValueError, match="not a keyframe"):
        sp.st.slot_of(20)
    # the pose graph moves the keyframes: poses in the order of frame_ids; the previous table keeps the old poses
    before = sp.st.slot_c2w_prev.clone()
    moved = torch.rand(3, 4, 4, generator=sp.g)
    sp.st.set_keyframe_poses(moved)
    for f, p in zip(sp.st.frame_ids, moved):
        sp.ref.poses[f] = p
    sp.ref.update(current=(50, 50, sp.ref.poses[50]))
    sp.st.set_current(sp.images[50], sp.ref.poses[50], frame_id=50)
    sp.check()
    assert torch.equal(sp.st.slot_c2w_prev, before)


def test_store_full_remove_add_takes_the_released_slot():
    sp = StorePair(4)
    for f in (1, 2, 3):
        sp.keyframe(f)
    with pytest.raises(ValueError, match="Maximum number of keyframes reached"):
        sp.st.add_keyframe(sp.images[1], 4)
    sp.remove(2)
    p = sp.keyframe(7)                                                       # slot 2 again: frame 7 sits BETWEEN 1 and 3 in the list
    assert sp.st.slot_of(7) == 2 and sp.st.frame_ids == [1, 7, 3]
    assert torch.equal(sp.st.slot_c2w_prev[2], p) and torch.equal(sp.st.slot_c2w[2], p)
    moved = torch.rand(3, 4, 4, generator=sp.g)
    sp.st.set_keyframe_poses(moved)                                          # still in the order of frame_ids
    assert torch.equal(sp.st.slot_c2w[2], moved[1]) and torch.equal(sp.st.c_c2w[2], moved[1])
    sp.st.clear_current()
    assert sp.st.frame_cid_to_ncid[:3].tolist() == [1, 2, 3] and torch.equal(sp.st.c_c2w[:3], moved)
    with pytest.raises(ValueError, match="Maximum number of keyframes reached"):
        sp.st.add_keyframe(sp.images[1], 8, c2w=p)


def test_store_keyframes_only_and_unknown_frame():
    sp = StorePair(3, keyframes_only=True)
    for f in (5, 6, 7):
        sp.keyframe(f)
    assert [sp.st.slot_of(f) for f in (5, 6, 7)] == [0, 1, 2]
    sp.remove(5)
    assert sp.st.frame_cid_to_ncid[:2].tolist() == [1, 2]
    sp.keyframe(9)
    assert sp.st.slot_of(9) == 0 and sp.st.frame_ids == [9, 6, 7]
    state = (list(sp.st.frame_ids), list(sp.st._free), sp.st.frame_cid_to_ncid.clone(), sp.st.c_c2w.clone(), int(sp.st.num_frames))
    with pytest.raises(ValueError, match="not a keyframe"):
        sp.st.remove_keyframe(123)
    assert state[0] == sp.st.frame_ids and state[1] == sp.st._free and torch.equal(state[2], sp.st.frame_cid_to_ncid)
    assert torch.equal(state[3], sp.st.c_c2w) and state[4] == int(sp.st.num_frames)
    sp.check()


# ------------------------------------------------------------------------------------------------ anchors and rewiring on CPU tensors
def cpu_renderer():
    fkw = dict(encoding_type="neural_graph_mapping.positional_encodings.PositionalEncodingFourier",
               encoding_kwargs=dict(dim_in=3, dim_out=32, mu=0.0, sigma=4.0, raw_coords=True), num_layers=1, dim_out=4,
               neus_initial_sd=1.0)
    torch.manual_seed(3)
    model = M.NeuralFieldSet(dim_points=3, field_type="neural_graph_mapping.models.NeuralField", field_kwargs=fkw, num_knn=2,
                             distance_factor=10.0, outside_value=1.0, field_radius=1.0, scale_mode="unit_cube")
    cam = Rr.Camera(32, 24, 25.0, 25.0, 15.5, 11.5)
    return Rr.NeuralGraphRenderer(model, cam, Rr.shipped_config(), device="cpu")


def store_with(frames, cap=8):
    st = KeyframeStore(cap, H, W, device="cpu")
    for f in frames:
        st.add_keyframe(torch.zeros(H, W, 4), f, c2w=torch.eye(4) * 1.0)
    return st


def anchored(frames, kf_of_field, reserve=None):
    r = cpu_renderer()
    n = len(kf_of_field)
    r.add_fields(n)
    pos, quat = torch.rand(n, 3), torch.rand(n, 4)
    r.set_field_poses(pos.clone(), quat.clone())
    if reserve:
        r.reserve_fields(reserve)
    st = store_with(frames)
    r.anchor_fields(st, kf_of_field)
    return r, st, pos, quat


@pytest.mark.parametrize("reserve", [None, 9])
def test_rewiring_rule_on_cpu_tensors(reserve):
    # later neighbour present before the update
    kf = [10, 20, 20, 30, 40, 20]
    r, st, pos, quat = anchored([10, 20, 30, 40], kf, reserve)
    assert r._global_map_dict["kf_ids"].dtype == torch.int64 and r._anchor["slot"].dtype == torch.int32
    assert r._global_map_dict["kf_ids"].tolist() == kf and r._anchor["slot"][:6].tolist() == [1, 2, 2, 3, 4, 2]
    if reserve:
        assert r._anchor["slot"].shape[0] == r._anchor["kf_ids"].shape[0] == reserve and r._anchor["slot"][6:].tolist() == [-1] * 3
    ptrs = (r._anchor["kf_ids"].data_ptr(), r._anchor["slot"].data_ptr())
    r.remove_keyframe(st, 20)
    want = RH.rewire(kf, [10, 20, 30, 40], [20])
    assert r._global_map_dict["kf_ids"].tolist() == want.tolist() == [10, 30, 30, 30, 40, 30]
    assert r._anchor["slot"][:6].tolist() == [1, 3, 3, 3, 4, 3] and st.frame_ids == [10, 30, 40]
    # the removed keyframe was the newest: only an earlier one is left
    r.remove_keyframe(st, 40)
    want = RH.rewire(want, [10, 30, 40], [40])
    assert r._global_map_dict["kf_ids"].tolist() == want.tolist() == [10, 30, 30, 30, 30, 30]
    assert ptrs == (r._anchor["kf_ids"].data_ptr(), r._anchor["slot"].data_ptr())       # in place
    # positions and orientations are not transformed (rm.py:928-929)
    assert torch.equal(r._global_map_dict["positions"], pos) and torch.equal(r._global_map_dict["orientations"], quat)
    # fields of two removed keyframes in one update
    kf = [10, 20, 30, 40, 30, 20]
    r, st, _, _ = anchored([10, 20, 30, 40], kf, reserve)
    r.remove_keyframe(st, [20, 30])
    assert r._global_map_dict["kf_ids"].tolist() == RH.rewire(kf, [10, 20, 30, 40], [20, 30]).tolist() == [10, 40, 40, 40, 40, 40]
    assert st.frame_ids == [10, 40] and r._anchor["slot"][:6].tolist() == [1, 4, 4, 4, 4, 4]
    r, st, _, _ = anchored([10, 20, 30, 40], kf, reserve)
    r.remove_keyframe(st, [30, 40])                                          # no later keyframe is left: the closest earlier one
    assert r._global_map_dict["kf_ids"].tolist() == RH.rewire(kf, [10, 20, 30, 40], [30, 40]).tolist() == [10, 20, 20, 20, 20, 20]
    # the reference's own corner: the later neighbour is the keyframe this very update adds -> the earlier one is taken
    assert RH.rewire([10, 20], [10, 20], [20], current_keyframe=25).tolist() == [10, 10]
    with pytest.raises(ValueError, match="not a keyframe"):
        r.remove_keyframe(st, 77)
    with pytest.raises(ValueError, match="no keyframe would be left"):
        r.remove_keyframe(st, [10, 20])
    assert st.frame_ids == [10, 20]


def test_anchor_bookkeeping_growth_and_checkpoint(tmp_path):
    r, st, _, _ = anchored([10, 20], [10, 20, 10])
    with pytest.raises(ValueError, match="not a keyframe"):
        r.anchor_fields(st, [10, 99, 10])
    with pytest.raises(ValueError, match="frame ids for"):
        r.anchor_fields(st, [10, 20])
    r.anchor_fields(st, [20], field_ids=[0])
    assert r._global_map_dict["kf_ids"].tolist() == [20, 20, 10]
    # without a reservation add_fields extends the anchors with unanchored rows
    r.add_fields(2)
    assert r._anchor["slot"].tolist() == [2, 2, 1, -1, -1] and r._anchor["kf_ids"].tolist() == [20, 20, 10, -1, -1]
    r.set_field_poses(torch.rand(5, 3), torch.rand(5, 4))
    assert r._global_map_dict["kf_ids"].tolist() == [20, 20, 10, -1, -1]
    # reserving afterwards carries the anchors over; reserved growth leaves new rows unanchored until they are given
    r.reserve_fields(8)
    assert r._anchor["slot"].tolist() == [2, 2, 1, -1, -1, -1, -1, -1]
    a_ptr = r._anchor["slot"].data_ptr()
    r.add_fields(1, positions=torch.rand(1, 3), orientations=torch.rand(1, 4))
    r.anchor_fields(st, [10], field_ids=[5])
    assert r._global_map_dict["kf_ids"].tolist() == [20, 20, 10, -1, -1, 10] and r._anchor["slot"].data_ptr() == a_ptr
    # checkpoint: kf_ids only when anchors were set; a loaded checkpoint keeps them for anchor_fields
    path = str(tmp_path / "m.pt")
    r.save_model(path)
    ck = torch.load(path)
    assert ck["map_dict"]["kf_ids"].tolist() == [20, 20, 10, -1, -1, 10] and ck["map_dict"]["kf_ids"].shape[0] == 6
    r2 = cpu_renderer()
    r2.load_model(path)
    assert r2._anchor is None and r2._global_map_dict["kf_ids"].tolist() == [20, 20, 10, -1, -1, 10]
    with pytest.raises(RuntimeError, match="anchor_fields first"):
        r2.repose_fields(st)
    keep = r2._global_map_dict["kf_ids"][:3]
    r2.anchor_fields(st, keep, field_ids=[0, 1, 2])
    assert r2._anchor["slot"].tolist() == [2, 2, 1, -1, -1, -1]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r2.repose_fields(st)
    plain = cpu_renderer()
    plain.add_fields(2)
    plain.set_field_poses(torch.rand(2, 3), torch.rand(2, 4))
    plain.save_model(path)
    assert "kf_ids" not in torch.load(path)["map_dict"]
