"""Fixed-capacity keyframe store for the multi-view target sampler.

The reference keeps its training frames in a preallocated image tensor plus tensors it REBUILDS at every frame
(``_init_mv_training_data`` / ``_update_mv_training_data``, run_mapping.py:1673-1713): ``_frame_cid_to_ncid`` and
``_c_c2w_tensor`` grow with every keyframe, so anything captured over them is stale one keyframe later.  ``KeyframeStore``
does the same bookkeeping into buffers of fixed shape and storage, all written in place, with the number of frames in a
device int32 -- what ``sample_target_mv_device(current_count=..., num_frames=...)`` and ``capture_training`` read.  The host
keeps the counts too; nothing here synchronises.

Slot layout as in the reference: slot 0 of ``nc_rgbd`` is the current frame (unless ``keyframes_only``), a keyframe takes
the front of the free list (``_free_rgbd_tensor_indices``): the never-used slots in ascending order, then the slots
``remove_keyframe`` released, oldest release first.  The frame list (``c_c2w``, ``frame_cid_to_ncid``) is the current
frame first, when there is one, then the keyframes in ascending slot order, as the reference's mask over
``_nc_frame_id_tensor`` gives it (rm.py:1701-1709) -- insertion order until a released slot is reused.  ``frame_ids`` is in
that order too.

For fields anchored to keyframes (``NeuralGraphRenderer.anchor_fields`` / ``repose_fields``) the store also keeps two pose
tables indexed by SLOT: ``slot_c2w``, the keyframe poses in force, and ``slot_c2w_prev``, the poses at the last re-pose.
A new keyframe's row of both is its pose, so its first re-pose leaves its fields alone.
"""
import bisect

import torch


class KeyframeStore:
    def __init__(self, capacity: int, height: int, width: int, device="cuda", keyframes_only: bool = False):
        if capacity < 1:
            raise ValueError(f"KeyframeStore: capacity must be >= 1, got {capacity}")
        self.capacity, self.keyframes_only = int(capacity), bool(keyframes_only)
        self.nc_rgbd = torch.zeros(capacity, height, width, 4, device=device)
        eye = torch.eye(4, device=device)
        self.c_c2w = eye.repeat(capacity, 1, 1).contiguous()               # padding poses stay finite
        self.frame_cid_to_ncid = torch.zeros(capacity, dtype=torch.int64, device=device)
        self.num_frames = torch.zeros(1, dtype=torch.int32, device=device)
        self.slot_c2w = eye.repeat(capacity, 1, 1).contiguous()            # keyframe poses in force, by slot
        self.slot_c2w_prev = eye.repeat(capacity, 1, 1).contiguous()       # keyframe poses at the last re-pose, by slot
        self._cur_c2w = eye.clone()
        first = 0 if self.keyframes_only else 1
        # slot of every list position, kept on the device in place: entry 0 is the current frame's slot 0, _list_slots (a view
        # of the rest) the keyframes' slots in list order; the tail is padding, clamped into range
        self._list_all = torch.cat((torch.zeros(1, dtype=torch.int64, device=device),
                                    torch.arange(first, first + capacity, device=device).clamp_(max=capacity - 1)))
        self._list_slots = self._list_all[1:]
        self.has_current = False          # host mirrors
        self.frame_ids = []               # frame id of every keyframe, list order (ascending slot)
        self._slots = []                  # its slot
        self._free = list(range(first, capacity))
        self.current_frame_id = -1
        self._refresh()

    # -- host-side counts ----------------------------------------------------------------------
    @property
    def num_keyframes(self) -> int:
        return len(self.frame_ids)

    @property
    def count(self) -> int:
        """host mirror of num_frames"""
        return int(self.has_current) + len(self.frame_ids)

    def _refresh(self):
        """frame list from the host state: in-place writes of host-known extents"""
        n, off, cap = len(self.frame_ids), int(self.has_current), self.capacity
        if self.has_current:
            self.c_c2w[0].copy_(self._cur_c2w)
            self.frame_cid_to_ncid.copy_(self._list_all[:cap])
        else:
            self.frame_cid_to_ncid.copy_(self._list_slots)
        if n:
            torch.index_select(self.slot_c2w, 0, self._list_slots[:n], out=self.c_c2w[off:off + n])
        self.num_frames.fill_(off + n)

    def slot_of(self, frame_id: int) -> int:
        """the nc_rgbd slot (= row of slot_c2w / slot_c2w_prev) of a keyframe"""
        try:
            return self._slots[self.frame_ids.index(int(frame_id))]
        except ValueError:
            raise ValueError(f"KeyframeStore: frame {frame_id} is not a keyframe of the store") from None

    # -- the reference's per-frame updates -----------------------------------------------------
    def set_current(self, rgbd: torch.Tensor, c2w: torch.Tensor, frame_id: int = -1):
        """the current frame with a tracked pose: slot 0, first in the list (rm.py:1691-1692, 1711)"""
        if self.keyframes_only:
            raise ValueError("KeyframeStore(keyframes_only=True) has no current-frame slot")
        self.nc_rgbd[0].copy_(rgbd)
        self._cur_c2w.copy_(c2w)
        self.current_frame_id = int(frame_id)
        self.has_current = True
        self._refresh()

    def clear_current(self):
        """tracking lost: slot 0 leaves the list (rm.py:1688-1689)"""
        self.has_current = False
        self.current_frame_id = -1
        self._refresh()

    def add_keyframe(self, rgbd: torch.Tensor, frame_id: int, c2w: torch.Tensor = None):
        """the front of the free list (rm.py:1694-1699); c2w=None: the current frame's pose (the current frame became a keyframe)"""
        if not self._free:
            raise ValueError("Maximum number of keyframes reached.")
        if c2w is None:
            if not self.has_current:
                raise ValueError("KeyframeStore.add_keyframe: no current pose to take, pass c2w")
            c2w = self._cur_c2w
        slot, n = self._free.pop(0), len(self.frame_ids)
        k = bisect.bisect_left(self._slots, slot)                 # list position: ascending slot
        self.nc_rgbd[slot].copy_(rgbd)
        self.slot_c2w[slot].copy_(c2w)
        self.slot_c2w_prev[slot].copy_(c2w)                       # the first re-pose of its fields is the bitwise no-op
        if k < n:                                                 # a released slot below later ones: the tail moves up
            self._list_slots[k + 1:n + 1] = self._list_slots[k:n].clone()
        self._list_slots[k].fill_(slot)
        self.frame_ids.insert(k, int(frame_id))
        self._slots.insert(k, slot)
        self._refresh()

    def remove_keyframe(self, frame_id: int):
        """The SLAM front end culled a keyframe (rm.py:907-915): its slot leaves the frame list and goes to the BACK of the
        free list, frame_ids loses the entry, num_frames drops; the image and the pose rows of the slot stay as they are
        until the slot is reused.  The reference appends the removed frame's id, not its slot, to its free list (rm.py:914)
        -- a slip there: the id need not be a free slot.  Here the slot goes on the list.  Unknown frame: ValueError,
        nothing changes.  In place, no synchronisation."""
        slot = self.slot_of(frame_id)
        k, n = self._slots.index(slot), len(self.frame_ids)
        if k < n - 1:
            self._list_slots[k:n - 1] = self._list_slots[k + 1:n].clone()
        del self.frame_ids[k], self._slots[k]
        self._free.append(slot)
        self._refresh()

    def set_keyframe_poses(self, c2ws: torch.Tensor):
        """new poses of all keyframes, in the order of frame_ids (the pose graph moved them: rm.py:1704-1713).  slot_c2w_prev
        keeps the poses of the last re-pose: NeuralGraphRenderer.repose_fields moves the anchored fields and advances it."""
        n = len(self.frame_ids)
        if tuple(c2ws.shape) != (n, 4, 4):
            raise ValueError(f"KeyframeStore.set_keyframe_poses: expected ({n}, 4, 4), got {tuple(c2ws.shape)}")
        if n:
            self.slot_c2w.index_copy_(0, self._list_slots[:n], c2ws.to(device=self.slot_c2w.device, dtype=self.slot_c2w.dtype))
        self._refresh()
