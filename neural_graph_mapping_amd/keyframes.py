"""Fixed-capacity keyframe store for the multi-view target sampler.

The reference keeps its training frames in a preallocated image tensor plus tensors it REBUILDS at every frame
(``_init_mv_training_data`` / ``_update_mv_training_data``, run_mapping.py:1673-1713): ``_frame_cid_to_ncid`` and
``_c_c2w_tensor`` grow with every keyframe, so anything captured over them is stale one keyframe later.  ``KeyframeStore``
does the same bookkeeping into buffers of fixed shape and storage, all written in place, with the number of frames in a
device int32 -- what ``sample_target_mv_device(current_count=..., num_frames=...)`` and ``capture_training`` read.  The host
keeps the counts too; nothing here synchronises.

Slot layout as in the reference: slot 0 of ``nc_rgbd`` is the current frame (unless ``keyframes_only``), keyframes take the
free slots in ascending order and are never released.  The frame list (``c_c2w``, ``frame_cid_to_ncid``) is the current frame
first, when there is one, then the keyframes in insertion order.
"""
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
        self._kf_c2w = eye.repeat(capacity, 1, 1).contiguous()             # keyframe poses, insertion order
        self._cur_c2w = eye.clone()
        first = 0 if self.keyframes_only else 1
        # slot of every list position, with / without the current frame in front (clamped: the tail is padding)
        self._ncid_kf = torch.arange(first, first + capacity, device=device).clamp_(max=capacity - 1)
        self._ncid_cur = torch.arange(capacity, device=device)
        self._first = first
        self.has_current = False          # host mirrors
        self.frame_ids = []               # frame id of every keyframe, insertion order
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
        n, off = len(self.frame_ids), int(self.has_current)
        if self.has_current:
            self.c_c2w[0].copy_(self._cur_c2w)
            self.frame_cid_to_ncid.copy_(self._ncid_cur)
        else:
            self.frame_cid_to_ncid.copy_(self._ncid_kf)
        if n:
            self.c_c2w[off:off + n].copy_(self._kf_c2w[:n])
        self.num_frames.fill_(off + n)

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
        """the next free slot (rm.py:1694-1699); c2w=None: the current frame's pose (the current frame became a keyframe)"""
        if self._first + len(self.frame_ids) >= self.capacity:
            raise ValueError("Maximum number of keyframes reached.")
        if c2w is None:
            if not self.has_current:
                raise ValueError("KeyframeStore.add_keyframe: no current pose to take, pass c2w")
            c2w = self._cur_c2w
        k = len(self.frame_ids)
        self.nc_rgbd[self._first + k].copy_(rgbd)
        self._kf_c2w[k].copy_(c2w)
        self.frame_ids.append(int(frame_id))
        self._refresh()

    def set_keyframe_poses(self, c2ws: torch.Tensor):
        """new poses of all keyframes, insertion order (the pose graph moved them: rm.py:1704-1713)"""
        n = len(self.frame_ids)
        if tuple(c2ws.shape) != (n, 4, 4):
            raise ValueError(f"KeyframeStore.set_keyframe_poses: expected ({n}, 4, 4), got {tuple(c2ws.shape)}")
        if n:
            self._kf_c2w[:n].copy_(c2ws)
        self._refresh()
