"""Render / train step of Neural Graph Mapping on the gfx950 kernels.

Host-side mirror of the renderer half of ``NeuralGraphMap`` (run_mapping.py): ``Target`` /
``Prediction`` records (:43-69), ``render_ijs`` (:439-666), ``quadrature`` (:709-799),
``compute_losses`` (:1769-1872) and the sparse-Adam plumbing (:347-389, :668-707, :1183-1221), plus
the fused fast path ``optimization_iteration`` that the mapping loop calls once per iteration
(:1123-1181).  The SLAM / pose-graph loop itself stays in the caller.
"""
import ctypes as C
from collections import namedtuple
import warnings
from typing import Dict, Optional

import torch

from . import _capi as K
from . import ops
from .models import NeuralFieldSet

Target = namedtuple("Target", ["ijs", "c2ws", "near_distances", "far_distances", "gt_distances", "field_ids", "rgbds",
                               "rgb_mask", "depth_mask", "term_probs", "term_mask"])
Prediction = namedtuple("Prediction", ["rgbds", "color_vars", "depth_vars", "term_probs", "freespace_geometry",
                                       "tsdf_residuals"])


class DeviceTarget(namedtuple("DeviceTarget", Target._fields + ("count", "subset_observed", "subset_random", "offsets",
                                                                "frame_cids", "u_xy", "world_size"))):
    """What NeuralGraphRenderer.sample_target_mv_device returns: the fields of Target at a fixed, host-known capacity
    (Fcap, R, ...), `count` = a device int32 tensor (1,) holding the number of surviving fields (rows count..Fcap-1 are
    padding: field_ids -1, masks 0, zeros elsewhere), plus the draws that produced them.
    NeuralGraphRenderer.optimization_iteration / capture_iteration take it as it is (the counted step: launched at Fcap,
    the kernels read `count` on the device); materialize() is only needed by consumers that want data-dependent shapes."""
    __slots__ = ()

    @staticmethod
    def from_sampler(o: dict, world_size: int) -> "DeviceTarget":
        """From the outputs of ops.target_sample_mv, or of ops.target_sample_mv_live (a LiveDeviceTarget then)"""
        rows = (o["ijs"], o["c2ws"], o["near"], o["far"], o["gt"], o["field_ids"], o["rgbds"], o["rgb_mask"], o["depth_mask"],
                o["term_probs"], o["term_mask"], o["count"], o["subset_observed"], o["subset_random"], o["offsets"],
                o["frame_cids"], o["u_xy"], int(world_size))                                       # in the order of _fields
        if "num_observed" in o:
            return LiveDeviceTarget(*rows, num_observed=o["num_observed"], num_random=o["num_random"])
        return DeviceTarget(*rows)

    def materialize(self) -> Target:
        """The usual Target, sliced to `count`: reading `count` is the one host synchronisation."""
        n = int(self.count.item())
        return Target(*(getattr(self, k)[:n] for k in Target._fields))

    def draws(self) -> dict:
        """The draws in the conventions of sample_target_mv(draws=...) (subset_observed: positions in current_field_ids,
        subset_random: field ids, offsets: already normalised, frame_cids / u_xy of the surviving fields): replaying them
        there reproduces this target.  Single process only (a rank's rows do not hold the other ranks' fields)."""
        if self.world_size != 1:
            raise ValueError("DeviceTarget.draws(): a sharded target holds only its own rank's fields")
        n = int(self.count.item())
        return dict(subset_observed=self.subset_observed, subset_random=self.subset_random, offsets=self.offsets,
                    frame_cids=self.frame_cids[:n], u_xy=self.u_xy[:n])


class LiveDeviceTarget(DeviceTarget):
    """The DeviceTarget of sample_target_mv_device(current_count=..., num_frames=...): subset_observed / subset_random are
    sized for their maxima with -1 past `num_observed` / `num_random` (device int32 tensors (1,)), since the number of
    current fields is read on the device.  materialize() / draws() slice by the device counts (they synchronise anyway)."""

    def __new__(cls, *args, num_observed, num_random, **kw):
        self = super().__new__(cls, *args, **kw)
        self.num_observed, self.num_random = num_observed, num_random
        return self

    def draws(self) -> dict:
        d = super().draws()
        d["subset_observed"] = self.subset_observed[:int(self.num_observed.item())]
        d["subset_random"] = self.subset_random[:int(self.num_random.item())]
        return d


class SvDeviceTarget(DeviceTarget):
    """The DeviceTarget of sample_target_sv_device (ngm_target_sample_sv): the multi-view draw fields (subset_observed,
    subset_random, offsets, frame_cids, u_xy) are None; the single-view draws are attributes, all device tensors at fixed
    shapes: pixels (num_points,) linear pixel indices with -1 past num_used (1,), hits (A,) crossing segments per entry of
    active_field_ids, num_candidates (1,), subset_fields (T,) positions in the candidate list with -1 past them, segments
    (capacity, R) the rays' points as linear pixel indices (-1 in padding rows)."""

    def __new__(cls, o: dict, world_size: int, rgbd, slot, num_train_fields: int):
        self = super().__new__(cls, o["ijs"], o["c2ws"], o["near"], o["far"], o["gt"], o["field_ids"], o["rgbds"], o["rgb_mask"],
                               o["depth_mask"], o["term_probs"], o["term_mask"], o["count"], None, None, None, None, None,
                               int(world_size))
        for k in ("pixels", "num_used", "hits", "num_candidates", "subset_fields", "segments"):
            setattr(self, k, o[k])
        self._rgbd, self._slot, self._num_train_fields = rgbd, slot, int(num_train_fields)
        return self

    def draws(self) -> dict:
        """The draws in the conventions of sample_target_sv(draws=...): subset_points = indices into torch.nonzero(depth),
        subset_fields = positions in the candidate list, segments = indices into the point list; replaying them there
        reproduces this target.  Reads the frame as it is NOW (and synchronises).  Single process only."""
        if self.world_size != 1:
            raise ValueError("DeviceTarget.draws(): a sharded target holds only its own rank's fields")
        img = self._rgbd
        if img.dim() == 4:
            img = img[0 if self._slot is None else min(max(int(self._slot.item()), 0), img.shape[0] - 1)]
        n = int(self.count.item())
        pixels = self.pixels[self.pixels >= 0]                 # after a replay unused entries (-1) may lie between used ones
        valid = torch.nonzero(img[..., 3].reshape(-1)).squeeze(1)              # ascending = the row order of torch.nonzero(depth)
        where = torch.full((img.shape[0] * img.shape[1],), -1, dtype=torch.int64, device=pixels.device)
        where[pixels] = torch.arange(pixels.shape[0], device=pixels.device)
        seg = self.segments[:n]
        seg = torch.where(seg >= 0, where[seg.clamp_min(0)], seg)              # -1: a recorded draw that named an unused point
        return dict(subset_points=torch.searchsorted(valid, pixels), segments=seg,
                    subset_fields=self.subset_fields[:min(int(self.num_candidates.item()), self._num_train_fields)])


class Camera:
    """Pinhole intrinsics with the reference's pixel-centre convention (camera.py:15-116)."""

    def __init__(self, width, height, fx, fy, cx, cy, s=0.0, pixel_center=0.0):
        if s != 0:
            raise NotImplementedError("Skew != 0 not supported.")
        self.fx, self.fy = fx, fy
        self.cx = cx - pixel_center + 0.5
        self.cy = cy - pixel_center + 0.5
        self.s, self.width, self.height = s, width, height

    def get_pinhole_camera_parameters(self, pixel_center: float):
        return self.fx, self.fy, self.cx - 0.5 + pixel_center, self.cy - 0.5 + pixel_center, self.s


class LossConfig:
    """Loss weights of rm.py:129-135 (defaults of config/neural_graph_map.yaml:31-37)."""

    def __init__(self, termination_weight=0.0, photometric_weight=1.0, depth_weight=1.0, freespace_weight=40.0,
                 tsdf_weight=50.0):
        self.termination_weight, self.photometric_weight = termination_weight, photometric_weight
        self.depth_weight, self.freespace_weight, self.tsdf_weight = depth_weight, freespace_weight, tsdf_weight


# keys NeuralGraphMap._read_config reads unconditionally (rm.py:116-220) among those this path consumes: a config the
# reference would refuse with a KeyError is refused here too, instead of training with a silent default
REQUIRED_CONFIG_KEYS = ("termination_weight", "photometric_weight", "photometric_loss", "depth_weight", "depth_loss",
                        "freespace_weight", "geometry_mode", "num_samples_coarse", "num_samples_depth_guided")


def shipped_config(**overrides) -> dict:
    """The render / loss / optimiser keys of the shipped config (config/neural_graph_map.yaml:26-70) with their shipped
    values -- a complete config for this path to start from (tests, tools, examples); `overrides` replace entries."""
    cfg = dict(color_factor=1.0, geometry_factor=20.0, learning_rate=1e-3, field_radius=1.0, termination_weight=0.0,
               photometric_weight=1.0, photometric_loss="l1", depth_weight=1.0, depth_loss="huber", freespace_weight=40.0,
               tsdf_weight=50.0, near_distance=0.0, far_distance=8.0, pixel_block_size=8192, block_size=3000000,
               geometry_mode="nrgbd", truncation_distance=0.1, num_train_fields=32, num_rays_per_field=512,
               num_samples_coarse=8, num_samples_depth_guided=16, range_depth_guided=None, adam_eps=1e-15,
               adam_weight_decay=1e-5)
    cfg.update(overrides)
    return cfg


def check_config(config: dict) -> None:
    """Fail loudly on what the reference requires and on what is not built (loss modes of losses.py:10-75)."""
    missing = [k for k in REQUIRED_CONFIG_KEYS if k not in config]
    if missing:
        raise KeyError(f"config lacks {missing}: NeuralGraphMap._read_config reads them unconditionally (rm.py:116-220)")
    if config["photometric_loss"] not in K.PHOTO:
        raise NotImplementedError(f"photometric_loss {config['photometric_loss']!r} is not built (built: {sorted(K.PHOTO)}, "
                                  "losses.py:26-36)")
    if config["depth_loss"] not in K.DEPTH:
        raise NotImplementedError(f"depth_loss {config['depth_loss']!r} is not built (built: {sorted(K.DEPTH)}, losses.py:60-75)")
    if config["geometry_mode"] not in K.GEO:
        raise ValueError(f"Unsupported geometry mode {config['geometry_mode']}")        # rm.py:760 wording


def make_render_cfg(camera: Camera, config: dict, guided: bool = True) -> K.RenderCfg:
    """Reference config keys (rm.py:116-220) -> ngm_render_cfg.  Optional keys keep the reference's `.get` defaults
    (tsdf_weight 0.0, color / geometry factor 1.0, range_depth_guided -> truncation_distance)."""
    check_config(config)
    fx, fy, cx, cy, _ = camera.get_pinhole_camera_parameters(0.0)
    tau = config.get("truncation_distance", 0.1)
    rho = config.get("range_depth_guided") or tau
    return K.render_cfg(
        geometry_mode=config["geometry_mode"], num_samples_coarse=config["num_samples_coarse"],
        num_samples_guided=config["num_samples_depth_guided"] if guided else 0,
        geometry_factor=config.get("geometry_factor", 1.0), color_factor=config.get("color_factor", 1.0),
        truncation_distance=tau, range_depth_guided=rho, fx=fx, fy=fy, cx=cx, cy=cy,
        w_termination=config["termination_weight"], w_photometric=config["photometric_weight"],
        w_depth=config["depth_weight"], w_freespace=config["freespace_weight"],
        w_tsdf=config.get("tsdf_weight", 0.0), photometric_loss=config["photometric_loss"], depth_loss=config["depth_loss"])


class NeuralGraphRenderer:
    """Renderer + per-field optimiser state for a ``NeuralFieldSet`` (hot-path half of NeuralGraphMap)."""

    def __init__(self, model: NeuralFieldSet, camera: Camera, config: dict, device="cuda"):
        self._model, self._camera, self._config, self._device = model, camera, dict(config), device
        # two radii, as in the reference: NeuralGraphMap._field_radius (run_mapping.py:137: sampler margins, near / far, grid
        # spacing, the mesh colour pass' `+ 0.1`) and the MODEL's own (models.py:278-285: the scaling of local coordinates and
        # the default inside test of the kNN branch).  The shipped configs set both from one YAML anchor; the kernels' field
        # configuration always carries the model's.
        self._field_radius = config.get("field_radius", model._field_radius)
        self._fc = model.field_cfg()
        # hidden layers of the forward kernels: "f32" = exact-fp32 MFMA; "bf16x3" = exact three-way bf16 split with fp32
        # accumulation (include/ngm_hip.h ngm_matmul_mode; fp32-level accuracy, same tolerances, bitwise deterministic,
        # 16x the matrix rate; fails loudly where not compiled); "auto" (default) = the split wherever it is compiled
        mm = config.get("mlp_matmul", "auto")
        self._fc.matmul_mode = K.MATMUL[mm]
        # activation stash of two-hidden-layer networks on the split path (include/ngm_hip.h, ngm_activation_stash): "full"
        # (default: both hidden layers' outputs, 512 B per sample, fastest) or "half" (layer 0's only, 256 B per sample: half
        # the stash memory and HBM traffic -- a 4096 x 128 x 32-field batch needs 4.3 instead of 8.6 GB --, the backward
        # recomputes the other layer on the matrix pipe: step + 1.5-4 %).  Part of THIS renderer's field configuration
        # (ABI 10): it sizes this renderer's workspaces; other renderers of the process are unaffected.
        self._fc.activation_stash = K.STASH[config.get("activation_stash") or "full"]
        # accumulation of the hash-table gradient (ngm_hash_grad_atomics): "exact" (default: Q23.40 integer LDS atomics, bitwise
        # reproducible) or "float" (opt-in: fp32 LDS atomics like the reference's CUDA package -- not reproducible run to run)
        self._fc.hash_grad_atomics = K.HASH_ATOMICS[config.get("hash_grad_atomics") or "exact"]
        fc = self._fc
        compiled = (fc.encoding in (K.ENC["fourier"], K.ENC["none"]) and fc.skip_mode == K.SKIP["no"] and 1 <= fc.num_layers <= 2
                    and 32 < fc.dim_enc <= 64 and 32 < fc.dim_hidden <= 64)
        # what the library resolves "auto" to for batch shapes whose LDS plan has room for the weight planes
        self.mlp_matmul = ("bf16x3" if compiled else "f32") if mm == "auto" else mm
        self._rc_train = make_render_cfg(camera, config, guided=True)
        self._rc_cache = {}
        self._mode = "train"               # rm.py:114: a new map is in train mode
        self._global_map_dict = None       # supplied by the mapping loop: positions / orientations
        self._learning_rate = config.get("learning_rate", 1e-3)
        self._adam_eps = config.get("adam_eps", 1e-15)
        self._adam_weight_decay = config.get("adam_weight_decay", 0.0)
        self._optim_state: Optional[Dict[str, Dict[str, torch.Tensor]]] = None
        self._step = 0
        self._step_dev = None
        self._ws_cache = {}
        self.process_group = None          # torch.distributed group for the loss all-reduce (None: single GPU)
        self.eval_fused = True             # render_pixels: one ngm_render_eval_knn call (False: the staged per-block entry points)
        self.eval_fallbacks = []           # why a fused evaluation call was retried with a smaller block / left to the staged loop
        self.last_eval_path = None
        self.peer_exchange = None          # distributed.PeerExchange: the same sum as one kernel inside the captured iteration
        self.peer_check_interval = 256     # iterations between PeerExchange.check() calls (a device synchronisation each)
        self._peer_calls = 0
        self.field_draw_generator = None   # torch.Generator of sample_target_mv(field_draw="balanced_by_owner"), see there
        self._target_iter_dev = None       # sample_target_mv_device's iteration counter (device int64, advanced by each call)
        self._warned_counted_fallback = False
        # opt-in: every update=True iteration adds one launch, training_iterations[field_ids] += 1 (rm.py:1188), so that
        # get_field_ids(min_iterations) keeps working when the iteration (and who trained in it) lives on the device
        self.track_training_iterations = False
        self._observe_frame_dev = None     # observed_fields_device's frame counter (device int64, advanced by each call)
        self.last_observed = None          # the chosen pixels / their number of the last observed_fields_device call
        # reserve_fields: dict(max=, epoch=, state={name: {exp_avg, exp_avg_sq} (max, ...)}, positions (max, 3), orientations
        # (max, 4), training_iterations (max,), num_fields_dev int32 (1,)); None = not reserved
        self._reserved: Optional[dict] = None
        self._reserve_epoch = 0
        # anchor_fields: dict(kf_ids int64, slot int32), one row per field (max_fields rows after reserve_fields); None = the
        # fields belong to no keyframe
        self._anchor: Optional[dict] = None

    def last_matmul(self, kernel: str = "forward") -> Optional[str]:
        """The arithmetic the library resolved `mlp_matmul` to in the LAST launch of the fused forward ("forward"), the
        point evaluation ("points") or the kNN evaluation ("knn"): "f32" | "bf16x3" (None before the first launch).
        `auto` is resolved per kernel and batch shape (LDS plan), so this -- not `self.mlp_matmul`, the host-side
        expectation -- is what a measurement should be labelled with."""
        v = K.lib().ngm_debug_last_matmul({"forward": 0, "points": 1, "knn": 2}[kernel])
        return {K.MATMUL["f32"]: "f32", K.MATMUL["bf16x3"]: "bf16x3"}.get(v)

    # -- map bookkeeping supplied by the caller ------------------------------------------------
    def set_field_poses(self, positions: torch.Tensor, orientations: torch.Tensor):
        """The poses of all fields.  After reserve_fields they are COPIED into the reserved pose rows (the loop-closure case:
        every pose moves, the storage -- what a captured graph reads -- stays); the number of rows must then be the number
        of fields: a map with reserved rows grows through add_fields(num_new, positions=, orientations=)."""
        rs = self._reserved
        if rs is not None:
            num = self._global_map_dict["num"]
            if positions.shape[0] != num or orientations.shape[0] != num:
                raise ValueError(f"set_field_poses: {positions.shape[0]} / {orientations.shape[0]} poses for {num} fields (reserved "
                                 "rows: add fields with add_fields(num_new, positions=, orientations=))")
            rs["positions"][:num].copy_(positions)
            rs["orientations"][:num].copy_(orientations)
            return
        old = self._global_map_dict
        self._global_map_dict = {"positions": positions, "orientations": orientations, "num": positions.shape[0]}
        if old is not None and "training_iterations" in old:            # the counts belong to the fields, not to their poses
            self._global_map_dict["training_iterations"] = old["training_iterations"]
        self._publish_kf_ids()

    def _training_iterations(self) -> torch.Tensor:
        """_global_map_dict["training_iterations"] (int64, one per field; rm.py:1188), created on first use and extended
        with zeros when fields were added, as add_fields extends the parameters"""
        md = self._global_map_dict
        if self._reserved is not None:                     # max_fields rows, zero past `num`: never reallocated
            return self._reserved["training_iterations"]
        ti, num = md.get("training_iterations"), md["num"]
        if ti is None or ti.shape[0] < num:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("training_iterations must exist before a graph capture (capture_iteration / "
                                   "capture_training create it when track_training_iterations is set)")
            new = torch.zeros(num, dtype=torch.int64, device=self._device)
            if ti is not None:
                new[:ti.shape[0]] = ti
            md["training_iterations"] = ti = new
        return ti

    def _count_training_iteration(self, field_ids: torch.Tensor, count: Optional[torch.Tensor]) -> None:
        if self.track_training_iterations and field_ids.shape[0] > 0:
            fids = field_ids if field_ids.dtype == torch.int64 else field_ids.long()
            # reserved rows: the bound is the capacity -- the sampler emits no id at or beyond the device field count (its
            # owner filter drops them), and training_iterations has a row for every id below the capacity
            num = self._global_map_dict["num"] if self._reserved is None else self._reserved["max"]
            ops.field_counts_add(fids.contiguous(), count, self._training_iterations(), num)

    def get_field_ids(self, min_iterations: Optional[int] = None) -> torch.Tensor:
        """NeuralGraphMap.get_field_ids (rm.py:2175-2181): the fields trained in at least min_iterations iterations (all
        fields for None).  The counts are kept only while track_training_iterations is set."""
        num = self._global_map_dict["num"]
        if min_iterations is None:
            return torch.arange(0, num, device=self._device)
        return torch.where(self._training_iterations()[:num] >= min_iterations)[0]

    def reserve_fields(self, max_fields: int) -> None:
        """Allocate the map ONCE for max_fields fields: every stacked parameter and its 16-bit copy (the model's
        reserve_fields), both Adam moments, positions, orientations, training_iterations, and `num_fields_dev`, a
        one-element int32 device tensor holding the number of fields.  The fields, moments, poses and counts the map holds
        are copied over.  all_fields_params, lp_fields_params, _optim_state and the pose tensors of _global_map_dict stay
        tensors of `num` rows -- leading-row views of the reservation -- and _global_map_dict["num"] stays the host mirror.
        add_fields(num_new, positions=, orientations=) then appends in place (one launch, no synchronisation) and
        sample_target_mv_device(current_count=, num_frames=), observed_fields_device and capture_training read
        num_fields_dev on the device: one captured graph keeps replaying while the map grows up to max_fields.
        Calling it again reallocates (a larger reservation): whatever was captured before must be captured again."""
        max_fields = int(max_fields)
        md = self._global_map_dict
        self._model.reserve_fields(max_fields)              # raises if the fields held do not fit
        num = self._model._reserved["num"]
        if md is not None and md["num"] != num:
            raise ValueError(f"reserve_fields: {md['num']} field poses but {num} fields")
        caps = self._model._reserved["params"]
        state = {k: {"exp_avg": torch.zeros_like(v), "exp_avg_sq": torch.zeros_like(v)} for k, v in caps.items()}
        if self._optim_state is not None:
            for k, st in self._optim_state.items():
                state[k]["exp_avg"][:num] = st["exp_avg"]
                state[k]["exp_avg_sq"][:num] = st["exp_avg_sq"]
        pdev = next(iter(caps.values())).device
        pos, quat = torch.zeros(max_fields, 3, device=pdev), torch.zeros(max_fields, 4, device=pdev)
        quat[:, 0] = 1.0
        ti = torch.zeros(max_fields, dtype=torch.int64, device=pdev)
        if md is not None:
            pos[:num], quat[:num] = md["positions"], md["orientations"]
            if md.get("training_iterations") is not None:
                ti[:num] = md["training_iterations"][:num]
        nfd = torch.zeros(1, dtype=torch.int32, device=pdev)
        nfd.fill_(num)
        self._reserve_epoch += 1
        self._reserved = dict(max=max_fields, epoch=self._reserve_epoch, state=state, positions=pos, orientations=quat,
                              training_iterations=ti, num_fields_dev=nfd)
        if self._anchor is not None:
            self._anchor = {k: self._anchor_rows(v, max_fields) for k, v in self._anchor.items()}
        self._set_num(num)

    def _set_num(self, num: int) -> None:
        """reserved mode: the public state as views of the first `num` rows (the model's own views are set by the model)"""
        rs = self._reserved
        self._optim_state = {k: {n: t[:num] for n, t in st.items()} for k, st in rs["state"].items()}
        self._global_map_dict = {"positions": rs["positions"][:num], "orientations": rs["orientations"][:num], "num": num,
                                 "training_iterations": rs["training_iterations"]}
        self._publish_kf_ids()

    def _append_reserved(self, num_new: int, positions, orientations) -> None:
        rs, m = self._reserved, self._model
        first = m._check_room(num_new)                      # ValueError before anything is touched
        pdev = rs["positions"].device
        if positions is None:
            positions = torch.zeros(num_new, 3, device=pdev)
        if orientations is None:
            orientations = torch.zeros(num_new, 4, device=pdev)
            orientations[:, 0] = 1.0
        if tuple(positions.shape) != (num_new, 3) or tuple(orientations.shape) != (num_new, 4):
            raise ValueError(f"add_fields({num_new}): positions must be ({num_new}, 3) and orientations ({num_new}, 4), got "
                             f"{tuple(positions.shape)} and {tuple(orientations.shape)}")
        positions = positions.to(device=pdev, dtype=torch.float32).contiguous()
        orientations = orientations.to(device=pdev, dtype=torch.float32).contiguous()
        if not rs["positions"].is_cuda:                    # CPU tensors: the bookkeeping without a GPU, plain torch
            m.add_fields(num_new)
            for st in rs["state"].values():
                st["exp_avg"][first:first + num_new] = 0.0
                st["exp_avg_sq"][first:first + num_new] = 0.0
            rs["positions"][first:first + num_new] = positions
            rs["orientations"][first:first + num_new] = orientations
            rs["training_iterations"][first:first + num_new] = 0
            rs["num_fields_dev"].fill_(first + num_new)
        else:                                              # one launch on the current stream (ngm_fields_append)
            mr = m._reserved
            proto = m._prototype_field.state_dict()
            tensors = [dict(param=mr["params"][k], exp_avg=rs["state"][k]["exp_avg"], exp_avg_sq=rs["state"][k]["exp_avg_sq"],
                            prototype=proto[k].detach().contiguous(), lp=None if mr["lp"] is None else mr["lp"].get(k))
                       for k in mr["params"]]
            ops.fields_append(tensors, positions, orientations, rs["positions"], rs["orientations"], rs["training_iterations"],
                              rs["num_fields_dev"], first)
            m._set_num(first + num_new)
        self._set_num(first + num_new)

    def add_fields(self, num_new: int, positions: Optional[torch.Tensor] = None, orientations: Optional[torch.Tensor] = None):
        """NeuralGraphMap._add_fields (rm.py:364-389): grow params + zero moments, keep the shared step.
        After reserve_fields the new fields are written IN PLACE into the next reserved rows -- parameters = the prototype,
        their 16-bit copy, zero moments, training_iterations 0, the given poses (positions (num_new, 3), orientations
        (num_new, 4) quaternions; omitted: origin / identity, to be followed by set_field_poses) -- and num_fields_dev is
        raised, on the GPU as one launch on the current stream without host synchronisation; beyond max_fields it raises
        ValueError and changes nothing."""
        if self._reserved is not None:
            return self._append_reserved(int(num_new), positions, orientations)
        if positions is not None or orientations is not None:
            raise ValueError("add_fields(positions=, orientations=) needs reserve_fields; without a reservation the poses "
                             "are the caller's tensors (set_field_poses)")
        self._model.add_fields(num_new)
        allp = self._model.all_fields_params
        new_state = {}
        for k, v in allp.items():
            m, s = torch.zeros_like(v), torch.zeros_like(v)
            if self._optim_state is not None:
                m[:-num_new] = self._optim_state[k]["exp_avg"]
                s[:-num_new] = self._optim_state[k]["exp_avg_sq"]
            new_state[k] = {"exp_avg": m, "exp_avg_sq": s}
        self._optim_state = new_state
        if self._anchor is not None:                        # the new fields belong to no keyframe yet
            self._anchor = {k: self._anchor_rows(v, v.shape[0] + num_new) for k, v in self._anchor.items()}
            self._publish_kf_ids()

    # -- fields anchored to keyframes (rm.py:844-952) ---------------------------------------------
    @staticmethod
    def _anchor_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
        """t extended to `rows` rows, the new ones unanchored (-1)"""
        out = torch.full((rows,), -1, dtype=t.dtype, device=t.device)
        out[:t.shape[0]] = t
        return out

    def _publish_kf_ids(self) -> None:
        """_global_map_dict["kf_ids"] (the reference's name): the anchors of the fields the dict describes, a view"""
        if self._anchor is not None and self._global_map_dict is not None:
            self._global_map_dict["kf_ids"] = self._anchor["kf_ids"][:self._global_map_dict["num"]]

    def anchor_fields(self, store, frame_ids, field_ids=None) -> None:
        """Attach fields to keyframes of `store` (a KeyframeStore): map_dict["kf_ids"] of the reference.  frame_ids: the frame
        id of the keyframe each given field belongs to, one per entry of field_ids (None: all fields, in order).  Sets
        _global_map_dict["kf_ids"] (int64) and the device table anchor_slot (int32: the keyframe's slot in the store, the
        row of its pose tables), which repose_fields reads.  After reserve_fields both have max_fields rows, allocated at the
        first call and written in place from then on; rows past `num` are unanchored (-1), and add_fields leaves new fields
        unanchored until they are given here.  A captured training graph reads neither."""
        md = self._global_map_dict
        if md is None:
            raise RuntimeError("anchor_fields: no fields yet (set_field_poses / reserve_fields first)")
        num, dev = md["num"], md["positions"].device
        fids = torch.arange(num) if field_ids is None else torch.as_tensor(field_ids, dtype=torch.int64).reshape(-1).cpu()
        kfs = torch.as_tensor(frame_ids, dtype=torch.int64).reshape(-1).cpu()
        if kfs.shape[0] != fids.shape[0]:
            raise ValueError(f"anchor_fields: {kfs.shape[0]} frame ids for {fids.shape[0]} fields")
        if fids.numel() and (int(fids.min()) < 0 or int(fids.max()) >= num):
            raise ValueError(f"anchor_fields: field ids must lie in [0, {num})")
        slot_of = {f: store.slot_of(f) for f in set(kfs.tolist())}          # ValueError for a frame that is no keyframe
        slots = torch.tensor([slot_of[f] for f in kfs.tolist()], dtype=torch.int32)
        if self._anchor is None:
            rows = num if self._reserved is None else self._reserved["max"]
            self._anchor = dict(kf_ids=torch.full((rows,), -1, dtype=torch.int64, device=dev),
                                slot=torch.full((rows,), -1, dtype=torch.int32, device=dev))
        elif self._anchor["kf_ids"].shape[0] < num:
            raise RuntimeError("anchor_fields: the anchors have fewer rows than the map (fields added behind the renderer's back)")
        idx = fids.to(dev)
        self._anchor["kf_ids"].index_copy_(0, idx, kfs.to(dev))
        self._anchor["slot"].index_copy_(0, idx, slots.to(dev))
        self._publish_kf_ids()

    def remove_keyframe(self, store, frame_id) -> None:
        """The SLAM front end culled keyframes (rm.py:907-929): every field anchored to a removed keyframe is rewired by the
        reference's rule -- to the next later keyframe that existed before this update, else to the closest earlier one
        (rm.py:918-921) -- by an in-place device write without synchronisation, then store.remove_keyframe runs.  Positions
        and orientations are not transformed (rm.py:928-929: the map holds absolute poses); the next repose_fields moves
        the rewired fields with their NEW keyframe.  frame_id: one frame id, or all the frame ids one update removes.  Call it
        before the update's own new keyframe is added to the store: every keyframe of the store counts as having existed."""
        removed = [int(f) for f in frame_id] if isinstance(frame_id, (list, tuple, set)) else [int(frame_id)]
        known = set(store.frame_ids)
        for f in removed:
            if f not in known:
                raise ValueError(f"remove_keyframe: frame {f} is not a keyframe of the store")
        new_kfs = known - set(removed)
        if not new_kfs:
            raise ValueError("remove_keyframe: no keyframe would be left to take the fields")
        for f in removed:
            kf_after = min((i for i in new_kfs if i >= f), default=None)
            new_anchor = kf_after if kf_after is not None else max(i for i in new_kfs if f >= i)
            if self._anchor is not None:
                kf, sl = self._anchor["kf_ids"], self._anchor["slot"]
                sl.masked_fill_(kf == f, store.slot_of(new_anchor))
                kf.masked_fill_(kf == f, new_anchor)
            store.remove_keyframe(f)

    def repose_fields(self, store) -> None:
        """NeuralGraphMap._update_field_poses (rm.py:937-952) after store.set_keyframe_poses: every anchored field moves with
        its keyframe, from the pose at the last re-pose (store.slot_c2w_prev) to the pose in force (store.slot_c2w), in
        place, as one ngm_fields_repose call on the current stream that also advances slot_c2w_prev -- no host
        synchronisation.  Fields whose keyframe did not move are not touched, bit for bit; unanchored fields and fields of
        a keyframe with a non-finite pose stay where they are.  With reserved rows the number of fields is read on the
        device.  Legal between replays of a capture_training graph: it reads the poses in place, and nothing it watches
        moves."""
        if self._anchor is None:
            raise RuntimeError("repose_fields: the fields belong to no keyframe (anchor_fields first)")
        rs, md = self._reserved, self._global_map_dict
        if rs is not None:
            pos, quat, nfd = rs["positions"], rs["orientations"], rs["num_fields_dev"]
        else:
            pos, quat, nfd = md["positions"], md["orientations"], None
        if self._anchor["slot"].shape[0] != pos.shape[0]:
            raise RuntimeError(f"repose_fields: {self._anchor['slot'].shape[0]} anchors for {pos.shape[0]} field poses")
        ops.fields_repose_(pos, quat, self._anchor["slot"], store.slot_c2w_prev, store.slot_c2w, num_fields_dev=nfd,
                           advance_prev=True)

    # -- new fields from a keyframe's depth (rm.py:265-345) -----------------------------------------
    COVER_DEFAULT_MAX_NEW = 4096           # cover_depth(max_new=None) without reserved rows

    def cover_depth(self, depth_or_rgbd, c2w, active_field_ids=None, shift=None, generator=None, max_new=None, camera=None):
        """Where NeuralGraphMap._extend_global_map_dict (rm.py:265-345) would put new fields for this keyframe: back-project
        the depth, drop the points within field_radius of an active field, snap the rest to a grid of edge 2 r / sqrt 3
        shifted by `shift`, drop the cells that hold an active field's centre, one field at the centre of every cell left.
        One ngm_cover_depth call on the current stream, no host synchronisation.
        depth_or_rgbd: (H, W) depth or (H, W, 4) r g b depth (a KeyframeStore slot is read in place); c2w (4, 4), on the
        device.  active_field_ids: int64 ids of the active fields (None: every field; entries < 0 or past the map are
        skipped, so padded lists pass).  shift=None draws torch.empty(3, device=...).uniform_(0.0, cell, generator=generator)
        on the device: the reference's own draw, from torch's generator.  max_new=None: the free reserved rows (at least 1),
        COVER_DEFAULT_MAX_NEW without a reservation.
        Returns (new_positions (max_new, 3) float32, counts (4,) int32 = num_new, status, uncovered valid pixels, valid
        pixels), see ops.cover_depth.  Deviations from the reference: pixels with a non-finite depth or world point are
        skipped (a lost pose adds nothing); its _bb_min / _bb_max, written and never read, are not kept."""
        cam = camera or self._camera
        fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
        rs, md = self._reserved, self._global_map_dict
        dev = depth_or_rgbd.device
        num = 0 if md is None else md["num"]
        if rs is not None:
            pos, free = rs["positions"], rs["max"] - num
        else:
            pos, free = (None if md is None else md["positions"].contiguous()), None
        if max_new is None:
            max_new = self.COVER_DEFAULT_MAX_NEW if free is None else max(free, 1)
        cell = ops.cover_cell(self._field_radius)
        if shift is None:
            shift = torch.empty(3, device=dev).uniform_(0.0, cell, generator=generator)
        ids = None
        if active_field_ids is not None:
            ids = torch.as_tensor(active_field_ids, dtype=torch.int64).reshape(-1).to(dev).contiguous()
            if rs is not None:                     # rows at or past `num` are reserved, not fields
                ids = torch.where(ids < num, ids, torch.full_like(ids, -1))
        c2w = c2w.to(device=dev, dtype=torch.float32).contiguous()
        shift = shift.to(device=dev, dtype=torch.float32).contiguous()
        return ops.cover_depth(depth_or_rgbd, c2w, shift, pos, self._field_radius, fx, fy, cx, cy, int(max_new), field_ids=ids,
                               num_active=None if ids is not None else num, cell=cell)

    def extend_map(self, depth_or_rgbd, frame_id, c2w, store=None, active_field_ids=None, shift=None, generator=None,
                   camera=None):
        """NeuralGraphMap._extend_global_map_dict (rm.py:265-345): cover this keyframe's depth with new fields and anchor
        them to it.  cover_depth, then ONE read-back of its 16-byte counts -- the number of fields and the `num`-row views
        of the map are host state, and an append whose count never leaves the device is a different change --, then
        add_fields(num_new, positions=...) with identity orientations (reserved rows: the one append launch; without a
        reservation add_fields(num_new) and set_field_poses of the concatenation), then, with `store`,
        anchor_fields(store, [frame_id] * num_new, field_ids=new ids) (rm.py:335, 343; frame_id must be a keyframe of it).
        Returns range(num_prev, num_prev + num_new); an empty range touches nothing.  More new fields than there is room
        for (reserved rows, or NGM_COVER_MAX_NEW), or a cell index outside (-2^20, 2^20), raises ValueError and changes
        nothing.  Legal between replays of a capture_training graph, exactly as add_fields is."""
        if store is not None:
            store.slot_of(frame_id)                # ValueError before anything happens
        md = self._global_map_dict
        num_prev = 0 if md is None else md["num"]
        room = None if self._reserved is None else self._reserved["max"] - num_prev
        new_positions, counts = self.cover_depth(depth_or_rgbd, c2w, active_field_ids=active_field_ids, shift=shift,
                                                 generator=generator, camera=camera)
        num_new, status = counts[:2].tolist()      # the one read-back
        if status == 2:
            raise ValueError("extend_map: a point of the depth image lies more than 2^20 grid cells from the origin")
        if status == 1 or (room is not None and num_new > room):
            left = f"{room} reserved rows are free" if room is not None else f"cover_depth's default max_new is {new_positions.shape[0]}"
            raise ValueError(f"extend_map: {num_new} new fields needed but {left}")
        if num_new == 0:
            return range(num_prev, num_prev)
        new_pos = new_positions[:num_new]
        if self._reserved is not None:
            self.add_fields(num_new, positions=new_pos)
        else:
            quat = torch.zeros(num_new, 4, device=new_pos.device)
            quat[:, 0] = 1.0
            old = None if md is None else (md["positions"], md["orientations"])
            self.add_fields(num_new)
            self.set_field_poses(new_pos.clone() if old is None else torch.cat((old[0], new_pos)),
                                 quat if old is None else torch.cat((old[1], quat)))
        new_ids = range(num_prev, num_prev + num_new)
        if store is not None:
            self.anchor_fields(store, [frame_id] * num_new, field_ids=list(new_ids))
        return new_ids

    # -- checkpoint interchange (rm.py:2147-2173) ------------------------------------------------
    def save_model(self, path: str) -> None:
        """torch.save of {map_dict, all_fields_params, state_dict}: the reference's checkpoint layout
        (optimizer moments are not saved there either); map_dict holds "kf_ids" only when anchor_fields set them.  With a
        peer exchange the health of every exchange so far is checked first: parameters trained behind a timed-out exchange
        are not written."""
        self.check_exchange()
        md, allp = self._global_map_dict, self._model.all_fields_params
        if self._reserved is not None:
            # torch.save of a view writes its whole storage (all max_fields rows): save contiguous copies of exactly `num` rows
            num = md["num"]
            md = {k: (v[:num].clone() if isinstance(v, torch.Tensor) else v) for k, v in md.items()}
            allp = {k: v.clone() for k, v in allp.items()}
        torch.save({"map_dict": md, "all_fields_params": allp, "state_dict": self._model.state_dict()}, path)

    def load_model(self, path: str) -> None:
        """Load a checkpoint of the reference's layout.  The tensors are allocated anew at the checkpoint's size, so a map
        with reserved rows LEAVES reserved mode (call reserve_fields again afterwards), and anything captured is stale."""
        self._reserved = self._model._reserved = None
        self._anchor = None                                 # a checkpoint's map_dict["kf_ids"] stays there: anchor_fields(store, them)
        ck = torch.load(path, map_location=self._device)
        self._model.load_state_dict(ck["state_dict"])
        self._model.all_fields_params = {k: v.to(self._device) for k, v in ck["all_fields_params"].items()}
        self._global_map_dict = ck["map_dict"]
        self._model.refresh_lp()
        self._optim_state = {k: {"exp_avg": torch.zeros_like(v), "exp_avg_sq": torch.zeros_like(v)}
                             for k, v in self._model.all_fields_params.items()}

    @torch.no_grad()
    def evaluate_points(self, points: torch.Tensor, block_size: Optional[int] = None) -> torch.Tensor:
        """kNN-blended field values at arbitrary world points (the dense-grid evaluation that
        _extract_mesh feeds to marching cubes, rm.py:2255-2261, 2320-2332), in blocks."""
        num = self._global_map_dict["num"]
        pos = self._global_map_dict["positions"][:num]
        quat = self._global_map_dict["orientations"][:num]
        params = self._model.kernel_params()
        m = self._model
        lead = points.shape[:-1]
        pts = points.reshape(-1, 3)
        block = int(block_size or self._config.get("block_size", 3000000))
        outs = [ops.field_eval_knn(self._fc, params, pts[s:s + block], pos, quat, m._num_knn, m._distance_factor,
                                   m._outside_value) for s in range(0, pts.shape[0], block)]
        return torch.cat(outs).reshape(*lead, 4)

    @torch.no_grad()
    def evaluate_grid(self, xs: torch.Tensor, ys: torch.Tensor, zs: torch.Tensor, channel: int = 3, negate: bool = False,
                      field_ids: Optional[torch.Tensor] = None, mask_radius: Optional[float] = None) -> torch.Tensor:
        """The lattice twin of evaluate_points: channel `channel` of the kNN-blended fields on xs x ys x zs as a
        (nx, ny, nz) volume, in one call (ngm_grid_eval_knn) -- evaluate_points(torch.cartesian_prod(xs, ys, zs))[:, channel]
        reshaped (and negated when `negate`), bit for bit.  `field_ids`: evaluate these fields only."""
        num = self._global_map_dict["num"]
        pos = self._global_map_dict["positions"][:num]
        quat = self._global_map_dict["orientations"][:num]
        fidx = None
        if field_ids is not None:
            fidx = field_ids.to(self._device).contiguous()
            pos, quat = pos[fidx].contiguous(), quat[fidx].contiguous()
        m = self._model
        return ops.grid_eval_knn(self._fc, m.kernel_params(), xs, ys, zs, pos, quat, m._num_knn, m._distance_factor,
                                 m._outside_value, fidx, mask_radius, channel, negate)

    def extract_mesh(self, mesh_file_path=None, resolution: Optional[float] = None, threshold: Optional[float] = None,
                     transform: Optional[torch.Tensor] = None, field_ids: Optional[torch.Tensor] = None, block: int = 200,
                     debug: Optional[dict] = None, fused: bool = True, stats: Optional[dict] = None):
        """_extract_mesh (rm.py:2186-2384): dense grid -> HIP marching cubes -> vertex colours -> PLY (see mesh.py)."""
        from . import mesh
        return mesh.extract_mesh(self, mesh_file_path, resolution, threshold, transform, field_ids, block, debug, fused, stats)

    def evaluate_mesh(self, gt, num_points: int = 200000, seed: int = 0, **extract_mesh_kwargs):
        """extract_mesh(**extract_mesh_kwargs) scored against the ground truth `gt` (a (verts, faces) pair of device tensors
        or a PLY path) by mesh.evaluate_mesh: the ten numbers of evaluation._evaluate_postprocessed_meshes
        (evaluation.py:163-208).  None where extract_mesh returns None (no surface)."""
        from . import mesh
        est = self.extract_mesh(**extract_mesh_kwargs)
        if est is None:
            return None
        return mesh.evaluate_mesh((est[0], est[1]), gt, num_points=num_points, seed=seed)

    def evaluate_raw_mesh(self, gt, c2ws, camera, gt_culling_method: str, est_culling_method: str, num_points: int = 200000,
                          seed: int = 0, bounds=None, mesh_alignment: bool = False, cull_kwargs: Optional[dict] = None,
                          align: Optional[str] = None, **extract_mesh_kwargs):
        """extract_mesh(**extract_mesh_kwargs) and the ground truth `gt`, both culled from the poses `c2ws` (OpenGL convention)
        seen through `camera`, then scored: mesh.evaluate_raw_mesh (evaluation.evaluate_raw_mesh, evaluation.py:211-251).
        cull_kwargs go to both mesh.cull_mesh calls (dict(max_edge=0.1): both meshes are subdivided first, as the reference
        does by default).  align="icp": the extracted mesh is aligned to the culled ground truth by point-to-plane ICP before
        it is culled (the reference's eval_mesh_alignment; mesh.align_mesh).  None where extract_mesh returns None (no surface)."""
        from . import mesh
        mesh._check_align(align)
        est = self.extract_mesh(**extract_mesh_kwargs)
        if est is None:
            return None
        return mesh.evaluate_raw_mesh((est[0], est[1]), gt, c2ws, camera, gt_culling_method, est_culling_method, num_points=num_points,
                                      seed=seed, bounds=bounds, mesh_alignment=mesh_alignment, align=align, **(cull_kwargs or {}))

    # -- reference-compatible API --------------------------------------------------------------
    def quadrature(self, sample_colors, sample_geometries, sample_distances, sample_depths, neus_isds=None):
        return ops.quadrature(self._rc_train, sample_colors, sample_geometries, sample_distances, sample_depths,
                              neus_isds)

    # -- train / eval sampling parameters (rm.py:1966-1974) ------------------------------------------
    def eval(self) -> None:
        """NeuralGraphMap.eval (rm.py:1966-1969): render_ijs / render_image sample `eval_num_samples` (configured, or derived
        from the training sample spacing, rm.py:199-207) in [eval_near_distance, eval_far_distance]."""
        self._mode = "eval"

    def train(self) -> None:
        """NeuralGraphMap.train (rm.py:1971-1974; the state a new map is in, :114): `num_samples_coarse` samples in
        [near_distance, far_distance]."""
        self._mode = "train"

    def _mode_sampling(self):
        """(_num_samples, _near_distance, _far_distance) of the current mode"""
        cfg = self._config
        if self._mode == "eval":
            return self.eval_num_samples(), cfg.get("eval_near_distance", 0.0), cfg.get("eval_far_distance", 8.0)
        return int(cfg["num_samples_coarse"]), cfg.get("near_distance", 0.0), cfg.get("far_distance", 8.0)

    def _rc_for(self, camera: Optional[Camera], guided: bool, overwrite: bool = True) -> K.RenderCfg:
        """ngm_render_cfg for `camera` (None: the constructor's) in the current mode; cached per (intrinsics, samples, flags)"""
        cam = camera or self._camera
        S, _, _ = self._mode_sampling()
        key = (cam.fx, cam.fy, cam.cx, cam.cy, S, bool(guided), bool(overwrite))
        rc = self._rc_cache.get(key)
        if rc is None:
            rc = make_render_cfg(cam, {**self._config, "num_samples_coarse": S}, guided=guided)
            rc.overwrite_behind_camera = int(bool(overwrite))
            self._rc_cache[key] = rc
        return rc

    def render_ijs(self, ijs, c2ws, camera=None, field_ids=None, use_vmap=False, near_distances=None,
                   far_distances=None, gt_distances=None, overwrite_samples_behind_camera=True, u_coarse=None,
                   u_guided=None, seed=0) -> Prediction:
        """NeuralGraphMap._render_ijs (rm.py:439-666), same arguments, same default branch.

        use_vmap=False (the default, rm.py:445): rays `ijs` (N,2) or (F,R,2) through the kNN-blended map -- all fields, or
        the subset `field_ids` (rm.py:502-508) --, `c2ws` (4,4) or per ray, optional per-ray near / far; with `gt_distances`
        and depth-guided samples configured, the second stratum + the free-space / TSDF vectors (rm.py:521-545, 624-639).
        Runs without autograd (stacked parameters are plain tensors in the reference too).
        use_vmap=True: the training branch, each ray row against ITS field; differentiable w.r.t. vmap_fields_params.
        `camera` is honoured on both (None = the constructor's camera); sample count and scalar near / far follow
        train() / eval().  Beyond the reference: `u_coarse` / `u_guided` replay the torch.rand draws of camera.py:274
        (shape (..., S)); otherwise the kernels draw from Philox with `seed`."""
        if use_vmap and field_ids is None:
            raise ValueError("field_ids=None only supported for use_vmap=False")                  # rm.py:497-498
        if not use_vmap:
            return self._render_ijs_knn(ijs, c2ws, camera, field_ids, near_distances, far_distances, gt_distances,
                                        overwrite_samples_behind_camera, u_coarse, u_guided, seed)
        self._model.set_vmap_fields(field_ids)
        for n, v in self._model.vmap_fields_params.items():
            if n not in K.NO_GRAD_PARAMS:                 # constants (hash shifts): no gradient, no Adam, no weight decay
                v.requires_grad_()
        _, near_c, far_c = self._mode_sampling()
        guided = gt_distances is not None and self._rc_train.num_samples_guided > 0
        # default True (rm.py:450); checked per sample
        rc = self._rc_for(camera, guided, overwrite_samples_behind_camera)
        pos = self._global_map_dict["positions"][field_ids]
        quat = self._global_map_dict["orientations"][field_ids]
        params = self._model.vmap_fields_params
        if rc.geometry_mode == K.GEO["neus"]:
            return self._render_ijs_staged(rc, ijs, c2ws, field_ids, near_distances, far_distances,
                                           gt_distances if guided else None, gt_distances, u_coarse,
                                           u_guided if guided else None, seed, overwrite_samples_behind_camera)
        rgbds, cvars, dvars, term, geoms, dists = ops.render_ijs_fused(
            self._fc, rc, params, ijs, c2ws, near_distances, far_distances, gt_distances if guided else None, pos, quat,
            u_coarse, u_guided if guided else None, seed, near_c, far_c)
        fs = ts = None
        tau = rc.truncation_distance
        if gt_distances is not None and geoms is not None:
            gt = gt_distances[..., None]
            if rc.w_freespace != 0.0:
                fs = geoms[dists < (gt - tau) * (gt != 0.0)] * tau                      # rm.py:624-630
            if rc.w_tsdf != 0.0:
                deltas = gt - dists
                m = (deltas.abs() < tau) & (gt != 0.0)
                ts = geoms[m] * tau - deltas[m]                                         # rm.py:632-639
        return Prediction(rgbds, cvars, dvars, term, fs, ts)

    @torch.no_grad()
    def _render_ijs_knn(self, ijs, c2ws, camera, field_ids, near, far, gt, overwrite, u_coarse, u_guided, seed,
                        params: Optional[dict] = None) -> Prediction:
        """_render_ijs(use_vmap=False) (rm.py:439-666 with :586-595): the rays are flattened to one row; without gt the
        whole call is ngm_render_eval_knn (samples, neighbour blend and quadrature in one pass over blocks of rays); with gt
        the per-sample geometry is needed for the free-space / TSDF vectors, so the staged entry points run
        (ngm_sample_rays_world -> ngm_field_eval_knn -> ngm_composite_fwd_packed), in blocks of `block_size` samples like
        the reference's batched_evaluation (rm.py:587-594)."""
        cfg, m, dev = self._config, self._model, self._device
        if self._rc_train.geometry_mode == K.GEO["neus"]:
            # rm.py:641-647 hands neus_isds=None to _quadrature on this branch, whose `None * float` raises (rm.py:754)
            raise TypeError("render_ijs(use_vmap=False) in geometry mode 'neus': the reference has no kNN branch for it "
                            "(neus_isds is None there, rm.py:641-647, 753-754); render with use_vmap=True")
        if ijs.dtype != torch.int64:
            raise TypeError("ijs must be int64 (row, col)")
        S, near_c, far_c = self._mode_sampling()
        n_g = int(cfg["num_samples_depth_guided"])
        guided = gt is not None and n_g > 0
        if guided and (near is None or far is None):
            # rm.py:522-526 compares the per-ray tensors with gt: None raises there as well
            raise TypeError("render_ijs: gt_distances with depth-guided samples needs per-ray near_distances and far_distances")
        lead = tuple(ijs.shape[:-1])
        N = 1
        for d in lead:
            N *= d
        flat = lambda t, *tail: None if t is None else t.reshape(N, *tail)
        ij, nr, fr, g = ijs.reshape(N, 2), flat(near), flat(far), flat(gt)
        if c2ws.dim() == 2:
            cw = c2ws
        else:
            cw = c2ws.expand(*lead, 4, 4).reshape(N, 4, 4)
        num = self._global_map_dict["num"]
        if field_ids is not None:                                                            # rm.py:502-508
            fids = field_ids.to(dev)
            pos, quat = self._global_map_dict["positions"][fids], self._global_map_dict["orientations"][fids]
        else:
            fids = None
            pos, quat = self._global_map_dict["positions"][:num], self._global_map_dict["orientations"][:num]
        if params is None:
            params = m.kernel_params()
        params = {k: v for k, v in params.items() if k != "_neus_sd"}
        rc = self._rc_for(camera, guided, overwrite)
        empty = lambda *shape: torch.empty(*shape, device=dev)
        if N == 0:
            fs = ts = None
            if gt is not None:
                fs = empty(0) if rc.w_freespace != 0.0 else None
                ts = empty(0) if rc.w_tsdf != 0.0 else None
            return Prediction(empty(*lead, 4), empty(*lead, 3), empty(*lead), empty(*lead), fs, ts)
        if gt is None and self.eval_fused:
            block = int(cfg.get("pixel_block_size", 8192))
            rb = int(cfg.get("eval_ray_block") or max(block, 32768))
            pred = self._fused_eval(lambda ray_block: ops.render_eval_knn(
                self._fc, rc, params, ij, cw, pos, quat, m._num_knn, m._distance_factor, m._outside_value, near=nr, far=fr,
                u=flat(u_coarse, S), seed=seed, near_const=near_c, far_const=far_c, field_index=fids, ray_block=ray_block),
                rb, block)
            if pred is not None:
                rgbd, cv, dv, term = pred
                return Prediction(rgbd.view(*lead, 4), cv.view(*lead, 3), dv.view(*lead), term.view(*lead), None, None)
        else:
            self.last_eval_path = "staged"
        St = S + (n_g if guided else 0)
        rays_per_block = max(1, int(cfg.get("block_size", 3000000)) // St)
        tau = rc.truncation_distance
        want_fs = gt is not None and rc.w_freespace != 0.0
        want_ts = gt is not None and rc.w_tsdf != 0.0
        behind = -100.0 if rc.geometry_mode in (K.GEO["occupancy"], K.GEO["density"]) else 1.0      # rm.py:614-622
        check_behind = overwrite and nr is not None and not bool((nr >= 0).all())                   # rm.py:494-495
        outs, fss, tss = [], [], []
        for s0 in range(0, N, rays_per_block):
            sl = slice(s0, s0 + rays_per_block)
            sub = lambda t: None if t is None else t[sl][None]
            pc, pw, dist = ops.sample_rays_world(rc, ij[sl][None], cw if cw.dim() == 2 else cw[sl][None], sub(nr), sub(fr),
                                                 sub(g) if guided else None, sub(flat(u_coarse, S)),
                                                 sub(flat(u_guided, n_g)) if guided else None, seed + s0,
                                                 near_const=near_c, far_const=far_c)
            out4 = ops.field_eval_knn(self._fc, params, pw.view(-1, 3), pos, quat, m._num_knn, m._distance_factor,
                                      m._outside_value, field_index=fids)
            dist, pc = dist.view(-1, St), pc.view(-1, St, 3)
            outs.append(ops.composite_packed(rc, out4, dist, pc))            # applies the behind-camera constant itself
            if want_fs or want_ts:
                geoms = out4.view(-1, St, 4)[..., 3]
                if check_behind:
                    geoms = torch.where(pc[..., 2] > 0, torch.full_like(geoms, behind), geoms)
                gg = g[sl][:, None]
                if want_fs:
                    fss.append(geoms[dist < (gg - tau) * (gg != 0.0)] * tau)             # rm.py:624-630
                if want_ts:
                    deltas = gg - dist
                    msk = (deltas.abs() < tau) & (gg != 0.0)
                    tss.append(geoms[msk] * tau - deltas[msk])                           # rm.py:632-639
        rgbd, cv, dv, term = (torch.cat([o[i] for o in outs]) for i in range(4))
        return Prediction(rgbd.view(*lead, 4), cv.view(*lead, 3), dv.view(*lead), term.view(*lead),
                          torch.cat(fss) if want_fs else None, torch.cat(tss) if want_ts else None)

    def _fused_eval(self, call, ray_block: int, min_block: int):
        """Run the fused evaluation call `call(ray_block)`; a block that does not fit (torch OOM, NGM_E_WORKSPACE) is halved
        down to `min_block`.  Returns None when the staged entry points must serve the call: the block cannot shrink
        further, or the library reports a shape the fused call does not support (NGM_E_UNSUPPORTED).  Every other error is
        raised.  Each distinct reason is recorded once in `eval_fallbacks`; `last_eval_path` names what ran."""
        rb = ray_block
        while True:
            try:
                out = call(rb)
                self.last_eval_path = f"fused, ray_block {rb}"
                return out
            except (K.NgmError, torch.cuda.OutOfMemoryError) as e:
                oom = isinstance(e, torch.cuda.OutOfMemoryError)
                code = getattr(e, "code", None)
                if not oom and code not in (K.NGM_E_WORKSPACE, K.NGM_E_UNSUPPORTED):
                    raise
                note = f"ray_block {rb}: {type(e).__name__}: {str(e)[:200]}"
                if note not in self.eval_fallbacks and len(self.eval_fallbacks) < 64:
                    self.eval_fallbacks.append(note)
                if oom:
                    torch.cuda.empty_cache()
                if rb <= min_block or code == K.NGM_E_UNSUPPORTED:
                    self.last_eval_path = "staged (fused call failed, see eval_fallbacks)"
                    return None
                rb = max(min_block, rb // 2)

    def _render_ijs_staged(self, rc, ijs, c2ws, field_ids, near, far, gt_sampler, gt, u_coarse, u_guided, seed,
                           overwrite_behind) -> Prediction:
        """_render_ijs as a chain of the standalone stages (sampler -> per-field evaluation -> quadrature), every stage
        an autograd function over its HIP kernels.  Serves the geometry mode the fused kernels do not: neus, whose
        occupancy couples neighbouring samples through the per-field learnable `_neus_sd` (rm.py:641-644, 753-758)."""
        params = self._model.vmap_fields_params
        pos = self._global_map_dict["positions"][field_ids]
        quat = self._global_map_dict["orientations"][field_ids]
        pc, pw, dists = ops.sample_rays_world(rc, ijs, c2ws, near, far, gt_sampler, u_coarse, u_guided, seed,
                                              near_const=self._config.get("near_distance", 0.0),
                                              far_const=self._config.get("far_distance", 8.0))
        F, R, S = dists.shape
        out = ops.field_eval(self._fc, {k: v for k, v in params.items() if k != "_neus_sd"}, pw.reshape(F, R * S, 3),
                             pos, quat).view(F, R, S, 4)
        colors = rc.color_factor * out[..., :3]                                              # rm.py:610
        geoms = out[..., 3]
        depths = -pc[..., 2]                                                                  # rm.py:612
        if overwrite_behind and near is not None and not bool((near >= 0).all()):             # rm.py:494-495
            const = -100.0 if rc.geometry_mode in (K.GEO["occupancy"], K.GEO["density"]) else 1.0   # rm.py:614-622
            geoms = torch.where(pc[..., 2] > 0, torch.full_like(geoms, const), geoms)
        isds = None
        if rc.geometry_mode == K.GEO["neus"]:
            isds = 1.0 / torch.abs(params["_neus_sd"].view(-1, 1, 1))                         # rm.py:641-644
        C, D, Cv, Dv, term, _ = ops.quadrature(rc, colors, geoms, dists, depths, isds)
        fs = ts = None
        tau = rc.truncation_distance
        if gt is not None:
            g = gt[..., None]
            if rc.w_freespace != 0.0:
                fs = geoms[dists < (g - tau) * (g != 0.0)] * tau                              # rm.py:624-630
            if rc.w_tsdf != 0.0:
                deltas = g - dists
                m = (deltas.abs() < tau) & (g != 0.0)
                ts = geoms[m] * tau - deltas[m]                                               # rm.py:632-639
        return Prediction(torch.cat([C, D[..., None]], -1), Cv, Dv, term, fs, ts)

    def optimization_iteration_staged(self, target: Target, u_coarse=None, u_guided=None, seed=0, update=True) -> dict:
        """The training iteration for configurations outside the fused kernels (geometry mode neus): staged render,
        torch loss, autograd through the stage kernels, the same sparse Adam (incl. `_neus_sd`)."""
        fids = target.field_ids
        pred = self.render_ijs(target.ijs, target.c2ws, field_ids=fids, use_vmap=True, near_distances=target.near_distances,
                               far_distances=target.far_distances, gt_distances=target.gt_distances,
                               u_coarse=u_coarse, u_guided=u_guided, seed=seed)
        loss = self.compute_losses(target, pred)
        params = self._model.vmap_fields_params
        names = [n for n, v in params.items() if v.requires_grad and n not in K.NO_GRAD_PARAMS]
        grads = torch.autograd.grad(loss["combined"], [params[n] for n in names], allow_unused=True)
        gd = {n: (g if g is not None else torch.zeros_like(params[n])) for n, g in zip(names, grads)}
        out = {k: v.detach() for k, v in loss.items()}
        out["prediction"] = pred
        if not update:
            out["grads"] = gd
            return out
        self._step += 1
        with torch.no_grad():
            for n in names:
                allp = self._model.all_fields_params[n]
                st = self._optim_state[n]
                ops.adam_sparse_(allp, st["exp_avg"], st["exp_avg_sq"], gd[n].contiguous(), fids, self._step,
                                 lr=self._learning_rate, eps=self._adam_eps, weight_decay=self._adam_weight_decay)
        if self._step_dev is not None:
            self._step_dev.fill_(self._step)
        self._model.refresh_lp()           # this path updates the fp32 masters tensor by tensor
        self._count_training_iteration(fids, None)
        return out

    def compute_losses(self, target: Target, prediction: Prediction) -> dict:
        """_compute_losses (rm.py:1769-1872) on torch tensors; loss dict keys carry the mode like rm.py:1827, 1837."""
        rc = self._rc_train
        pk = "photometric_" + self._config["photometric_loss"]
        m = target.depth_mask & (prediction.term_probs > rc.term_threshold)
        loss = {}
        tm = target.term_mask
        loss["termination"] = ((prediction.term_probs[tm] - target.term_probs[tm]) ** 2).mean()
        diff = target.rgbds[m][:, :3] - prediction.rgbds[m][:, :3]
        dk = "depth_" + self._config["depth_loss"]
        p_d, t_d = prediction.rgbds[m][:, 3], target.rgbds[m][:, 3]
        if rc.photometric_mode == K.PHOTO["gaussian_nll"]:                   # losses.py:30-36 (the autograd path propagates
            cv = prediction.color_vars[m]                                     # through the variances: render_ijs_bwd with seeds on them)
            nlls = 0.5 * diff ** 2 / cv + torch.log(torch.sqrt(cv))
            loss[pk] = diff.abs().mean() if nlls.mean() > 2 else nlls.mean()
        else:
            loss[pk] = diff.abs().mean() if rc.photometric_mode == K.PHOTO["l1"] else (diff ** 2).mean()   # losses.py:26-29
        if rc.depth_mode == K.DEPTH["gaussian_nll"]:                         # losses.py:64-69
            dv = prediction.depth_vars[m] + 1e-15
            loss[dk] = (0.5 * (p_d - t_d) ** 2 / dv + torch.log(torch.sqrt(dv))).mean()
        elif rc.depth_mode == K.DEPTH["laplacian_nll"]:                      # losses.py:70-75
            dv = prediction.depth_vars[m]
            loss[dk] = ((t_d - p_d).abs() / torch.sqrt(0.5 * dv + 1e-6) + 0.5 * torch.log(2 * dv + 1e-6)).mean()
        else:
            loss[dk] = torch.nn.functional.huber_loss(p_d, t_d, delta=rc.huber_delta)
        total = (rc.w_termination * loss["termination"] + rc.w_photometric * loss[pk]
                 + rc.w_depth * loss[dk])
        if prediction.freespace_geometry is not None:
            loss["freespace"] = ((prediction.freespace_geometry - rc.truncation_distance) ** 2).mean()
            total = total + rc.w_freespace * loss["freespace"]
        if prediction.tsdf_residuals is not None:
            loss["tsdf"] = (prediction.tsdf_residuals ** 2).mean()
            total = total + rc.w_tsdf * loss["tsdf"]
        loss["combined"] = total
        return loss

    # -- training-target sampler (rm.py:1259-1459) ------------------------------------------------
    @torch.no_grad()
    def sample_target_mv(self, current_field_ids, c_c2w, nc_rgbd, frame_cid_to_ncid, num_train_fields, num_rays_per_field,
                         num_fields=None, camera: Optional[Camera] = None, draws: Optional[dict] = None,
                         field_draw: str = "reference", world_size: int = 1) -> Target:
        """NeuralGraphMap._sample_target_mv: choose the fields to train, find the keyframes that see them, sample
        keyframes and pixels, collect the RGB-D supervision.  State that the reference keeps on `self` is passed in:
        c_c2w (Nc,4,4) = _c_c2w_tensor, nc_rgbd (N,H,W,4) = _nc_rgbd_tensor, frame_cid_to_ncid (Nc,).
        The random draws are made with torch on this device in the reference's order (multinomial, multinomial,
        randn, multinomial, rand); `draws` (dict: subset_observed, subset_random, offsets, frame_cids, u_xy)
        replays recorded ones.  The geometry between the draws runs in two HIP kernels.
        field_draw="balanced_by_owner" (opt-in, with world_size) replaces the choice of fields by
        distributed.draw_fields_balanced: the same draw per owner rank with a quota of num_train_fields / world -- every
        rank trains equally many fields per iteration; not the reference's distribution, see DESIGN.md §7."""
        if field_draw not in ("reference", "balanced_by_owner"):
            raise NotImplementedError(f"field_draw={field_draw!r}: 'reference' or 'balanced_by_owner'")
        cam = camera or self._camera
        dev = self._device
        radius = self._field_radius + 0.0
        num_fields = self._global_map_dict["num"] if num_fields is None else num_fields
        d = draws or {}
        cur = current_field_ids.to(dev)
        if field_draw == "balanced_by_owner" and world_size > 1 and not draws:
            from . import distributed as D
            # every rank must draw the SAME set: a dedicated generator, seeded identically everywhere and consumed by nothing
            # else (the process-global CUDA stream also feeds the per-rank ray draws below, whose consumption may differ
            # between ranks -- sharded / early-exit sampling -- and would silently desynchronise the active sets)
            if self.field_draw_generator is None:
                self.field_draw_generator = torch.Generator(device="cpu").manual_seed(0x5EED0F1E1D5)
            field_ids = D.draw_fields_balanced(cur.cpu(), num_fields, num_train_fields, world_size,
                                               generator=self.field_draw_generator).to(dev)
            if getattr(self, "debug_check_field_draw", False) and self.process_group is not None:
                ref = field_ids.clone()
                torch.distributed.broadcast(ref, 0, group=self.process_group)
                assert torch.equal(ref, field_ids), "balanced_by_owner: ranks drew different active sets"
        else:                                                      # rm.py:1280-1319
            n_obs = min(num_train_fields // 2, len(cur))
            sub_obs = d["subset_observed"].to(dev) if draws else torch.multinomial(torch.ones(len(cur), device=dev), n_obs)
            obs_ids = cur[sub_obs]
            n_rand = min(num_train_fields - len(obs_ids), num_fields - len(obs_ids))
            if n_rand > 0:
                dist = torch.ones(num_fields, device=dev)
                dist[obs_ids] = 0.0
                sub_rand = d["subset_random"].to(dev) if draws else torch.multinomial(dist, n_rand)
                field_ids = torch.unique(torch.cat((torch.arange(num_fields, device=dev)[sub_rand], obs_ids)))
            else:
                field_ids = obs_ids
        pos_w = self._global_map_dict["positions"][field_ids].contiguous()
        if draws:
            offsets = d["offsets"].to(dev)
        else:
            offsets = torch.randn((20, 3), device=dev)
            offsets /= torch.linalg.norm(offsets, dim=-1, keepdim=True)
        fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
        kf = ops.keyframes_struct(c_c2w.contiguous(), nc_rgbd, frame_cid_to_ncid, fx, fy, cx, cy)
        kf_mask, bbox = ops.target_visibility(kf, pos_w, offsets, radius)
        fmask = kf_mask.any(-1)                                    # fields no keyframe sees are dropped (rm.py:1365-1379)
        kf_mask, field_ids, pos_w, bbox = kf_mask[fmask], field_ids[fmask], pos_w[fmask].contiguous(), bbox[fmask].contiguous()
        F, R = len(field_ids), num_rays_per_field
        frame_cids = d["frame_cids"].to(dev) if draws else torch.multinomial(kf_mask.float(), R, replacement=True)
        u_xy = d["u_xy"].to(dev) if draws else torch.rand(F, R, 2, device=dev)
        o = ops.target_rays(kf, pos_w, radius, bbox, frame_cids, u_xy)
        return Target(ijs=o["ijs"], c2ws=o["c2ws"], near_distances=o["near"], far_distances=o["far"],
                      gt_distances=o["gt"], field_ids=field_ids, rgbds=o["rgbds"], rgb_mask=o["rgb_mask"],
                      depth_mask=o["depth_mask"], term_probs=o["term_probs"], term_mask=o["term_mask"])

    @torch.no_grad()
    def sample_target_mv_device(self, current_field_ids, c_c2w, nc_rgbd, frame_cid_to_ncid, num_train_fields, num_rays_per_field,
                                num_fields=None, camera: Optional[Camera] = None, seed: int = 0, iteration: Optional[int] = None,
                                world_size: int = 1, rank: int = 0, *, current_count: Optional[torch.Tensor] = None,
                                num_frames: Optional[torch.Tensor] = None) -> DeviceTarget:
        """sample_target_mv with every draw made on the device (ngm_target_sample_mv: three kernels, no host synchronisation,
        no data-dependent shapes), so it can be captured in a graph.  Same distribution as the reference's sampler, NOT the
        same random numbers: the draws come from Philox4x32-10 keyed by (seed, iteration) -- the field draw and offsets by
        those alone, ray k of field g by (seed, iteration, g, k) -- not from torch's generator.
        iteration=None: a device counter owned by this renderer is read and advanced by the call (a graph replay draws the
        next iteration's targets); an int uses that iteration and leaves the counter alone.
        world_size / rank: every rank draws the same fields; rows are made only for drawn fields with id % world_size == rank
        (distributed.field_owner), in draw order, bit for bit the single-process rows of those fields.
        Precondition (not checked: that would synchronise): current_field_ids is duplicate-free, ids in [0, num_fields), as
        the reference's is.  Returns a DeviceTarget; .materialize() gives the Target for optimization_iteration.
        current_count / num_frames (both or neither; one-element int32 device tensors): the live sampler
        (ngm_target_sample_mv_live) -- current_field_ids, c_c2w and frame_cid_to_ncid are then fixed-capacity buffers
        (observed_fields_device and KeyframeStore fill such), only their first current_count / num_frames entries are read,
        and the result is bit for bit that of this call on the sliced tensors: the shapes no longer follow the frame, so a
        captured graph outlives it.  Returns a LiveDeviceTarget.
        After reserve_fields the live sampler also reads the NUMBER OF FIELDS on the device (ngm_target_sample_mv_grow,
        num_fields_dev): current_field_ids then has at most max_fields entries, the row capacity is the host-known
        min(num_train_fields, fields this rank owns among max_fields), and rows below `count` are bit for bit those of an
        unreserved map of exactly `num` fields.  Without current_count the call uses the host's `num` as before."""
        if (current_count is None) != (num_frames is None):
            raise ValueError("sample_target_mv_device: current_count and num_frames go together (both device tensors, or neither)")
        cam = camera or self._camera
        dev = self._device
        rs = self._reserved if current_count is not None else None      # reserved rows + live counts: the grow entry point
        if rs is not None:
            if num_fields is not None and int(num_fields) != self._global_map_dict["num"]:
                raise ValueError("sample_target_mv_device: with reserved field rows the number of fields is read on the device "
                                 "(num_fields_dev); leave num_fields=None")
            num_fields = rs["max"]
        num_fields = self._global_map_dict["num"] if num_fields is None else num_fields
        cur = current_field_ids if current_field_ids.device == torch.device(dev) else current_field_ids.to(dev)
        if cur.dtype != torch.int64:
            cur = cur.long()
        counter = None
        if iteration is None:
            if self._target_iter_dev is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("sample_target_mv_device: call it once outside the graph capture first (or pass "
                                       "iteration=...): the device iteration counter must exist before the capture")
                self._target_iter_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            counter = self._target_iter_dev
        fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
        views = [cur.contiguous(), c_c2w.contiguous()]
        if current_count is not None:
            views = [views[0], current_count, views[1], num_frames]
        sampler = ops.target_sample_mv if current_count is None else ops.target_sample_mv_live
        positions = self._global_map_dict["positions"].contiguous()
        if rs is not None:
            sampler, positions = ops.target_sample_mv_grow, rs["positions"]
            views.append(rs["num_fields_dev"])
        o = sampler(*views, nc_rgbd.contiguous(), frame_cid_to_ncid.contiguous(), positions,
                    fx, fy, cx, cy, self._field_radius + 0.0, int(num_fields), int(num_train_fields), int(num_rays_per_field),
                    seed=seed, iteration=iteration, iteration_dev=counter, world_size=world_size, rank=rank)
        return DeviceTarget.from_sampler(o, world_size)

    @torch.no_grad()
    def observed_fields_device(self, rgbd_image, c2w, num_points: int = 500, seed: int = 0, frame: Optional[int] = None,
                               out=None, draws: Optional[dict] = None, camera: Optional[Camera] = None):
        """NeuralGraphMap._get_observed_fields (rm.py:1642-1670) on the device (ngm_target_observed_fields): which fields
        does this RGB-D frame see?  No host synchronisation and fixed shapes -- returns (ids, count): ids (num_fields,)
        int64, the observed field ids ascending with -1 past count, a one-element int32 device tensor; exactly what
        sample_target_mv_device(current_count=...) and capture_training read.  out=(ids, count) writes into given tensors
        (the buffers a captured graph keeps reading).  rgbd_image (H, W, 4) and c2w (4, 4) are device tensors.
        Same distribution as the reference's multinomial draw of num_points valid pixels, NOT torch's random numbers:
        Philox keyed by (seed, frame); frame=None reads and advances a device counter owned by this renderer.
        draws=dict(pixels=...) replays num_points recorded linear pixel indices instead.  The chosen pixels and their
        number are kept in `last_observed` (device tensors)."""
        cam = camera or self._camera
        dev = self._device
        counter = None
        if frame is None:
            if self._observe_frame_dev is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("observed_fields_device: call it once outside the graph capture first (or pass frame=...)")
                self._observe_frame_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            counter = self._observe_frame_dev
        ids_out, count_out = out if out is not None else (None, None)
        fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
        rs = self._reserved            # reserved rows: ids (max_fields,), the fields tested = num_fields_dev, read on the device
        positions = self._global_map_dict["positions"].contiguous() if rs is None else rs["positions"]
        o = ops.target_observed_fields(rgbd_image, c2w, positions, fx, fy, cx, cy, self._field_radius + 0.0,
                                       int(self._global_map_dict["num"] if rs is None else rs["max"]), num_points=num_points,
                                       seed=seed, frame=frame, frame_dev=counter,
                                       subset_in=None if draws is None else draws["pixels"], ids_out=ids_out, count_out=count_out,
                                       num_fields_dev=None if rs is None else rs["num_fields_dev"])
        self.last_observed = dict(pixels=o["pixels"], num_used=o["num_used"])
        return o["current_field_ids"], o["current_count"]

    def sample_target_sv(self, rgbd_image, c2w, active_field_ids, num_train_fields, num_rays_per_field,
                         camera: Optional[Camera] = None, draws: Optional[dict] = None, num_points: int = 50000) -> Target:
        """NeuralGraphMap._sample_target_sv (`update_mode: single_view`, rm.py:1461-1583): fields and rays from ONE RGB-D
        frame.  The depth image is back-projected, `num_points` (50 000 in the reference) of its points are drawn, fields
        whose sphere is crossed by at least num_rays_per_field of the segments camera -> point are candidates, rays are
        drawn among each field's crossing segments.  The three torch.multinomial draws are made on this device in the
        reference's order; `draws` (dict: subset_points, subset_fields, segments) replays recorded ones.  The
        segment-sphere test (fields x points) and the per-ray targets run in two HIP kernels."""
        cam = camera or self._camera
        dev = self._device
        radius = self._field_radius + 0.0
        d = draws or {}
        rgbd_image = rgbd_image.to(dev).contiguous()
        c2w = c2w.to(dev)
        active = active_field_ids.to(dev)
        pos_w = self._global_map_dict["positions"][active]
        pos_c = (pos_w - c2w[:3, 3]) @ c2w[:3, :3]                          # utils.transform_points(..., inv=True): R^T (p - t)
        fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
        depth = rgbd_image[..., 3]
        ijs = torch.nonzero(depth)                                         # camera.py:374: only pixels with depth
        dv = depth[ijs[:, 0], ijs[:, 1]]
        points = torch.stack(((ijs[:, 1].float() - cx) * dv / fx, -(ijs[:, 0].float() - cy) * dv / fy, -dv), -1)
        sub = d["subset_points"].to(dev) if draws else torch.multinomial(torch.ones(len(points), device=dev), num_points)
        points, ijs = points[sub].contiguous(), ijs[sub].contiguous()
        mins, maxs = points.min(0)[0], points.max(0)[0]
        aabb_mask = ((pos_c - radius) <= maxs).all(-1) & ((pos_c + radius) >= mins).all(-1)
        pos_in = pos_c[aabb_mask].contiguous()
        hit = ops.target_sv_intersect(pos_in, points, radius)
        seg_mask = hit.sum(-1) >= num_rays_per_field
        hit = hit[seg_mask]
        ids, pc = active[aabb_mask][seg_mask], pos_in[seg_mask]
        if len(hit) > num_train_fields:
            sf = d["subset_fields"].to(dev) if draws else torch.multinomial(torch.ones(len(hit), device=dev), num_train_fields)
            ids, pc, hit = ids[sf], pc[sf], hit[sf]
        segments = d["segments"].to(dev) if draws else torch.multinomial(hit.float(), num_rays_per_field)
        o = ops.target_sv_rays(pc.contiguous(), radius, ijs, segments, rgbd_image, fx, fy, cx, cy)
        return Target(ijs=o["ijs"], c2ws=c2w, near_distances=o["near"], far_distances=o["far"], gt_distances=o["gt"],
                      field_ids=ids, rgbds=o["rgbds"], rgb_mask=o["rgb_mask"], depth_mask=o["depth_mask"],
                      term_probs=o["term_probs"], term_mask=o["term_mask"])

    def sample_target_sv_device(self, rgbd, c2w, active_field_ids, num_train_fields, num_rays_per_field, num_points: int = 50000,
                                seed: int = 0, iteration: Optional[int] = None, world_size: int = 1, rank: int = 0,
                                camera: Optional[Camera] = None, slot: Optional[torch.Tensor] = None,
                                draws: Optional[dict] = None) -> DeviceTarget:
        """sample_target_sv with every draw made on the device (ngm_target_sample_sv: no host synchronisation, no
        data-dependent shape, no hit matrix in memory), so it can be captured in a graph.  Same distribution as the
        reference's sampler, NOT the same random numbers: Philox4x32-10 keyed by (seed, iteration) -- the points by pixel,
        the fields by field id, the rays of field g by (g, pixel) -- so a row depends on (seed, iteration, frame, g) only.
        rgbd (H, W, 4) with c2w (4, 4), or a frame stack (S, H, W, 4) / (S, 4, 4) with slot (one-element int32 device tensor):
        the frame clamp(slot, 0, S - 1) is read, so a captured graph changes frames by a 4-byte device write.
        active_field_ids (A,) int64, duplicate-free; entries < 0 or past the number of fields are skipped (a fixed-length
        buffer padded with -1 works).  iteration=None: the renderer's device iteration counter is read and advanced by the
        call (call once outside a capture first); an int uses that iteration and leaves the counter alone.
        world_size / rank: every rank makes the same draw; rows are made only for drawn fields with id % world_size == rank.
        With reserved rows (reserve_fields) the reserved positions are read and the number of fields comes from the device.
        draws=dict(pixels=, subset_fields=, segments=): recorded draws instead (pixels: num_points linear pixel indices in
        order; subset_fields: T positions in the candidate list, used when there are more than T candidates; segments:
        (rows, R) indices into pixels); any of them may be missing, segments needs pixels.
        Returns an SvDeviceTarget with min(T, A, fields of this rank) rows, `count` of them valid."""
        cam = camera or self._camera
        dev = self._device
        counter = None
        if iteration is None:
            if self._target_iter_dev is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("sample_target_sv_device: call it once outside the graph capture first (or pass "
                                       "iteration=...): the device iteration counter must exist before the capture")
                self._target_iter_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            counter = self._target_iter_dev
        act = active_field_ids if active_field_ids.device == torch.device(dev) else active_field_ids.to(dev)
        if act.dtype != torch.int64:
            act = act.long()
        rs = self._reserved
        positions = self._global_map_dict["positions"].contiguous() if rs is None else rs["positions"]
        num_fields = int(self._global_map_dict["num"] if rs is None else rs["max"])
        T, R = int(num_train_fields), int(num_rays_per_field)
        d = {k: (None if v is None else v.to(dev).long().contiguous()) for k, v in (draws or {}).items()}
        capacity = K.target_sample_sv_plan(act.shape[0], num_fields, T, R, int(num_points), int(world_size), int(rank))
        seg = d.get("segments")
        if seg is not None and seg.shape[0] < capacity:                   # recorded rows: the fields that survived
            seg = torch.cat([seg, seg.new_zeros(capacity - seg.shape[0], seg.shape[1])])
        fx, fy, cx, cy, _ = cam.get_pinhole_camera_parameters(0.0)
        o = ops.target_sample_sv(rgbd, c2w, act.contiguous(), positions, fx, fy, cx, cy, self._field_radius + 0.0, num_fields, T, R,
                                 num_points=num_points, seed=seed, iteration=iteration, iteration_dev=counter,
                                 world_size=world_size, rank=rank, slot=slot,
                                 num_fields_dev=None if rs is None else rs["num_fields_dev"], capacity=capacity,
                                 pixels_in=d.get("pixels"), subset_fields_in=d.get("subset_fields"), segments_in=seg)
        return SvDeviceTarget(o, world_size, rgbd, slot, T)

    def capture_training_sv(self, rgbd, c2w, active_field_ids, num_train_fields, num_rays_per_field, num_points: int = 50000,
                            seed=0, camera: Optional[Camera] = None, world_size: int = 1, rank: int = 0, *,
                            slot: Optional[torch.Tensor] = None):
        """capture_training for `update_mode: single_view`: sample_target_sv_device(iteration=None) followed by the counted
        optimization_iteration on its target, as ONE captured graph.  Returns a callable like capture_training's (`.target`,
        `.graph`).  rgbd, c2w, active_field_ids and slot are READ IN PLACE at every replay: write a new frame into the
        stack, rewrite `slot` or the (fixed-length, -1 padded) active_field_ids between replays freely; their shapes and
        storage, the number of fields and the stacked parameters must stay (the same host check, the same "capture again"
        error) -- or, after reserve_fields, the reservation, and add_fields between replays is legal."""
        why = self.counted_step_unsupported()
        if why is not None:
            raise RuntimeError(f"capture_training_sv: {why} is outside the counted step (optimization_iteration would fall "
                               "back to DeviceTarget.materialize(), which synchronises)")
        named = dict(rgbd=rgbd, c2w=c2w, active_field_ids=active_field_ids)
        if slot is not None:
            named["slot"] = slot
        for n, t in named.items():
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"capture_training_sv: {n} must be a contiguous device tensor (it is read in place at every replay)")
        if active_field_ids.dtype != torch.int64:
            raise TypeError("capture_training_sv: active_field_ids must be int64")
        if slot is not None and slot.dtype != torch.int32:
            raise TypeError("capture_training_sv: slot must be int32")

        def sample():
            return self.sample_target_sv_device(rgbd, c2w, active_field_ids, num_train_fields, num_rays_per_field,
                                                num_points=num_points, seed=seed, iteration=None, world_size=world_size, rank=rank,
                                                camera=camera, slot=slot)
        return self._capture_sampled("capture_training_sv", named, sample, self._reserved is not None,
                                     self._global_map_dict["num"], seed)

    # -- eval path: render_image / PSNR (rm.py:402-437, 1966-2000; evaluation.py:46-56) ----------
    def eval_num_samples(self) -> int:
        """rm.py:199-207: derived from the training sample spacing unless configured."""
        cfg = self._config
        if cfg.get("eval_num_samples") is not None:
            return int(cfg["eval_num_samples"])
        n_g = cfg.get("num_samples_depth_guided", 0)
        tau = cfg.get("truncation_distance", 0.1)
        rho = cfg.get("range_depth_guided") or tau
        spacing = 2 * rho / n_g if n_g > 0 else 2 * self._field_radius / cfg["num_samples_coarse"]
        return int((cfg.get("eval_far_distance", 8.0) - cfg.get("eval_near_distance", 0.0)) / spacing)

    @torch.no_grad()
    def render_pixels(self, c2w: torch.Tensor, begin: int, end: int, params: Optional[dict] = None,
                      camera: Optional[Camera] = None, u: Optional[torch.Tensor] = None, seed: int = 0):
        """Pixels [begin, end) of the flattened (row-major) image, single stratum, kNN-blended fields (the loop body of
        render_image, rm.py:402-437 = _render_ijs(x, c2w, camera) per block); sample count and near / far of the current
        mode (call eval() first, as rm.py:1879, 1978 do).  `params` overrides the model's stacked parameters (the
        all-gathered set on a sharded map).  Returns (rgbds (n,4), depth_vars (n,))."""
        cam = camera or self._camera
        cfg = self._config
        S, near_c, far_c = self._mode_sampling()
        rc = self._rc_for(cam, False)
        w = cam.width
        dev = self._device
        idx = torch.arange(begin, end, device=dev)
        ijs = torch.stack((idx // w, idx % w), -1)
        num = self._global_map_dict["num"]
        pos = self._global_map_dict["positions"][:num]
        quat = self._global_map_dict["orientations"][:num]
        if params is None:
            params = self._model.kernel_params()
        params = {k: v for k, v in params.items() if k != "_neus_sd"}
        m = self._model
        block = int(cfg.get("pixel_block_size", 8192))
        if self.eval_fused:
            # the whole loop below as one call (ngm_render_eval_knn): same blocks, same draws, same arithmetic; the samples,
            # the blended field outputs and the camera-frame points stay out of memory.  `eval_ray_block` = rays per internal
            # block (default: max(pixel_block_size, 32768) -- the reference chunks at 8192 pixels to bound ITS memory; the
            # pair records of 32768 x 640 samples are 1.3 GB here, and larger blocks mean fewer launches and shorter tails:
            # 14.3 -> 13.1 ms per 640-sample image, 5.8 -> 4.2 ms at 128 samples).  The in-kernel jitter stream is seeded
            # per block, so the block size decides WHICH draws a pixel gets (not their distribution; explicit `u` is
            # unaffected); with eval_ray_block = pixel_block_size the image equals the staged loop below bit for bit.
            # Memory: the transient workspace grows with the block (about 1.2 GB at S = 640, K = 2; 3.7 GB at S = 1024, K = 4).  A
            # block that does not fit (torch OOM, NGM_E_WORKSPACE) is halved down to the reference's pixel_block_size; if even
            # that fails -- or the library reports a shape the fused call does not support (NGM_E_UNSUPPORTED) -- the staged
            # loop below runs, as it would have with eval_fused = False; any other error is raised.  A fall-back is recorded
            # once per reason (`eval_fallbacks`), never silent about WHICH path ran: `last_eval_path`.
            rb = int(cfg.get("eval_ray_block") or max(block, 32768))
            pred = self._fused_eval(lambda ray_block: ops.render_eval_knn(
                self._fc, rc, params, ijs, c2w, pos, quat, m._num_knn, m._distance_factor, m._outside_value,
                u=None if u is None else u[begin:end], seed=seed + begin, near_const=near_c, far_const=far_c,
                ray_block=ray_block), rb, block)
            if pred is not None:
                return pred[0], pred[2]
        else:
            self.last_eval_path = "staged"
        rgbds, dvars = [], []
        for s0 in range(0, ijs.shape[0], block):
            ij = ijs[s0:s0 + block]
            ub = None if u is None else u[begin + s0:begin + s0 + block][None]
            pc, pw, dist = ops.sample_rays_world(rc, ij, c2w, None, None, None, ub, None, seed + begin + s0,
                                                 near_const=near_c, far_const=far_c)
            out4 = ops.field_eval_knn(self._fc, params, pw.view(-1, 3), pos, quat, m._num_knn, m._distance_factor,
                                      m._outside_value)
            rgbd, _, dv, _ = ops.composite_packed(rc, out4, dist.view(-1, S), pc.view(-1, S, 3))
            rgbds.append(rgbd)
            dvars.append(dv)
        if not rgbds:
            return torch.empty(0, 4, device=dev), torch.empty(0, device=dev)
        return torch.cat(rgbds), torch.cat(dvars)

    @torch.no_grad()
    def render_image(self, c2w: torch.Tensor, camera: Optional[Camera] = None, u: Optional[torch.Tensor] = None,
                     seed: int = 0):
        """render_image (rm.py:402-437): every pixel of `camera`, single stratum, kNN-blended fields, in the current mode
        like the reference: its callers switch to eval() first (rm.py:1879-1906, 1978-2019); in train mode this renders
        with `num_samples_coarse` samples in [near_distance, far_distance], as the reference would.

        Returns (rgbds (H,W,4), depth_vars (H,W)).  `u` (H*W, S) optionally supplies the torch.rand draws."""
        cam = camera or self._camera
        rgbd, dv = self.render_pixels(c2w, 0, cam.height * cam.width, camera=cam, u=u, seed=seed)
        return rgbd.reshape(cam.height, cam.width, 4), dv.reshape(cam.height, cam.width)

    @staticmethod
    def psnr(prediction: torch.Tensor, target: torch.Tensor, crop: int = 0) -> float:
        """evaluation.psnr (evaluation.py:46-56): clamp to [0,1], optional border crop, data_range 1."""
        if crop > 0:
            prediction, target = prediction[crop:-crop, crop:-crop], target[crop:-crop, crop:-crop]
        mse = ((prediction.clamp(0.0, 1.0) - target.clamp(0.0, 1.0)) ** 2).mean()
        return float(10.0 * torch.log10(1.0 / mse))

    def _eval_request(self, metrics, crop):
        from . import evaluation
        cfg = self._config
        metrics = evaluation.check_metrics(cfg.get("eval_metrics") or [] if metrics is None else metrics)
        return metrics, evaluation._check_crop(cfg.get("eval_crop", 0) if crop is None else crop)

    @torch.no_grad()
    def evaluate_frame(self, c2w: torch.Tensor, target_rgbd: torch.Tensor, camera: Optional[Camera] = None, metrics=None,
                       crop: Optional[int] = None, seed: int = 0) -> dict:
        """NeuralGraphMap._evaluate_frame (rm.py:1977-2020): eval(), render_image(c2w, camera), the frame scored against
        `target_rgbd` (H, W, 4) on the device by one evaluation.image_metrics call, train() afterwards as rm.py:2019 does.
        metrics: names out of "psnr", "ssim", "depthl1" (default: config `eval_metrics`, which defaults to []); "lpips" raises
        NotImplementedError.  crop defaults to config `eval_crop`.  Returns {metric: float} for the metrics asked for, in
        that order: one transfer."""
        from . import evaluation
        metrics, crop = self._eval_request(metrics, crop)
        cam = camera or self._camera
        ops._require_gpu(target_rgbd)
        if tuple(target_rgbd.shape) != (cam.height, cam.width, 4) or target_rgbd.dtype != torch.float32:
            raise ValueError(f"evaluate_frame expects target_rgbd as ({cam.height}, {cam.width}, 4) float32, got "
                             f"{tuple(target_rgbd.shape)} {target_rgbd.dtype}")
        self.eval()
        try:
            rgbd, _ = self.render_image(c2w, camera, seed=seed)
            row = evaluation.image_metrics_raw(rgbd[None], target_rgbd[None], crop)[0].cpu()
        finally:
            self.train()
        return {m: float(row[evaluation.OUT_COLUMNS.index(m)]) for m in metrics}

    @torch.no_grad()
    def evaluate_frames(self, c2ws, target_rgbds, camera: Optional[Camera] = None, metrics=None, crop: Optional[int] = None,
                        seed: int = 0, batch: int = 16):
        """_evaluate_frame over the frames of a chunk or a sequence (rm.py:1897-1906, 1930-1936): frame i is rendered from
        c2ws[i] with `seed` and scored against target_rgbds[i]; the frames are scored `batch` at a time and everything is
        read back once at the end.  Returns (mean_dict, per_frame): the reference's _mean_metric_dict (rm.py:82-92) of the
        metrics asked for, and the (N, 8) host array of ngm_image_metrics rows (evaluation.OUT_COLUMNS).  No frame: ({}, (0, 8))."""
        from . import evaluation
        metrics, crop = self._eval_request(metrics, crop)
        if len(c2ws) != len(target_rgbds):
            raise ValueError(f"evaluate_frames: {len(c2ws)} poses and {len(target_rgbds)} targets")
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            raise ValueError(f"evaluate_frames: batch must be an integer >= 1, got {batch!r}")
        rows = []
        self.eval()
        try:
            for s0 in range(0, len(c2ws), batch):
                pred = torch.stack([self.render_image(c2ws[i], camera, seed=seed)[0] for i in range(s0, min(s0 + batch, len(c2ws)))])
                tgt = torch.stack([target_rgbds[i].to(pred.device) for i in range(s0, s0 + pred.shape[0])])
                rows.append(evaluation.image_metrics_raw(pred, tgt, crop))
        finally:
            self.train()
        import numpy as np
        if not rows:
            return {}, np.zeros((0, 8))
        per_frame = torch.cat(rows).cpu().numpy()
        return evaluation.mean_metric_dict(per_frame, metrics), per_frame

    # -- fused fast path -----------------------------------------------------------------------
    def _workspace(self, F, R):
        key = (F, R)
        if key not in self._ws_cache:
            wsb = K.lib().ngm_render_workspace(C.byref(self._fc), C.byref(self._rc_train), F, R, 1)
            if wsb < 0:                                    # a configuration the library refuses: its status and message
                K.check(int(wsb), "ngm_render_workspace")
            dev = self._device
            self._ws_cache[key] = dict(
                ws=torch.empty(wsb, device=dev, dtype=torch.uint8), wsb=wsb,
                rgbds=torch.empty(F, R, 4, device=dev), color_vars=torch.empty(F, R, 3, device=dev),
                depth_vars=torch.empty(F, R, device=dev), term_probs=torch.empty(F, R, device=dev),
                sums=torch.zeros(K.NGM_NUM_LOSS_SUMS, device=dev), loss=torch.zeros(8, device=dev),
                philox=torch.zeros(1, device=dev, dtype=torch.int64))
        return self._ws_cache[key]

    def optimization_iteration(self, target: Target, u_coarse=None, u_guided=None, seed=0, update=True) -> dict:
        """One training iteration (rm.py:1123-1221): fused forward + losses, (all-reduce), fused backward,
        sparse Adam on the touched fields.  Returns the loss dict (device scalars) and, with
        update=False, also the gradients.  Every launch is asynchronous on the current stream and the
        sequence is hipGraph-capturable (device-side step / jitter counters, no allocation after the
        first call with a given batch shape).

        A DeviceTarget (sample_target_mv_device) is consumed as it is -- the counted step: every launch is sized for the
        capacity Fcap and the kernels read `target.count` on the device, so nothing here synchronises or depends on the
        count, and one captured graph serves every count in [0, Fcap].  Rows >= count are never read (their field_ids of
        -1 included) and never written: `prediction` rows and, with update=False, gradient rows >= count are unspecified
        (leftovers of earlier calls).  count == 0 is an iteration like _idle_iteration's: zero sums, NaN loss terms, no
        parameter touched, counters advanced; with a process group / peer_exchange the loss exchange is entered by every
        rank whatever its count.  Configurations outside the counted step (geometry mode neus, triplane encoding, *_nll
        loss modes) fall back to target.materialize() with a one-time RuntimeWarning (it synchronises) -- under graph
        capture they raise instead."""
        if isinstance(target, DeviceTarget):
            return self._counted_iteration(target, u_coarse, u_guided, seed, update)
        if self._rc_train.geometry_mode == K.GEO["neus"] and not self._neus_fused():
            return self.optimization_iteration_staged(target, u_coarse, u_guided, seed, update)
        return self._fused_iteration(target, u_coarse, u_guided, seed, update)

    def _fused_iteration(self, target: Target, u_coarse, u_guided, seed, update, count=None) -> dict:
        """The iteration on the fused kernels, plain (count None) or counted: forward, loss exchange, backward"""
        if target.ijs.shape[0] == 0:                      # counted: capacity 0 is known on the host (a rank that owns no field at all)
            return self._idle_iteration(update)
        ctx = self._iteration_forward(target, u_coarse, u_guided, seed, advance=update, count=count)
        if self.process_group is not None:
            # the only cross-GPU exchange of the path: global loss sums / counts (64 bytes); counted: entered by every rank,
            # whatever its own count
            self._exchange(ctx["w"]["sums"])
        return self._iteration_backward(ctx, update)

    def counted_step_unsupported(self) -> Optional[str]:
        """Why this renderer's configuration is outside the counted step (None: it is inside).  The library draws the same
        line (ngm_render_*_counted: NGM_E_UNSUPPORTED): neus and the triplane encoding run launches over all F rows, the
        *_nll loss modes are left out."""
        rc, fc = self._rc_train, self._fc
        if rc.geometry_mode == K.GEO["neus"]:
            return "geometry mode 'neus'"
        if fc.encoding == K.ENC["triplane"]:
            return "the triplane encoding"
        if rc.photometric_mode == K.PHOTO["gaussian_nll"] or rc.depth_mode != K.DEPTH["huber"]:
            return "the *_nll loss modes"
        return None

    def _counted_iteration(self, target: "DeviceTarget", u_coarse=None, u_guided=None, seed=0, update=True) -> dict:
        """optimization_iteration on a DeviceTarget: the fused step at capacity with the device count (never materialize(),
        never a read of `count`), or the warned fallback for configurations outside the counted step."""
        why = self.counted_step_unsupported()
        if why is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"optimization_iteration(DeviceTarget): {why} is outside the counted step and the "
                                   "fallback (DeviceTarget.materialize()) synchronises: it cannot be captured")
            if not self._warned_counted_fallback:
                self._warned_counted_fallback = True
                warnings.warn(f"optimization_iteration(DeviceTarget): {why} is outside the counted step; falling back to "
                              "DeviceTarget.materialize(), which synchronises with the host every iteration",
                              RuntimeWarning, stacklevel=3)
            return self.optimization_iteration(target.materialize(), u_coarse, u_guided, seed, update)
        return self._fused_iteration(target, u_coarse, u_guided, seed, update, count=target.count)

    def check_exchange(self):
        """Raise if the in-graph loss exchange ever timed out or lost step (its sums were partial then, i.e. the update of
        that iteration used wrong loss normalisers).  Synchronises; called automatically every `peer_check_interval`
        iterations, call it yourself before trusting losses / checkpoints of a multi-GPU run.  No-op without PeerExchange."""
        if self.peer_exchange is not None:
            self.peer_exchange.check()

    def _count_exchange(self):
        """host-side bookkeeping of one (launched or replayed) exchange; the periodic health check"""
        self._peer_calls += 1
        if self.peer_exchange is not None and self.peer_check_interval and self._peer_calls % self.peer_check_interval == 0:
            if not torch.cuda.is_current_stream_capturing():
                self.peer_exchange.check()

    def _exchange(self, sums: torch.Tensor):
        if self.peer_exchange is not None:
            self.peer_exchange.allreduce(sums)       # one kernel on the current stream: xGMI peer writes, capturable
            self._count_exchange()
        else:
            torch.distributed.all_reduce(sums, group=self.process_group)

    def _neus_fused(self) -> bool:
        """the neus geometry mode runs in the fused kernels for the Fourier / no encoding without skip connections
        (two-pass compositing in the forward, neighbour terms + per-field d/d _neus_sd in the backward); the staged path
        (standalone sampler / field / quadrature kernels under autograd) serves the other encodings"""
        fc = self._fc
        return fc.encoding in (K.ENC["fourier"], K.ENC["none"]) and fc.skip_mode == K.SKIP["no"]

    def _idle_iteration(self, update=True) -> dict:
        """A rank none of whose fields is active in this iteration: it contributes zeros to the loss
        all-reduce (which it must still enter), launches nothing else, and keeps the shared counters in step."""
        from . import distributed as D
        sums = torch.zeros(16, device=self._device)
        if self.process_group is not None:
            self._exchange(sums)
        rc = self._rc_train
        loss = D.loss_values_from_sums(sums, rc.w_termination, rc.w_photometric, rc.w_depth, rc.w_freespace, rc.w_tsdf,
                                       self._config["photometric_loss"], self._config["depth_loss"])
        if update:
            self._step += 1
            if self._step_dev is None:
                self._step_dev = torch.full((1,), self._step, device=self._device, dtype=torch.int64)
            else:
                self._step_dev += 1
        else:
            loss["grads"] = {}
        loss["prediction"] = None
        return loss

    def _iteration_forward(self, target: Target, u_coarse=None, u_guided=None, seed=0, advance=True, count=None) -> dict:
        """First half of the iteration: fused forward + local loss sums (everything before the all-reduce).
        One device counter counts the iterations: the forward adds it to the Philox offset, the loss-reduction kernel
        advances it (advance=True) and Adam then reads it as its step -- no launch of its own for the bookkeeping.
        count (device int32 (1,)): the counted step -- `target` holds that many rows followed by padding; the padded
        field_ids go to the kernels as they are (rows >= count are not read)."""
        L = K.lib()
        fc, rc = self._fc, self._rc_train
        fids = target.field_ids
        F, R = target.ijs.shape[0], target.ijs.shape[1]
        names = K.param_names(fc)
        allp = {n: self._model.all_fields_params[n] for n in names}       # fp32 masters (Adam)
        kp = self._model.kernel_params()                                   # what the kernels read (reduced precision or masters)
        lp = None if self._model.lp_fields_params is None else {n: kp[n] for n in names}
        kernel_p = {n: kp[n] for n in names}
        neus = rc.geometry_mode == K.GEO["neus"]
        if neus:
            kernel_p["_neus_sd"] = self._model.all_fields_params["_neus_sd"]
        ps = ops.params_struct(fc, kernel_p, fids)                         # rows field_ids[f] in place: no gather
        w = self._workspace(F, R)
        keep = []
        if self._step_dev is None:
            self._step_dev = torch.full((1,), self._step, device=self._device, dtype=torch.int64)
        rays = ops.make_rays(rc, target.ijs, target.c2ws, target.near_distances, target.far_distances,
                             target.gt_distances, self._global_map_dict["positions"],
                             self._global_map_dict["orientations"], u_coarse, u_guided, seed, keep=keep,
                             pose_index=fids, philox_offset_dev=self._step_dev, philox_autoinc=advance)
        dm = target.depth_mask.view(torch.uint8) if target.depth_mask.dtype == torch.bool else target.depth_mask
        tm = target.term_mask
        if tm is not None and tm.dtype == torch.bool:
            tm = tm.view(torch.uint8)
        rgbds_t = ops._f32c(target.rgbds)
        tg = K.Targets(ops._ptr(rgbds_t), dm.data_ptr(), ops._ptr(tm), ops._ptr(target.term_probs))
        pred = K.Prediction(w["rgbds"].data_ptr(), w["color_vars"].data_ptr(), w["depth_vars"].data_ptr(),
                            w["term_probs"].data_ptr())
        st = ops._stream()
        # single GPU: nothing happens between forward and backward, so the loss partials are reduced by the backward
        # itself (deferred reduction, one launch less); with a process group the sums are needed here for the all-reduce
        defer = self.process_group is None
        fn, args = "ngm_render_fwd", [C.byref(fc), C.byref(rc), C.byref(ps), C.byref(rays), C.byref(tg), C.byref(pred),
                                      None if defer else w["sums"].data_ptr(), w["ws"].data_ptr(), w["wsb"], st]
        if count is not None:
            if count.dtype != torch.int32 or count.numel() != 1 or not count.is_cuda:
                raise TypeError("count must be a device int32 tensor of one element")
            fn += "_counted"
            args.append(count.data_ptr())
        K.check(getattr(L, fn)(*args), fn)
        return dict(fc=fc, rc=rc, ps=ps, rays=rays, tg=tg, pred=pred, w=w, F=F, fids=fids, allp=allp, lp=lp, defer=defer,
                    neus=neus, count=count, keep=(keep, dm, tm, rgbds_t, target))

    def _iteration_backward(self, ctx: dict, update=True) -> dict:
        """Second half: compositing + MLP backward with the (global) loss sums, sparse Adam, counters."""
        L = K.lib()
        fc, rc, ps, rays, tg, pred, w, F, fids, allp = (ctx[k] for k in ("fc", "rc", "ps", "rays", "tg", "pred", "w", "F",
                                                                         "fids", "allp"))
        st = ops._stream()
        if "grads" not in w:
            w["grads"], w["gs"], w["gflat"] = ops.alloc_grads(fc, F, self._device)
        grads, gs = w["grads"], w["gs"]
        if ctx.get("neus") and "_neus_sd" not in grads:
            grads["_neus_sd"] = torch.zeros(F, device=self._device)
            gs.neus_sd = grads["_neus_sd"].data_ptr()
        count = ctx.get("count")
        # backward (+ sparse Adam in the same call: the gradient-reduction kernel applies the update of the MLP tensors itself,
        # rm.py:1183-1221; the device counter already holds the new step, the loss reduction advanced it); with a count the
        # *_counted entry point takes its pointer as one more argument
        fn, args = "ngm_render_bwd", [C.byref(fc), C.byref(rc), C.byref(ps), C.byref(rays), C.byref(tg), C.byref(pred),
                                      None if ctx.get("defer") else w["sums"].data_ptr(), C.byref(gs)]
        if update:
            arr, n_mlp, lat = ops.adam_tensor_arrays(fc, allp, self._optim_state, grads, ctx.get("lp"))
            fn += "_adam"
            args += [arr, n_mlp, lat, ops._ptr(fids), int(self._step) + 1, ops._ptr(self._step_dev), self._learning_rate, 0.9, 0.999,
                     self._adam_eps, self._adam_weight_decay]
        args += [w["loss"].data_ptr(), w["ws"].data_ptr(), w["wsb"], st]
        if count is not None:
            fn += "_counted"
            args.append(count.data_ptr())
        K.check(getattr(L, fn)(*args), fn)
        if update:
            self._step += 1                # one counter for all fields (rm.py:380-385); after the call: a refused step is no step
        if update and count is None:       # the counted step has neither: these launches run over all F rows
            if fc.encoding == K.ENC["triplane"]:      # the feature planes: gradient from the fixed-point scatter, same sparse Adam
                gp = grads["_encoding.plane_coef"]
                self._adam_one_tensor("_encoding.plane_coef", gp, allp["_encoding.plane_coef"].stride(0), gp.stride(0),
                                      gp[0].numel(), fids, F, st)
            if ctx.get("neus"):      # the per-field standard deviation is a parameter of its own (rm.py:641-644): same Adam
                self._adam_one_tensor("_neus_sd", grads["_neus_sd"], 1, 1, 1, fids, F, st)
        if update:
            self._count_training_iteration(fids, count)
        lv = w["loss"]
        loss = {"combined": lv[0], "termination": lv[1], "photometric_" + self._config["photometric_loss"]: lv[2],
                "depth_" + self._config["depth_loss"]: lv[3],
                "freespace": lv[4], "tsdf": lv[5]}
        if not update:
            loss["grads"] = grads
        loss["prediction"] = Prediction(w["rgbds"], w["color_vars"], w["depth_vars"], w["term_probs"], None, None)
        return loss

    def _adam_one_tensor(self, name, grad, stride, grad_stride, numel, fids, F, st) -> None:
        """sparse Adam on rows `fids` of one stacked parameter tensor, at the step this iteration has just counted"""
        p, stt = self._model.all_fields_params[name], self._optim_state[name]
        one = (K.AdamTensor * 1)(K.AdamTensor(p.data_ptr(), stt["exp_avg"].data_ptr(), stt["exp_avg_sq"].data_ptr(),
                                              grad.data_ptr(), stride, grad_stride, numel))
        K.check(K.lib().ngm_adam_sparse_multi(one, 1, ops._ptr(fids), F, int(self._step), ops._ptr(self._step_dev),
                                              self._learning_rate, 0.9, 0.999, self._adam_eps, self._adam_weight_decay, 0,
                                              None, st), "ngm_adam_sparse_multi")

    def capture_iteration(self, target: Target, seed=0, u_coarse=None, u_guided=None):
        """Capture optimization_iteration(target) into hipGraphs (torch.cuda.CUDAGraph); the returned callable
        replays it.  Tensors of `target` are read in place at every replay; the Adam step counter and the Philox
        jitter offset live on the device and advance inside the graph.  With a process group the iteration becomes
        two graphs (before / after the loss all-reduce) and the 64-byte collective is issued between the replays --
        unless `peer_exchange` is set: then the exchange is a kernel of the ONE captured graph.
        A DeviceTarget is captured as the counted step: the one graph serves every active count up to its capacity."""
        if self._rc_train.geometry_mode == K.GEO["neus"] and not self._neus_fused():
            raise NotImplementedError("capture_iteration: the staged (neus) iteration allocates under autograd; call "
                                      "optimization_iteration directly")
        count = None
        if isinstance(target, DeviceTarget):
            why = self.counted_step_unsupported()
            if why is not None:
                raise RuntimeError(f"capture_iteration(DeviceTarget): {why} is outside the counted step; capture a "
                                   "materialised Target instead")
            count = target.count
        if self.track_training_iterations:
            self._training_iterations()                       # must exist before the capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):                                # warm-up on a side stream (allocations, lazy init)
                self.optimization_iteration(target, u_coarse, u_guided, seed=seed)
        torch.cuda.current_stream().wait_stream(s)

        def whole():
            return self.optimization_iteration(target, u_coarse, u_guided, seed=seed)
        return self._capture("capture_iteration", whole,
                             lambda: self._iteration_forward(target, u_coarse, u_guided, seed, advance=True, count=count))

    def _capture(self, caller: str, whole, forward):
        """The capture both capture_iteration and capture_training end in, after their own warm-up.  `whole()` is one
        iteration; `forward()` its part before the loss all-reduce, returning the context _iteration_backward(ctx, True)
        finishes.  Single GPU, or the loss exchange is a kernel of the iteration (distributed.PeerExchange): `whole` as one
        graph.  A process group without peer exchange: two graphs on one pool around the collective, captured in
        thread-local mode (the process group's watchdog thread may touch the HIP runtime meanwhile); if that capture is
        refused, `whole` itself is returned (`.graph` None, `.capture_error` the message) after a RuntimeWarning.  The
        capture pass records, it does not execute: `_step` is put back, and every replay counts one step."""
        step0 = self._step
        if self.process_group is None or self.peer_exchange is not None:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = whole()
            self._step = step0

            def replay():
                graph.replay()
                self._step += 1
                if self.peer_exchange is not None:
                    self._count_exchange()                    # the exchange is a kernel of this graph: periodic health check
                return out
            replay.graph = graph
            return replay
        try:
            g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, capture_error_mode="thread_local"):
                ctx = forward()
            with torch.cuda.graph(g2, pool=g1.pool(), capture_error_mode="thread_local"):
                out = self._iteration_backward(ctx, True)
        except RuntimeError as err:
            # capture refused (runtime / collective library combination): plain launches still work, but the caller
            # is told -- an iteration of ~10 launches is launch-bound without the graph (`.graph is None`)
            self._step = step0
            torch.cuda.synchronize()
            warnings.warn(f"{caller}: graph capture refused ({err}); falling back to plain launches", RuntimeWarning, stacklevel=3)
            whole.graph, whole.capture_error = None, str(err)
            return whole
        self._step = step0
        sums, group = ctx["w"]["sums"], self.process_group

        def replay2():
            g1.replay()
            torch.distributed.all_reduce(sums, group=group)
            g2.replay()
            self._step += 1
            return out
        replay2.graph = (g1, g2)
        return replay2

    def capture_training(self, current_field_ids, c_c2w, nc_rgbd, frame_cid_to_ncid, num_train_fields, num_rays_per_field,
                         seed=0, camera: Optional[Camera] = None, world_size: int = 1, rank: int = 0, *,
                         current_count: Optional[torch.Tensor] = None, num_frames: Optional[torch.Tensor] = None):
        """The whole training iteration as ONE captured graph: sample_target_mv_device(iteration=None) followed by the
        counted optimization_iteration on its DeviceTarget -- sampler, forward, losses, backward and sparse Adam, with no
        host synchronisation and no data-dependent shape.  Returns a callable; every call replays the graph, i.e. draws the
        NEXT iteration's targets (the renderer's device iteration counter advances inside the graph) and trains on them,
        and returns the loss dict of device scalars.  `.target` is the static DeviceTarget the replays overwrite, `.graph`
        the torch.cuda.CUDAGraph -- or the pair (before / after the loss all-reduce) with a process group and no
        `peer_exchange`, as capture_iteration builds it; None if the runtime refused that capture (plain launches then).

        The input tensors and the field poses are READ IN PLACE at every replay: update their contents freely (new
        keyframes in the same store, moved fields), but the graph is valid only while their shapes and storage, the
        number of fields and the stacked parameter tensors are unchanged (add_fields / load_model need a new capture).
        Shapes, data pointers and `num` are checked on the host at every replay (no synchronisation); the inputs must be
        contiguous device tensors (current_field_ids / frame_cid_to_ncid int64), since a copy made here would be the
        one the graph keeps reading.

        current_count / num_frames (both or neither; one-element int32 device tensors): the live sampler, see
        sample_target_mv_device.  current_field_ids, c_c2w and frame_cid_to_ncid are then fixed-capacity buffers whose
        first current_count / num_frames entries are read at every replay, so ONE capture serves every frame (a new
        observed set: observed_fields_device(out=...)) and every keyframe (KeyframeStore) until fields are added -- or,
        after reserve_fields(max_fields), beyond that: the graph then reads the number of fields on the device as well, the
        replay check watches the reservation (storage addresses and capacities) instead of `num` and the row counts, and
        add_fields(num_new, positions=, orientations=) between replays is legal up to max_fields.  Replacing any reserved
        tensor, reserve_fields again or load_model still raise "capture again".

        Every rank must own at least one field of the map (a capacity of 0 rows raises ValueError: nothing to capture).

        Before the capture the sampler and the counted step run once with update=False (allocations, the device
        counters); the iteration counter is put back afterwards, so the first replay is the iteration the counter named
        when this was called, and nothing has been trained yet."""
        why = self.counted_step_unsupported()
        if why is not None:
            raise RuntimeError(f"capture_training: {why} is outside the counted step (optimization_iteration would fall "
                               "back to DeviceTarget.materialize(), which synchronises)")
        if (current_count is None) != (num_frames is None):
            raise ValueError("capture_training: current_count and num_frames go together (both device tensors, or neither)")
        dev = torch.device(self._device)
        named = dict(current_field_ids=current_field_ids, c_c2w=c_c2w, nc_rgbd=nc_rgbd, frame_cid_to_ncid=frame_cid_to_ncid)
        if current_count is not None:
            named.update(current_count=current_count, num_frames=num_frames)
        for n, t in named.items():
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"capture_training: {n} must be a contiguous device tensor (it is read in place at every replay)")
        for n in ("current_field_ids", "frame_cid_to_ncid"):
            if named[n].dtype != torch.int64:
                raise TypeError(f"capture_training: {n} must be int64")
        num_fields = self._global_map_dict["num"]
        grow = self._reserved is not None and current_count is not None      # the graph reads num_fields_dev

        def sample():
            return self.sample_target_mv_device(current_field_ids, c_c2w, nc_rgbd, frame_cid_to_ncid, num_train_fields,
                                                num_rays_per_field, num_fields=None if grow else num_fields, camera=camera, seed=seed,
                                                iteration=None, world_size=world_size, rank=rank, current_count=current_count,
                                                num_frames=num_frames)
        return self._capture_sampled("capture_training", named, sample, grow, num_fields, seed)

    def _capture_sampled(self, caller: str, named: dict, sample, grow: bool, num_fields: int, seed):
        """What capture_training and capture_training_sv share: `sample()` (a device sampler with iteration=None, returning a
        DeviceTarget) + the counted step as one graph through _capture, the warm-up that leaves the iteration counter where
        it was, and the replay check over `named` (the caller's inputs, read in place), the field poses, the stacked
        parameters and -- grow -- the reservation."""
        def watched():
            ts = dict(named, positions=self._global_map_dict["positions"], orientations=self._global_map_dict["orientations"])
            ts.update({"param " + n: v for n, v in self._model.all_fields_params.items()})
            if self.track_training_iterations:
                ts["training_iterations"] = self._training_iterations()
            if not grow:
                return {n: (t.data_ptr(), tuple(t.shape)) for n, t in ts.items()}
            # reserved rows: the views the step reads (addresses; row shapes without the row count) + the reservation itself
            seen = {n: (t.data_ptr(), tuple(t.shape) if n in named else tuple(t.shape[1:])) for n, t in ts.items()}
            rs, mr = self._reserved, self._model._reserved
            if rs is None or mr is None:
                return dict(seen, reservation=None)
            caps = {"reserved " + n: t for n, t in mr["params"].items()}
            caps.update({"reserved lp " + n: t for n, t in (mr["lp"] or {}).items()})
            for n, st in rs["state"].items():
                caps["reserved exp_avg " + n], caps["reserved exp_avg_sq " + n] = st["exp_avg"], st["exp_avg_sq"]
                seen["exp_avg " + n] = (self._optim_state[n]["exp_avg"].data_ptr(),)
                seen["exp_avg_sq " + n] = (self._optim_state[n]["exp_avg_sq"].data_ptr(),)
            for n in ("positions", "orientations", "training_iterations", "num_fields_dev"):
                caps["reserved " + n] = rs[n]
            seen.update({n: (t.data_ptr(), tuple(t.shape)) for n, t in caps.items()})
            seen["reservation"] = (rs["max"], rs["epoch"])
            return seen
        for n in ("positions", "orientations"):
            if not self._global_map_dict[n].is_contiguous():
                raise ValueError(f"{caller}: the field {n} must be contiguous (read in place at every replay)")

        if self.track_training_iterations:
            self._training_iterations()                       # must exist before the capture
        # once outside the capture, on a side stream: creates the device counters, the workspace and the gradient buffers
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            it0 = None if self._target_iter_dev is None else self._target_iter_dev.clone()
            probe = sample()
            if probe.ijs.shape[0] == 0:
                raise ValueError(f"{caller}: this rank's capacity is 0 (it owns none of the fields that can be drawn: "
                                 "fewer fields than ranks); there is no step to capture -- call optimization_iteration, "
                                 "which runs the idle iteration for such a rank")
            self.optimization_iteration(probe, seed=seed, update=False)
            if it0 is None:
                self._target_iter_dev.zero_()
            else:
                self._target_iter_dev.copy_(it0)
        torch.cuda.current_stream().wait_stream(s)

        def step():                                           # the refused capture's fallback too: a fresh target per call
            step.target = sample()
            return self.optimization_iteration(step.target, seed=seed)

        def forward():
            step.target = sample()
            return self._iteration_forward(step.target, None, None, seed, advance=True, count=step.target.count)
        run = self._capture(caller, step, forward)
        if run.graph is None:
            run.target = None
            return run
        seen = watched()

        def replay():
            now = watched()
            if now != seen or (not grow and self._global_map_dict["num"] != num_fields):
                changed = sorted(n for n in now if now[n] != seen.get(n)) or ["number of fields"]
                raise RuntimeError(f"{caller}: {changed} changed shape or storage since the capture; the graph "
                                   "reads the captured addresses -- capture again")
            return run()
        replay.graph, replay.target = run.graph, step.target
        return replay
