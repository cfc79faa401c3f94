"""PyTorch-ROCm custom ops over the C ABI (include/ngm_hip.h).

torch is plumbing here (device memory, streams, autograd glue); every op below is a hand-written
gfx950 kernel reached through ``_capi``.  There is NO CPU / eager fallback: tensors must live on a
ROCm device ("cuda" under PyTorch-ROCm) and the HIP library must be built, otherwise the call raises.
"""
import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _capi as K


# ------------------------------------------------------------------------------------------------
# torch.library registration: every op below is visible to the dispatcher as torch.ops.ngm355.<name>
# (schema, fake/meta shapes, autograd formula) and calls the C ABI underneath.  "cuda" (= ROCm) kernels only:
# there is no CPU registration on purpose.  Configuration structs travel as small uint8 CPU tensors (the bytes
# of ngm_field_cfg / ngm_render_cfg), stacked parameter dictionaries as Tensor[] in K.param_names() order.
# ------------------------------------------------------------------------------------------------
NS = "ngm355"


_BLOBS: Dict[bytes, torch.Tensor] = {}       # struct bytes -> its uint8 CPU tensor (a renderer uses a handful of distinct structs)
_STRUCTS: Dict[int, object] = {}             # id(blob tensor) -> decoded ctypes struct (the blobs above live for the process)


def cfg_blob(struct) -> torch.Tensor:
    raw = bytes(struct)
    t = _BLOBS.get(raw)
    if t is None:
        if len(_BLOBS) > 4096:
            _BLOBS.clear(); _STRUCTS.clear()
        t = _BLOBS[raw] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        _STRUCTS[id(t)] = type(struct).from_buffer_copy(raw)
    return t


def _decode(blob: torch.Tensor, cls):
    s = _STRUCTS.get(id(blob))
    if s is not None and isinstance(s, cls):
        return s                             # read-only use below: the cached struct is never mutated
    return cls.from_buffer_copy(blob.numpy().tobytes())


def _field_cfg(blob: torch.Tensor) -> "K.FieldCfg":
    return _decode(blob, K.FieldCfg)


def _render_cfg(blob: torch.Tensor) -> "K.RenderCfg":
    return _decode(blob, K.RenderCfg)


def _op(name, mutates_args=()):
    return torch.library.custom_op(f"{NS}::{name}", mutates_args=mutates_args, device_types="cuda")


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("neural_graph_mapping_amd ops need ROCm device tensors; there is no CPU fallback "
                               "(the CPU restatement under oracle/ is test infrastructure only)")


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t, name="tensor"):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


# ------------------------------------------------------------------------------------------------
# parameter plumbing: dict of stacked (N, ...) tensors <-> ngm_params / ngm_grads
# ------------------------------------------------------------------------------------------------
_TORCH_DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def params_struct(fc: K.FieldCfg, params: Dict[str, torch.Tensor], field_index: Optional[torch.Tensor] = None):
    """dict of stacked (N, ...) tensors -> ngm_params.  The weights may be stored as float32, bfloat16 or float16 (all
    of them in the same type; the constant hash shifts stay float32): ngm_params.dtype tells the kernels, which widen to
    fp32 when they stage a field (storage only: the arithmetic is fp32 either way)."""
    ptrs, strides = {}, {}
    dts = set()
    for n, shp in K.param_shapes(fc).items():
        if n not in params:
            raise KeyError(f"missing parameter tensor '{n}'")
        t = params[n]
        _require_gpu(t)
        const = n in K.NO_GRAD_PARAMS
        if t.dtype not in _TORCH_DT or (const and t.dtype != torch.float32) or tuple(t.shape[1:]) != tuple(shp):
            raise ValueError(f"parameter '{n}' must be {'float32' if const else 'float32 / bfloat16 / float16'} (N,{shp}), "
                             f"got {t.dtype} {tuple(t.shape)}")
        if not const:
            dts.add(t.dtype)
        inner = t[0] if t.shape[0] > 0 else t
        if t.shape[0] > 0 and not inner.is_contiguous():
            raise ValueError(f"parameter '{n}' rows must be contiguous")
        ptrs[n] = t.data_ptr()
        strides[n] = t.stride(0) if t.shape[0] > 1 else int(torch.tensor(shp).prod())
    if len(dts) != 1:
        raise ValueError(f"the weight tensors must share one storage type, got {sorted(str(d) for d in dts)}")
    fi = None
    if field_index is not None:
        _require_gpu(field_index)
        if field_index.dtype != torch.int64:
            raise TypeError("field_index must be int64")
        fi = field_index.contiguous().data_ptr()
    ps = K.params_struct(fc, ptrs, strides, fi, _TORCH_DT[dts.pop()])
    sd = params.get("_neus_sd")
    if sd is not None:                 # per-field standard deviation of the neus geometry mode (fused render only)
        _require_gpu(sd)
        if sd.dtype != torch.float32 or sd.dim() != 1:
            raise ValueError("'_neus_sd' must be float32 (N,)")
        ps.neus_sd, ps.neus_sd_stride = sd.data_ptr(), sd.stride(0) if sd.shape[0] > 1 else 1
    return ps


def alloc_grads(fc: K.FieldCfg, F: int, device, flat: Optional[torch.Tensor] = None):
    """Gradient tensors (F, ...) per parameter name; views into one flat (F, P) arena."""
    shapes = K.param_shapes(fc)
    total = sum(int(torch.tensor(s).prod()) for s in shapes.values())
    if flat is None:
        flat = torch.zeros(F, total, device=device, dtype=torch.float32)
    grads, ptrs, strides, off = {}, {}, {}, 0
    for n, shp in shapes.items():
        numel = int(torch.tensor(shp).prod())
        grads[n] = flat[:, off:off + numel].view(F, *shp)
        ptrs[n] = flat.data_ptr() + off * 4
        strides[n] = flat.stride(0)
        off += numel
    return grads, K.grads_struct(fc, ptrs, strides), flat


def alloc_grads_separate(fc: K.FieldCfg, F: int, device):
    """One tensor per parameter name (custom-op outputs may not alias each other, so no shared arena here)."""
    shapes = K.param_shapes(fc)
    grads = {n: torch.zeros(F, *shp, device=device, dtype=torch.float32) for n, shp in shapes.items()}
    ptrs = {n: g.data_ptr() for n, g in grads.items()}
    strides = {n: int(torch.tensor(shp).prod()) for n, shp in shapes.items()}
    return grads, K.grads_struct(fc, ptrs, strides)


# ------------------------------------------------------------------------------------------------
# K2+K3: NeuralFieldSet.forward(use_vmap=True) with autograd
# ------------------------------------------------------------------------------------------------
@_op("field_eval")
def _field_eval_op(fcfg: torch.Tensor, points: torch.Tensor, pos: Optional[torch.Tensor], quat: Optional[torch.Tensor],
                   params: List[torch.Tensor]) -> torch.Tensor:
    fc = _field_cfg(fcfg)
    pd = dict(zip(K.param_names(fc), params))
    F, P, _ = points.shape
    out = torch.empty(F, P, 4, device=points.device, dtype=torch.float32)
    ps = params_struct(fc, pd)
    K.check(K.lib().ngm_field_eval_fwd(C.byref(fc), C.byref(ps), F, P, _ptr(points), _ptr(_f32c(pos)),
                                       _ptr(_f32c(quat)), _ptr(out), _stream()), "ngm_field_eval_fwd")
    return out


@_field_eval_op.register_fake
def _(fcfg, points, pos, quat, params):
    return points.new_empty(points.shape[0], points.shape[1], 4)


@_op("field_eval_bwd")
def _field_eval_bwd_op(fcfg: torch.Tensor, points: torch.Tensor, pos: Optional[torch.Tensor], quat: Optional[torch.Tensor],
                       d_out: torch.Tensor, params: List[torch.Tensor]) -> List[torch.Tensor]:
    fc = _field_cfg(fcfg)
    names = K.param_names(fc)
    pd = dict(zip(names, params))
    F, P, _ = points.shape
    grads, gs = alloc_grads_separate(fc, F, points.device)
    ps = params_struct(fc, pd)
    L = K.lib()
    wsb = L.ngm_field_eval_bwd_workspace(C.byref(fc), F, P)
    ws = torch.empty(wsb, device=points.device, dtype=torch.uint8)
    K.check(L.ngm_field_eval_bwd(C.byref(fc), C.byref(ps), F, P, _ptr(points), _ptr(_f32c(pos)), _ptr(_f32c(quat)),
                                 _ptr(_f32c(d_out, "d_out")), C.byref(gs), _ptr(ws), wsb, _stream()), "ngm_field_eval_bwd")
    return [grads[n] for n in names]


@_field_eval_bwd_op.register_fake
def _(fcfg, points, pos, quat, d_out, params):
    return [torch.empty_like(p, dtype=torch.float32) for p in params]      # gradients are fp32 whatever the storage dtype


def _field_eval_setup(ctx, inputs, output):
    fcfg, points, pos, quat, params = inputs
    ctx.fcfg, ctx.has_pose, ctx.n = fcfg, pos is not None, len(params)
    ctx.save_for_backward(points, *([pos, quat] if pos is not None else []), *params)


def _field_eval_backward(ctx, d_out):
    points, *rest = ctx.saved_tensors
    pos, quat = (rest[0], rest[1]) if ctx.has_pose else (None, None)
    params = rest[2:] if ctx.has_pose else rest
    grads = torch.ops.ngm355.field_eval_bwd(ctx.fcfg, points, pos, quat, d_out.contiguous(), list(params))
    return None, None, None, None, grads


_field_eval_op.register_autograd(_field_eval_backward, setup_context=_field_eval_setup)


# ---- the same under autograd with an activation stash (ABI 11): the forward writes the hidden activations, the backward is the
# fused training step's MLP backward (k_field_bwd_b3 in point mode) instead of the recomputing fp32 kernel
@_op("field_eval_train")
def _field_eval_train_op(fcfg: torch.Tensor, points: torch.Tensor, pos: Optional[torch.Tensor], quat: Optional[torch.Tensor],
                         params: List[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    fc = _field_cfg(fcfg)
    pd = dict(zip(K.param_names(fc), params))
    F, P, _ = points.shape
    L = K.lib()
    out = torch.empty(F, P, 4, device=points.device, dtype=torch.float32)
    sb = int(L.ngm_field_eval_stash_bytes(C.byref(fc), F, P))
    if sb <= 0:
        raise K.NgmError("field_eval_train: this configuration has no stash-reading backward (ngm_field_eval_stash_bytes == 0)")
    stash = torch.empty(sb, device=points.device, dtype=torch.uint8)      # an output: lives until the backward has run
    ps = params_struct(fc, pd)
    K.check(L.ngm_field_eval_fwd_train(C.byref(fc), C.byref(ps), F, P, _ptr(points), _ptr(_f32c(pos)), _ptr(_f32c(quat)), _ptr(out),
                                       _ptr(stash), sb, _stream()), "ngm_field_eval_fwd_train")
    return out, stash


@_field_eval_train_op.register_fake
def _(fcfg, points, pos, quat, params):
    return points.new_empty(points.shape[0], points.shape[1], 4), points.new_empty(0, dtype=torch.uint8)


@_op("field_eval_bwd_stash")
def _field_eval_bwd_stash_op(fcfg: torch.Tensor, points: torch.Tensor, pos: Optional[torch.Tensor], quat: Optional[torch.Tensor],
                             d_out: torch.Tensor, stash: torch.Tensor, params: List[torch.Tensor]) -> List[torch.Tensor]:
    fc = _field_cfg(fcfg)
    names = K.param_names(fc)
    pd = dict(zip(names, params))
    F, P, _ = points.shape
    grads, gs = alloc_grads_separate(fc, F, points.device)
    ps = params_struct(fc, pd)
    L = K.lib()
    wsb = L.ngm_field_eval_bwd_workspace(C.byref(fc), F, P)
    ws = torch.empty(wsb, device=points.device, dtype=torch.uint8)
    K.check(L.ngm_field_eval_bwd_stash(C.byref(fc), C.byref(ps), F, P, _ptr(points), _ptr(_f32c(pos)), _ptr(_f32c(quat)),
                                       _ptr(_f32c(d_out, "d_out")), C.byref(gs), _ptr(stash), stash.numel(), _ptr(ws), wsb, _stream()),
            "ngm_field_eval_bwd_stash")
    return [grads[n] for n in names]


@_field_eval_bwd_stash_op.register_fake
def _(fcfg, points, pos, quat, d_out, stash, params):
    return [torch.empty_like(p, dtype=torch.float32) for p in params]


def _field_eval_train_setup(ctx, inputs, output):
    fcfg, points, pos, quat, params = inputs
    ctx.fcfg, ctx.has_pose, ctx.n = fcfg, pos is not None, len(params)
    ctx.save_for_backward(points, output[1], *([pos, quat] if pos is not None else []), *params)
    ctx.mark_non_differentiable(output[1])
    ctx.set_materialize_grads(False)         # no zero "gradient" of the stash's size (a 2 GB fill per backward at 4 M points)


def _field_eval_train_backward(ctx, d_out, _d_stash):
    if d_out is None:
        return None, None, None, None, None
    points, stash, *rest = ctx.saved_tensors
    pos, quat = (rest[0], rest[1]) if ctx.has_pose else (None, None)
    params = rest[2:] if ctx.has_pose else rest
    grads = torch.ops.ngm355.field_eval_bwd_stash(ctx.fcfg, points, pos, quat, d_out.contiguous(), stash, list(params))
    return None, None, None, None, grads


_field_eval_train_op.register_autograd(_field_eval_train_backward, setup_context=_field_eval_train_setup)

# Above this many bytes of stash (256 B per point and hidden layer) a differentiable field_eval keeps the recomputing backward
# (no stash is held between forward and backward).  The reference's own training batch (32 fields x 512 rays x 24 samples)
# stashes 0.2 GB; the MI355X has 288 GB.
FIELD_EVAL_STASH_MAX_BYTES = 16 << 30


def field_eval(fc: K.FieldCfg, params: Dict[str, torch.Tensor], points, pos=None, quat=None):
    """(F,P,3) points -> (F,P,4); differentiable w.r.t. the parameters (not the points/poses).
    Dispatches through torch.ops.ngm355.field_eval; when a gradient will be asked for and the network has a stash-reading
    backward (ngm_field_eval_stash_bytes > 0) through torch.ops.ngm355.field_eval_train: same outputs bit for bit, the hidden
    activations kept for the backward (k_field_bwd_b3 in point mode) instead of being recomputed there."""
    names = K.param_names(fc)
    plist = [params[n] for n in names]
    _require_gpu(points, pos, quat, *plist)
    points = _f32c(points, "points")
    if torch.is_grad_enabled() and any(p.requires_grad for p in plist) and points.shape[1] > 0:
        sb = int(K.lib().ngm_field_eval_stash_bytes(C.byref(fc), points.shape[0], points.shape[1]))
        if 0 < sb <= FIELD_EVAL_STASH_MAX_BYTES:
            return torch.ops.ngm355.field_eval_train(cfg_blob(fc), points, pos, quat, plist)[0]
    return torch.ops.ngm355.field_eval(cfg_blob(fc), points, pos, quat, plist)


def encode(fc: K.FieldCfg, params: Dict[str, torch.Tensor], points, pos=None, quat=None):
    """The positional encoding alone (positional_encodings.py:19-66, 164-276): (F,P,3) points -> (F,P,dim_enc), no autograd.
    Standalone stage entry point (ngm_encode_fwd) -- the fused kernels never materialise this tensor."""
    names = K.param_names(fc)
    plist = [params[n] for n in names]
    _require_gpu(points, pos, quat, *plist)
    pts = _f32c(points, "points")
    F, P = pts.shape[0], pts.shape[1]
    out = torch.empty(F, P, fc.dim_enc, device=pts.device, dtype=torch.float32)
    ps = params_struct(fc, dict(zip(names, plist)))
    K.check(K.lib().ngm_encode_fwd(C.byref(fc), C.byref(ps), F, P, _ptr(pts), _ptr(None if pos is None else _f32c(pos)),
                                   _ptr(None if quat is None else _f32c(quat)), _ptr(out), _stream()), "ngm_encode_fwd")
    return out


def encode_bwd(fc: K.FieldCfg, params: Dict[str, torch.Tensor], points, d_enc, pos=None, quat=None) -> Dict[str, torch.Tensor]:
    """Backward of `encode` w.r.t. the encoding's own parameters (ngm_encode_bwd): d_enc (F,P,dim_enc) ->
    {"_encoding._linear.weight": (F, dim_enc - 3, 3)} (Fourier) or {"_encoding.lattice_values": (F, L, T, 2)} (hash);
    {} for the parameter-free encodings."""
    names = K.param_names(fc)
    plist = [params[n] for n in names]
    _require_gpu(points, d_enc, pos, quat, *plist)
    pts, de = _f32c(points, "points"), _f32c(d_enc, "d_enc")
    F, P = pts.shape[0], pts.shape[1]
    if tuple(de.shape) != (F, P, fc.dim_enc):
        raise ValueError(f"d_enc must be (F, P, dim_enc) = {(F, P, fc.dim_enc)}, got {tuple(de.shape)}")
    ps = params_struct(fc, dict(zip(names, plist)))
    out, g = {}, K.Grads()
    if fc.encoding == K.ENC["fourier"]:
        t = out["_encoding._linear.weight"] = torch.empty(F, *K.param_shapes(fc)["_encoding._linear.weight"], device=pts.device)
        g.enc_w, g.enc_w_stride = t.data_ptr(), t.stride(0)
    elif fc.encoding == K.ENC["permuto"]:
        t = out["_encoding.lattice_values"] = torch.empty(F, *K.param_shapes(fc)["_encoding.lattice_values"], device=pts.device)
        g.lattice, g.lattice_stride = t.data_ptr(), t.stride(0)
    L = K.lib()
    wsb = L.ngm_encode_bwd_workspace(C.byref(fc), F, P)
    ws = torch.empty(max(int(wsb), 256), device=pts.device, dtype=torch.uint8)
    K.check(L.ngm_encode_bwd(C.byref(fc), C.byref(ps), F, P, _ptr(pts), _ptr(None if pos is None else _f32c(pos)),
                             _ptr(None if quat is None else _f32c(quat)), _ptr(de), C.byref(g), _ptr(ws), ws.numel(), _stream()),
            "ngm_encode_bwd")
    return out


@_op("field_eval_knn")
def _field_eval_knn_op(fcfg: torch.Tensor, points: torch.Tensor, pos: torch.Tensor, quat: torch.Tensor,
                       params: List[torch.Tensor], num_knn: int, distance_factor: float, outside_value: float,
                       field_index: Optional[torch.Tensor], mask_radius: float) -> torch.Tensor:
    fc = _field_cfg(fcfg)
    P, NF = points.shape[0], pos.shape[0]
    out = torch.empty(P, 4, device=points.device, dtype=torch.float32)
    if P == 0:
        return out
    ps = params_struct(fc, dict(zip(K.param_names(fc), params)), field_index)
    L = K.lib()
    wsb = L.ngm_field_eval_knn_workspace(NF, P, num_knn)
    ws = torch.empty(wsb, device=points.device, dtype=torch.uint8)
    K.check(L.ngm_field_eval_knn(C.byref(fc), C.byref(ps), NF, P, _ptr(points), _ptr(_f32c(pos)), _ptr(_f32c(quat)),
                                 num_knn, distance_factor, outside_value, mask_radius, _ptr(out), _ptr(ws), wsb, _stream()),
            "ngm_field_eval_knn")
    return out


@_field_eval_knn_op.register_fake
def _(fcfg, points, pos, quat, params, num_knn, distance_factor, outside_value, field_index, mask_radius):
    return points.new_empty(points.shape[0], 4)


def field_eval_knn(fc, params, points, pos, quat, num_knn=2, distance_factor=10.0, outside_value=1.0,
                   field_index=None, mask_radius=None):
    """models.py:347-405: kNN-blended evaluation of world points (P,3) over all fields -> (P,4).
    `mask_radius` = the `field_radius` argument of the reference's forward (models.py:293, 368): which points count as
    inside a field; the local coordinates are scaled with the model's own radius (fc.field_radius) either way.
    Dispatches through torch.ops.ngm355.field_eval_knn."""
    plist = [params[n] for n in K.param_names(fc)]
    _require_gpu(points, pos, quat, *plist)
    return torch.ops.ngm355.field_eval_knn(cfg_blob(fc), _f32c(points.reshape(-1, 3)), pos, quat, plist, int(num_knn),
                                           float(distance_factor), float(outside_value), field_index,
                                           float(mask_radius) if mask_radius else 0.0)


@_op("grid_eval_knn")
def _grid_eval_knn_op(fcfg: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, zs: torch.Tensor, pos: torch.Tensor,
                      quat: torch.Tensor, params: List[torch.Tensor], num_knn: int, distance_factor: float,
                      outside_value: float, field_index: Optional[torch.Tensor], mask_radius: float, channel: int,
                      negate: bool) -> torch.Tensor:
    fc = _field_cfg(fcfg)
    nx, ny, nz, NF = xs.shape[0], ys.shape[0], zs.shape[0], pos.shape[0]
    L = K.lib()
    wsb = L.ngm_grid_eval_knn_workspace(NF, nx, ny, nz, num_knn)
    if wsb < 0:                # the shape is refused before anything is allocated (NGM_E_UNSUPPORTED: nx ny nz K >= 2^31)
        K.check(int(wsb), "ngm_grid_eval_knn_workspace")
    vol = torch.empty(nx, ny, nz, device=xs.device, dtype=torch.float32)
    ps = params_struct(fc, dict(zip(K.param_names(fc), params)), field_index)
    ws = torch.empty(wsb, device=xs.device, dtype=torch.uint8)
    K.check(L.ngm_grid_eval_knn(C.byref(fc), C.byref(ps), NF, _ptr(_f32c(pos)), _ptr(_f32c(quat)), _ptr(xs), nx, _ptr(ys), ny,
                                _ptr(zs), nz, num_knn, distance_factor, outside_value, mask_radius, channel, int(negate),
                                _ptr(vol), _ptr(ws), wsb, _stream()), "ngm_grid_eval_knn")
    return vol


@_grid_eval_knn_op.register_fake
def _(fcfg, xs, ys, zs, pos, quat, params, num_knn, distance_factor, outside_value, field_index, mask_radius, channel, negate):
    return xs.new_empty(xs.shape[0], ys.shape[0], zs.shape[0])


def grid_eval_knn(fc, params, xs, ys, zs, pos, quat, num_knn=2, distance_factor=10.0, outside_value=1.0,
                  field_index=None, mask_radius=None, channel=3, negate=False):
    """One channel of the kNN-blended fields on the lattice xs x ys x zs (three 1-D fp32 device axes, uniform or not) as a
    (nx, ny, nz) volume: field_eval_knn(torch.cartesian_prod(xs, ys, zs))[:, channel].reshape(nx, ny, nz), negated when
    `negate`, bit for bit, in one call that keeps neither the points nor the (P, 4) output in memory (one block of
    _extract_mesh's grid, rm.py:2236-2261).  Raises NgmError with code NGM_E_UNSUPPORTED when nx ny nz K >= 2^31.
    Dispatches through torch.ops.ngm355.grid_eval_knn."""
    plist = [params[n] for n in K.param_names(fc)]
    _require_gpu(xs, ys, zs, pos, quat, *plist)
    for t, n in ((xs, "xs"), (ys, "ys"), (zs, "zs")):
        if t.dim() != 1 or t.shape[0] < 1:
            raise ValueError(f"grid_eval_knn: {n} must be a 1-D axis with at least one coordinate, got {tuple(t.shape)}")
    if not 0 <= int(channel) <= 3:
        raise ValueError("grid_eval_knn: channel must be 0..3")
    return torch.ops.ngm355.grid_eval_knn(cfg_blob(fc), _f32c(xs, "xs"), _f32c(ys, "ys"), _f32c(zs, "zs"), pos, quat, plist,
                                          int(num_knn), float(distance_factor), float(outside_value), field_index,
                                          float(mask_radius) if mask_radius else 0.0, int(channel), bool(negate))


# ------------------------------------------------------------------------------------------------
# K1: sampler
# ------------------------------------------------------------------------------------------------
_LIN_CACHE = {}


def linspace_table(n: int, device):
    """torch.linspace(0,1,n+1) of camera.py:271 as a device table for the kernels.  Computed by torch on
    the host (bit-identical to the CPU reference / oracle; ROCm's device linspace may differ in the
    last bit for non power-of-two n) and cached per (n, device)."""
    key = (int(n), str(device))
    if key not in _LIN_CACHE:
        _LIN_CACHE[key] = torch.linspace(0.0, 1.0, steps=n + 1, dtype=torch.float32).to(device)
    return _LIN_CACHE[key]


def make_rays(rc: K.RenderCfg, ijs, c2ws, near, far, gt, pos, quat, u_coarse=None, u_guided=None, seed=0, offset=0,
              near_const=0.0, far_const=8.0, keep=None, pose_index=None, philox_offset_dev=None, philox_autoinc=False):
    """Build an ngm_rays record; `keep` (list) receives every temporary that must outlive the launch."""
    keep = keep if keep is not None else []
    _require_gpu(ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided)
    if ijs.dtype != torch.int64:
        raise TypeError("ijs must be int64 (row, col)")
    ijs = ijs.contiguous()
    F, R = (ijs.shape[0], ijs.shape[1]) if ijs.dim() == 3 else (1, ijs.shape[0])
    per_ray = 0 if c2ws.dim() == 2 else 1
    c2ws = _f32c(c2ws)
    if per_ray and c2ws.numel() != F * R * 16:
        c2ws = c2ws.expand(F, R, 4, 4).contiguous()
    dev = ijs.device
    lin_c = linspace_table(rc.num_samples_coarse, dev)
    lin_g = linspace_table(rc.num_samples_guided, dev) if rc.num_samples_guided > 0 else None
    ts = [ijs, c2ws, _f32c(near), _f32c(far), _f32c(gt), _f32c(pos), _f32c(quat), _f32c(u_coarse), _f32c(u_guided),
          lin_c, lin_g]
    if pose_index is not None:
        pose_index = pose_index.contiguous()
        _require_gpu(pose_index)
    keep.extend(ts + [pose_index, philox_offset_dev])
    return K.Rays(F, R, _ptr(ts[0]), _ptr(ts[1]), per_ray, 1 if (philox_autoinc and philox_offset_dev is not None) else 0, _ptr(ts[2]), _ptr(ts[3]), _ptr(ts[4]),
                  float(near_const), float(far_const), _ptr(ts[5]), _ptr(ts[6]), _ptr(ts[7]), _ptr(ts[8]),
                  _ptr(ts[9]), _ptr(ts[10]), int(seed), int(offset), _ptr(pose_index), _ptr(philox_offset_dev))


@_op("sample_rays")
def _sample_rays_op(rcfg: torch.Tensor, ijs: torch.Tensor, c2ws: Optional[torch.Tensor], near: Optional[torch.Tensor],
                    far: Optional[torch.Tensor], gt: Optional[torch.Tensor], u_coarse: Optional[torch.Tensor],
                    u_guided: Optional[torch.Tensor], seed: int, near_const: float, far_const: float,
                    num_samples: int) -> List[torch.Tensor]:
    """[points_cam (F,R,S,3), points_world (F,R,S,3) or empty (no c2ws), distances (F,R,S), dirs (F,R,3)]"""
    rc = _render_cfg(rcfg)
    dev = ijs.device
    F, R = ijs.shape[0], ijs.shape[1]
    world = c2ws is not None
    pos, quat = torch.zeros(F, 3, device=dev), torch.zeros(F, 4, device=dev)
    keep = []
    rays = make_rays(rc, ijs, c2ws if world else torch.eye(4, device=dev), near, far, gt, pos, quat, u_coarse, u_guided,
                     seed, near_const=near_const, far_const=far_const, keep=keep)
    S = rc.num_samples_coarse + (rc.num_samples_guided if gt is not None else 0)
    assert S == num_samples
    pc = torch.empty(F, R, S, 3, device=dev)
    pw = torch.empty((F, R, S, 3) if world else (0,), device=dev)
    dist = torch.empty(F, R, S, device=dev)
    dirs = torch.empty(F, R, 3, device=dev)
    K.check(K.lib().ngm_sample_rays_world(C.byref(rc), C.byref(rays), _ptr(pc), _ptr(pw) if world else None, _ptr(dist),
                                          _ptr(dirs), _stream()), "ngm_sample_rays_world")
    return [pc, pw, dist, dirs]


@_sample_rays_op.register_fake
def _(rcfg, ijs, c2ws, near, far, gt, u_coarse, u_guided, seed, near_const, far_const, num_samples):
    F, R, S = ijs.shape[0], ijs.shape[1], num_samples
    f = lambda *shape: torch.empty(*shape, device=ijs.device, dtype=torch.float32)
    return [f(F, R, S, 3), f(F, R, S, 3) if c2ws is not None else f(0), f(F, R, S), f(F, R, 3)]


def sample_rays(rc: K.RenderCfg, ijs, near, far, gt=None, u_coarse=None, u_guided=None, seed=0):
    """camera.py:215-292 + rm.py:521-545 -> (points_cam (F,R,S,3), distances (F,R,S), dirs (F,R,3))."""
    _require_gpu(ijs, near, far, gt, u_coarse, u_guided)
    S = rc.num_samples_coarse + (rc.num_samples_guided if gt is not None else 0)
    pc, _, dist, dirs = torch.ops.ngm355.sample_rays(cfg_blob(rc), ijs, None, near, far, gt, u_coarse, u_guided, int(seed),
                                                     0.0, 8.0, S)
    return pc, dist, dirs


def sample_rays_world(rc: K.RenderCfg, ijs, c2ws, near=None, far=None, gt=None, u_coarse=None, u_guided=None, seed=0,
                      near_const=0.0, far_const=8.0):
    """sampler + utils.transform_points (rm.py:513-547): (points_cam, points_world, distances), each (F,R,S,.)."""
    _require_gpu(ijs, c2ws, near, far, gt, u_coarse, u_guided)
    if ijs.dim() == 2:
        ijs = ijs[None]
    S = rc.num_samples_coarse + (rc.num_samples_guided if gt is not None else 0)
    pc, pw, dist, _ = torch.ops.ngm355.sample_rays(cfg_blob(rc), ijs, c2ws, near, far, gt, u_coarse, u_guided, int(seed),
                                                   float(near_const), float(far_const), S)
    return pc, pw, dist


@_op("sample_rays_weighted")
def _sample_rays_weighted_op(rcfg: torch.Tensor, ijs: torch.Tensor, boundaries: torch.Tensor, weights: torch.Tensor,
                             u_bin: Optional[torch.Tensor], u_off: Optional[torch.Tensor], seed: int) -> List[torch.Tensor]:
    """[points_cam (F,R,S,3), distances (F,R,S), dirs (F,R,3)]"""
    rc = _render_cfg(rcfg)
    dev = ijs.device
    F, R, S, B = ijs.shape[0], ijs.shape[1], rc.num_samples_coarse, weights.shape[-1]
    pos, quat = torch.zeros(F, 3, device=dev), torch.zeros(F, 4, device=dev)
    keep = []
    rays = make_rays(rc, ijs, torch.eye(4, device=dev), None, None, None, pos, quat, u_bin, u_off, seed, keep=keep)
    bd, w = _f32c(boundaries), _f32c(weights)
    pc = torch.empty(F, R, S, 3, device=dev)
    dist = torch.empty(F, R, S, device=dev)
    dirs = torch.empty(F, R, 3, device=dev)
    K.check(K.lib().ngm_sample_rays_weighted(C.byref(rc), C.byref(rays), B, _ptr(bd), _ptr(w), _ptr(pc), _ptr(dist), _ptr(dirs),
                                             _stream()), "ngm_sample_rays_weighted")
    return [pc, dist, dirs]


@_sample_rays_weighted_op.register_fake
def _(rcfg, ijs, boundaries, weights, u_bin, u_off, seed):
    F, R, S = ijs.shape[0], ijs.shape[1], _render_cfg(rcfg).num_samples_coarse
    f = lambda *shape: torch.empty(*shape, device=ijs.device, dtype=torch.float32)
    return [f(F, R, S, 3), f(F, R, S), f(F, R, 3)]


def sample_rays_weighted(rc: K.RenderCfg, ijs, boundaries, weights, u_bin=None, u_off=None, seed=0):
    """Camera.sample_ijs_uniform(ijs, num_samples, weights=..., boundaries=...) (camera.py:277-289): weighted sampling from
    per-ray distance bins -> (points_cam (F,R,S,3), distances (F,R,S) in draw order, dirs (F,R,3)); S = rc.num_samples_coarse.
    ijs (F,R,2) int64, boundaries (F,R,B+1) sorted, weights (F,R,B); u_bin / u_off (F,R,S): the reference's two torch.rand
    draws, in its order, or both None = in-kernel Philox."""
    if (weights is None) != (boundaries is None):
        raise ValueError("Either both or none of weights and boundaries must be None.")       # camera.py:260-261
    if weights is None:
        raise ValueError("sample_rays_weighted: boundaries and weights are required (the stratified branch is sample_rays)")
    if (u_bin is None) != (u_off is None):
        raise ValueError("sample_rays_weighted: u_bin and u_off go together (both None = in-kernel Philox)")
    _require_gpu(ijs, boundaries, weights, u_bin, u_off)
    if ijs.dim() == 2:
        ijs, boundaries, weights = ijs[None], boundaries[None], weights[None]
        u_bin, u_off = (None if u_bin is None else u_bin[None]), (None if u_off is None else u_off[None])
    if boundaries.shape[:-1] != ijs.shape[:-1] or weights.shape[:-1] != ijs.shape[:-1] or boundaries.shape[-1] != weights.shape[-1] + 1:
        raise ValueError("boundaries (..., num_bins + 1) and weights (..., num_bins) must match the leading dims of ijs")
    want = (*ijs.shape[:-1], int(rc.num_samples_coarse))            # the kernel indexes the draws as (F, R, S)
    for name, u in (("u_bin", u_bin), ("u_off", u_off)):
        if u is not None and tuple(u.shape) != want:
            raise ValueError(f"sample_rays_weighted: {name} must have shape {want} (leading dims of ijs, num_samples), got {tuple(u.shape)}")
    pc, dist, dirs = torch.ops.ngm355.sample_rays_weighted(cfg_blob(rc), ijs, boundaries, weights, u_bin, u_off, int(seed))
    return pc, dist, dirs


@_op("composite_packed")
def _composite_packed_op(rcfg: torch.Tensor, field_out4: torch.Tensor, dists: torch.Tensor,
                         points_cam: torch.Tensor) -> List[torch.Tensor]:
    rc = _render_cfg(rcfg)
    N, S = dists.shape
    dev = dists.device
    rgbd, cv, dv, term = (torch.empty(N, 4, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, device=dev),
                          torch.empty(N, device=dev))
    K.check(K.lib().ngm_composite_fwd_packed(C.byref(rc), N, S, _ptr(field_out4), _ptr(dists), _ptr(points_cam), _ptr(rgbd),
                                             _ptr(cv), _ptr(dv), _ptr(term), _stream()), "ngm_composite_fwd_packed")
    return [rgbd, cv, dv, term]


@_composite_packed_op.register_fake
def _(rcfg, field_out4, dists, points_cam):
    N = dists.shape[0]
    return [dists.new_empty(N, 4), dists.new_empty(N, 3), dists.new_empty(N), dists.new_empty(N)]


def composite_packed(rc: K.RenderCfg, field_out4, dists, points_cam):
    """_quadrature on the raw (N,S,4) field outputs (eval path): -> rgbd (N,4), Cvar (N,3), Dvar (N), term (N)."""
    _require_gpu(field_out4, dists, points_cam)
    S = dists.shape[-1]
    N = dists.numel() // S
    return tuple(torch.ops.ngm355.composite_packed(cfg_blob(rc), _f32c(field_out4).reshape(N, S, 4), _f32c(dists).reshape(N, S),
                                                   _f32c(points_cam).reshape(N, S, 3)))


@_op("render_eval_knn")
def _render_eval_knn_op(fcfg: torch.Tensor, rcfg: torch.Tensor, ijs: torch.Tensor, c2ws: torch.Tensor,
                        near: Optional[torch.Tensor], far: Optional[torch.Tensor], u: Optional[torch.Tensor], seed: int,
                        near_const: float, far_const: float, pos: torch.Tensor, quat: torch.Tensor, params: List[torch.Tensor],
                        num_knn: int, distance_factor: float, outside_value: float, field_index: Optional[torch.Tensor],
                        mask_radius: float, ray_block: int) -> List[torch.Tensor]:
    fc, rc = _field_cfg(fcfg), _render_cfg(rcfg)
    N, NF = ijs.shape[0], pos.shape[0]
    dev = ijs.device
    rgbd, cv, dv, term = (torch.empty(N, 4, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, device=dev),
                          torch.empty(N, device=dev))
    if N == 0:
        return [rgbd, cv, dv, term]
    ps = params_struct(fc, dict(zip(K.param_names(fc), params)), field_index)
    keep = []
    rays = make_rays(rc, ijs[None], c2ws, None if near is None else near[None], None if far is None else far[None], None,
                     pos[:1], quat[:1], None if u is None else u[None], None, seed, near_const=near_const, far_const=far_const,
                     keep=keep)
    pred = K.Prediction(_ptr(rgbd), _ptr(cv), _ptr(dv), _ptr(term))
    L = K.lib()
    ray_block = max(1, min(int(ray_block), N))
    wsb = L.ngm_render_eval_knn_workspace(C.byref(rc), NF, ray_block, num_knn)
    if wsb < 0:
        raise K.NgmError("ngm_render_eval_knn_workspace: bad argument")
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    K.check(L.ngm_render_eval_knn(C.byref(fc), C.byref(rc), C.byref(ps), NF, _ptr(_f32c(pos)), _ptr(_f32c(quat)), C.byref(rays),
                                  num_knn, distance_factor, outside_value, mask_radius, ray_block, C.byref(pred), _ptr(ws), wsb,
                                  _stream()), "ngm_render_eval_knn")
    return [rgbd, cv, dv, term]


@_render_eval_knn_op.register_fake
def _(fcfg, rcfg, ijs, c2ws, near, far, u, seed, near_const, far_const, pos, quat, params, num_knn, distance_factor,
      outside_value, field_index, mask_radius, ray_block):
    N = ijs.shape[0]
    f = lambda *shape: torch.empty(*shape, device=ijs.device, dtype=torch.float32)
    return [f(N, 4), f(N, 3), f(N), f(N)]


def render_eval_knn(fc, rc: K.RenderCfg, params, ijs, c2ws, pos, quat, num_knn=2, distance_factor=10.0, outside_value=1.0,
                    near=None, far=None, u=None, seed=0, near_const=0.0, far_const=8.0, field_index=None, mask_radius=None,
                    ray_block=8192):
    """render_image's block loop (rm.py:402-437) in one call: eval-style samples of the rays `ijs` (N,2) -> kNN-blended
    fields -> quadrature; -> (rgbd (N,4), color_vars (N,3), depth_vars (N,), term (N,)).  The results equal
    sample_rays_world -> field_eval_knn -> composite_packed per block of `ray_block` rays (block b drawing with seed +
    b * ray_block); the samples, the blended outputs and the camera-frame points never reach memory.
    Dispatches through torch.ops.ngm355.render_eval_knn."""
    plist = [params[n] for n in K.param_names(fc)]
    _require_gpu(ijs, c2ws, pos, quat, near, far, u, *plist)
    if ijs.dtype != torch.int64 or ijs.dim() != 2:
        raise TypeError("ijs must be int64 (N,2) [row, col]")
    return tuple(torch.ops.ngm355.render_eval_knn(cfg_blob(fc), cfg_blob(rc), ijs.contiguous(), c2ws, near, far, u, int(seed),
                                                  float(near_const), float(far_const), pos, quat, plist, int(num_knn),
                                                  float(distance_factor), float(outside_value), field_index,
                                                  float(mask_radius) if mask_radius else 0.0, int(ray_block)))


# ------------------------------------------------------------------------------------------------
# fused render (NeuralGraphMap._render_ijs(use_vmap=True), rm.py:439-666) with autograd
# ------------------------------------------------------------------------------------------------
def _rays_from(rc, ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, seed, near_const, far_const, keep):
    return make_rays(rc, ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, seed, near_const=near_const,
                     far_const=far_const, keep=keep)


@_op("render_ijs")
def _render_ijs_op(fcfg: torch.Tensor, rcfg: torch.Tensor, ijs: torch.Tensor, c2ws: torch.Tensor, near: Optional[torch.Tensor],
                   far: Optional[torch.Tensor], gt: Optional[torch.Tensor], pos: torch.Tensor, quat: torch.Tensor,
                   u_coarse: Optional[torch.Tensor], u_guided: Optional[torch.Tensor], seed: int, near_const: float,
                   far_const: float, save: bool, num_samples: int, workspace_bytes: int,
                   params: List[torch.Tensor]) -> List[torch.Tensor]:
    """[rgbds (F,R,4), color_vars (F,R,3), depth_vars (F,R), term_probs (F,R), geoms (F,R,S) | empty, dists (F,R,S) | empty,
    workspace (bytes) | empty]; geoms / dists / workspace are filled when `save` (needed for a backward or for the
    free-space / TSDF vectors of the Prediction)."""
    fc, rc = _field_cfg(fcfg), _render_cfg(rcfg)
    keep = []
    rays = _rays_from(rc, ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, seed, near_const, far_const, keep)
    F, R = rays.F, rays.R
    dev = ijs.device
    S = rc.num_samples_coarse + (rc.num_samples_guided if gt is not None else 0)
    assert S == num_samples
    rgbds, cvars, dvars, term = (torch.empty(F, R, 4, device=dev), torch.empty(F, R, 3, device=dev),
                                 torch.empty(F, R, device=dev), torch.empty(F, R, device=dev))
    pred = K.Prediction(rgbds.data_ptr(), cvars.data_ptr(), dvars.data_ptr(), term.data_ptr())
    L = K.lib()
    ps = params_struct(fc, dict(zip(K.param_names(fc), params)))
    wsb = L.ngm_render_workspace(C.byref(fc), C.byref(rc), F, R, 1) if save else 0
    if wsb != workspace_bytes:
        raise ValueError(f"render_ijs: workspace_bytes {workspace_bytes} != ngm_render_workspace {wsb}")
    ws = torch.empty(wsb, device=dev, dtype=torch.uint8)
    K.check(L.ngm_render_fwd(C.byref(fc), C.byref(rc), C.byref(ps), C.byref(rays), None, C.byref(pred), None,
                             _ptr(ws) if save else None, wsb, _stream()), "ngm_render_fwd")
    geoms = torch.empty((F, R, S) if save else (0,), device=dev)
    dists = torch.empty((F, R, S) if save else (0,), device=dev)
    if save:
        K.check(L.ngm_render_read_samples(C.byref(fc), C.byref(rc), F, R, S, ws.data_ptr(), geoms.data_ptr(),
                                          dists.data_ptr(), _stream()), "ngm_render_read_samples")
    return [rgbds, cvars, dvars, term, geoms, dists, ws]


@_render_ijs_op.register_fake
def _(fcfg, rcfg, ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, seed, near_const, far_const, save, num_samples,
      workspace_bytes, params):
    F, R, S = ijs.shape[0], ijs.shape[1], num_samples
    f = lambda *shape: torch.empty(*shape, device=ijs.device, dtype=torch.float32)
    n = (F, R, S) if save else (0,)
    return [f(F, R, 4), f(F, R, 3), f(F, R), f(F, R), f(*n), f(*n),
            torch.empty(workspace_bytes, device=ijs.device, dtype=torch.uint8)]


@_op("render_ijs_bwd", mutates_args=("workspace",))
def _render_ijs_bwd_op(fcfg: torch.Tensor, rcfg: torch.Tensor, ijs: torch.Tensor, c2ws: torch.Tensor,
                       near: Optional[torch.Tensor], far: Optional[torch.Tensor], gt: Optional[torch.Tensor],
                       pos: torch.Tensor, quat: torch.Tensor, u_coarse: Optional[torch.Tensor],
                       u_guided: Optional[torch.Tensor], seed: int, near_const: float, far_const: float,
                       d_rgbds: torch.Tensor, d_term: torch.Tensor, d_geoms: Optional[torch.Tensor],
                       workspace: torch.Tensor, params: List[torch.Tensor], d_cvars: Optional[torch.Tensor] = None,
                       d_dvars: Optional[torch.Tensor] = None, rgbds: Optional[torch.Tensor] = None,
                       term: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """gradients w.r.t. `params`; the backward kernels overwrite the saved forward values in `workspace` (single use).
    d_cvars / d_dvars: seeds on the rendered variances (losses.py's *_nll modes); then `rgbds` / `term` = the forward's outputs."""
    fc, rc = _field_cfg(fcfg), _render_cfg(rcfg)
    keep = []
    rays = _rays_from(rc, ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, seed, near_const, far_const, keep)
    names = K.param_names(fc)
    grads, gs = alloc_grads_separate(fc, rays.F, ijs.device)
    ps = params_struct(fc, dict(zip(names, params)))
    if d_cvars is not None or d_dvars is not None:
        pred = K.Prediction(_ptr(rgbds), None, None, _ptr(term))
        K.check(K.lib().ngm_render_bwd_seeded_vars(C.byref(fc), C.byref(rc), C.byref(ps), C.byref(rays), C.byref(pred), _ptr(d_rgbds),
                                                   _ptr(d_cvars), _ptr(d_dvars), _ptr(d_term), _ptr(d_geoms), C.byref(gs),
                                                   workspace.data_ptr(), workspace.numel(), _stream()), "ngm_render_bwd_seeded_vars")
        return [grads[n] for n in names]
    K.check(K.lib().ngm_render_bwd_seeded(C.byref(fc), C.byref(rc), C.byref(ps), C.byref(rays), _ptr(d_rgbds), _ptr(d_term),
                                          _ptr(d_geoms), C.byref(gs), workspace.data_ptr(), workspace.numel(), _stream()),
            "ngm_render_bwd_seeded")
    return [grads[n] for n in names]


@_render_ijs_bwd_op.register_fake
def _(fcfg, rcfg, ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, seed, near_const, far_const, d_rgbds, d_term,
      d_geoms, workspace, params, d_cvars=None, d_dvars=None, rgbds=None, term=None):
    return [torch.empty_like(p, dtype=torch.float32) for p in params]      # gradients are fp32 whatever the storage dtype


_RAY_SLOTS = ("ijs", "c2ws", "near", "far", "gt", "pos", "quat", "u_coarse", "u_guided")


def _render_ijs_setup(ctx, inputs, output):
    fcfg, rcfg, *rest = inputs
    ray_t, (seed, near_const, far_const, save, _, _), params = rest[:9], rest[9:15], rest[15]
    ctx.fcfg, ctx.rcfg, ctx.scalars, ctx.save = fcfg, rcfg, (seed, near_const, far_const), save
    ctx.present = [t is not None for t in ray_t]
    ctx.consumed = False
    # (rgbds and term_probs ride along for seeds on the variances: the means and the weight sum they are taken around)
    ctx.save_for_backward(*[t for t in ray_t if t is not None], output[0], output[3], output[6], *params)
    ctx.n_params = len(params)
    ctx.set_materialize_grads(False)       # an output the loss does not touch arrives as None (color_vars / depth_vars mostly)


def _render_ijs_backward(ctx, grads):
    if not ctx.save:
        raise RuntimeError("render_ijs: backward through a render that saved nothing (call with requires_grad parameters)")
    if ctx.consumed:
        raise RuntimeError("render_ijs: second backward through the same render -- the backward kernels overwrite the "
                           "saved per-sample values in place (single-use workspace, include/ngm_hip.h); render again")
    ctx.consumed = True
    saved = list(ctx.saved_tensors)
    params = saved[len(saved) - ctx.n_params:]
    rgbds, term, ws = saved[len(saved) - ctx.n_params - 3:len(saved) - ctx.n_params]
    it = iter(saved)
    ray_t = [next(it) if p else None for p in ctx.present]
    d_rgbds, d_cvars, d_dvars, d_term, d_geoms, _, _ = grads
    seed, near_const, far_const = ctx.scalars
    d_rgbds = torch.zeros_like(rgbds) if d_rgbds is None else d_rgbds.contiguous()
    d_term = torch.zeros_like(term) if d_term is None else d_term.contiguous()
    d_geoms = None if (d_geoms is None or not d_geoms.numel()) else d_geoms.contiguous()
    if d_cvars is not None or d_dvars is not None:      # the loss reads the rendered variances (losses.py's *_nll modes)
        g = torch.ops.ngm355.render_ijs_bwd(ctx.fcfg, ctx.rcfg, *ray_t, seed, near_const, far_const, d_rgbds, d_term, d_geoms, ws,
                                            params, None if d_cvars is None else d_cvars.contiguous(),
                                            None if d_dvars is None else d_dvars.contiguous(), rgbds, term)
    else:
        g = torch.ops.ngm355.render_ijs_bwd(ctx.fcfg, ctx.rcfg, *ray_t, seed, near_const, far_const, d_rgbds, d_term, d_geoms, ws,
                                            params)
    return (None,) * 17 + (g,)


_render_ijs_op.register_autograd(_render_ijs_backward, setup_context=_render_ijs_setup)


def render_ijs_fused(fc: K.FieldCfg, rc: K.RenderCfg, params: Dict[str, torch.Tensor], ijs, c2ws, near, far, gt, pos, quat,
                     u_coarse=None, u_guided=None, seed=0, near_const=0.0, far_const=8.0):
    """-> (rgbds, color_vars, depth_vars, term_probs, geoms | None, dists | None); differentiable w.r.t. `params` through
    rgbds / color_vars / depth_vars / term_probs / geoms.  Dispatches through torch.ops.ngm355.render_ijs."""
    plist = [params[n] for n in K.param_names(fc)]
    _require_gpu(ijs, c2ws, near, far, gt, pos, quat, u_coarse, u_guided, *plist)
    save = bool(gt is not None or (torch.is_grad_enabled() and any(t.requires_grad for t in plist)))
    if c2ws.dim() != 2 and c2ws.numel() != ijs.shape[0] * ijs.shape[1] * 16:
        c2ws = c2ws.expand(ijs.shape[0], ijs.shape[1], 4, 4)
    wsb = int(K.lib().ngm_render_workspace(C.byref(fc), C.byref(rc), ijs.shape[0], ijs.shape[1], 1)) if save else 0
    if wsb < 0:                                            # a configuration the library refuses: its status and message
        K.check(wsb, "ngm_render_workspace")
    out = torch.ops.ngm355.render_ijs(cfg_blob(fc), cfg_blob(rc), ijs.contiguous(), _f32c(c2ws), _f32c(near), _f32c(far),
                                      _f32c(gt), _f32c(pos), _f32c(quat), _f32c(u_coarse), _f32c(u_guided), int(seed),
                                      float(near_const), float(far_const), save,
                                      rc.num_samples_coarse + (rc.num_samples_guided if gt is not None else 0), wsb, plist)
    rgbds, cvars, dvars, term, geoms, dists, _ = out
    # color_vars / depth_vars stay in the graph: a loss that reads them (losses.py's *_nll modes) seeds them, and the backward
    # then runs ngm_render_bwd_seeded_vars; a loss that does not leaves their gradients None (set_materialize_grads(False))
    return (rgbds, cvars, dvars, term, geoms if save else None, dists.detach() if save else None)


# ------------------------------------------------------------------------------------------------
# K4: quadrature with autograd (rm.py:709-799)
# ------------------------------------------------------------------------------------------------
def _s_eff(rc, S):
    return S - 1 if rc.geometry_mode in (K.GEO["density"], K.GEO["neus"]) else S


@_op("quadrature")
def _quadrature_op(rcfg: torch.Tensor, colors: torch.Tensor, geoms: torch.Tensor, dists: torch.Tensor, depths: torch.Tensor,
                   isds: Optional[torch.Tensor], num_weights: int) -> List[torch.Tensor]:
    rc = _render_cfg(rcfg)
    N, S = geoms.shape
    assert num_weights == _s_eff(rc, S)
    dev = geoms.device
    Cc, D, Cv, Dv, T = (torch.empty(N, 3, device=dev), torch.empty(N, device=dev), torch.empty(N, 3, device=dev),
                        torch.empty(N, device=dev), torch.empty(N, device=dev))
    W = torch.empty(N, _s_eff(rc, S), device=dev)
    K.check(K.lib().ngm_composite_fwd(C.byref(rc), N, S, _ptr(colors), _ptr(geoms), _ptr(dists), _ptr(depths),
                                      _ptr(isds), _ptr(Cc), _ptr(D), _ptr(Cv), _ptr(Dv), _ptr(T), _ptr(W),
                                      _stream()), "ngm_composite_fwd")
    return [Cc, D, Cv, Dv, T, W]


@_quadrature_op.register_fake
def _(rcfg, colors, geoms, dists, depths, isds, num_weights):
    N = geoms.shape[0]          # shapes from tensor sizes and ints only: the cfg bytes are not readable under fake mode
    return [geoms.new_empty(N, 3), geoms.new_empty(N), geoms.new_empty(N, 3), geoms.new_empty(N), geoms.new_empty(N),
            geoms.new_empty(N, num_weights)]


@_op("quadrature_bwd")
def _quadrature_bwd_op(rcfg: torch.Tensor, colors: torch.Tensor, geoms: torch.Tensor, dists: torch.Tensor,
                       depths: torch.Tensor, isds: Optional[torch.Tensor], dC: torch.Tensor, dD: torch.Tensor,
                       dT: torch.Tensor, want_isd: bool) -> List[torch.Tensor]:
    rc = _render_cfg(rcfg)
    N, S = geoms.shape
    d_colors, d_geoms = torch.empty_like(colors), torch.empty_like(geoms)
    d_isd = torch.empty(N if want_isd else 0, device=geoms.device)
    K.check(K.lib().ngm_composite_bwd(C.byref(rc), N, S, _ptr(colors), _ptr(geoms), _ptr(dists), _ptr(depths),
                                      _ptr(isds), _ptr(dC), _ptr(dD), _ptr(dT), _ptr(d_colors), _ptr(d_geoms),
                                      _ptr(d_isd) if want_isd else None, _stream()), "ngm_composite_bwd")
    return [d_colors, d_geoms, d_isd]


@_quadrature_bwd_op.register_fake
def _(rcfg, colors, geoms, dists, depths, isds, dC, dD, dT, want_isd):
    return [torch.empty_like(colors), torch.empty_like(geoms), geoms.new_empty(geoms.shape[0] if want_isd else 0)]


def _quadrature_setup(ctx, inputs, output):
    rcfg, colors, geoms, dists, depths, isds, _ = inputs
    ctx.rcfg, ctx.has_isd = rcfg, isds is not None
    ctx.save_for_backward(colors, geoms, dists, depths, *([isds] if isds is not None else []))


def _quadrature_backward(ctx, grads):
    dC, dD, _, _, dT, _ = grads
    colors, geoms, dists, depths, *rest = ctx.saved_tensors
    isds = rest[0] if ctx.has_isd else None
    N = geoms.shape[0]
    z = lambda g, *shape: torch.zeros(*shape, device=geoms.device) if g is None else g.contiguous()
    want = ctx.has_isd and ctx.needs_input_grad[5] and _render_cfg(ctx.rcfg).geometry_mode == K.GEO["neus"]
    d_colors, d_geoms, d_isd = torch.ops.ngm355.quadrature_bwd(ctx.rcfg, colors, geoms, dists, depths, isds, z(dC, N, 3),
                                                               z(dD, N), z(dT, N), bool(want))
    return None, d_colors, d_geoms, None, None, (d_isd if want else None), None


_quadrature_op.register_autograd(_quadrature_backward, setup_context=_quadrature_setup)


def quadrature(rc: K.RenderCfg, sample_colors, sample_geometries, sample_distances, sample_depths, neus_isds=None):
    """Returns (ray_colors, ray_depths, ray_color_vars, ray_depth_vars, ray_term_probs, sample_weights).
    NeuralGraphMap._quadrature (rm.py:709-799) with autograd; dispatches through torch.ops.ngm355.quadrature."""
    _require_gpu(sample_colors, sample_geometries, sample_distances, sample_depths, neus_isds)
    lead = sample_geometries.shape[:-1]
    S = sample_geometries.shape[-1]
    N = sample_geometries.numel() // S
    isd_flat = None
    if neus_isds is not None:                        # one value per ray (autograd undoes the broadcast)
        isd_flat = neus_isds.expand(*lead, 1).reshape(N).contiguous().float()
    Cc, D, Cv, Dv, T, W = torch.ops.ngm355.quadrature(
        cfg_blob(rc), _f32c(sample_colors).reshape(N, S, 3), _f32c(sample_geometries).reshape(N, S),
        _f32c(sample_distances).reshape(N, S), _f32c(sample_depths).reshape(N, S), isd_flat, _s_eff(rc, S))
    return (Cc.view(*lead, 3), D.view(*lead), Cv.detach().view(*lead, 3), Dv.detach().view(*lead), T.view(*lead),
            W.detach().view(*lead, W.shape[-1]))


# ------------------------------------------------------------------------------------------------
# sparse Adam
# ------------------------------------------------------------------------------------------------
@_op("adam_sparse_", mutates_args=("param", "exp_avg", "exp_avg_sq"))
def _adam_sparse_op(param: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, grad: torch.Tensor,
                    field_index: torch.Tensor, step: int, lr: float, beta1: float, beta2: float, eps: float,
                    weight_decay: float) -> None:
    F = grad.shape[0]
    numel = grad[0].numel()
    K.check(K.lib().ngm_adam_sparse(_ptr(param), _ptr(exp_avg), _ptr(exp_avg_sq), param.stride(0), _ptr(grad),
                                    grad.stride(0), _ptr(field_index), F, numel, int(step), lr, beta1, beta2, eps,
                                    weight_decay, _stream()), "ngm_adam_sparse")


def adam_sparse_(param, exp_avg, exp_avg_sq, grad, field_index, step, lr=1e-3, betas=(0.9, 0.999), eps=1e-15,
                 weight_decay=1e-5):
    """In-place Adam on rows `field_index` of stacked tensors (N, ...); grad is (F, ...).
    torch.ops.ngm355.adam_sparse_ (declared as mutating param / exp_avg / exp_avg_sq)."""
    _require_gpu(param, exp_avg, exp_avg_sq, grad, field_index)
    torch.ops.ngm355.adam_sparse_(param, exp_avg, exp_avg_sq, grad, field_index, int(step), float(lr), float(betas[0]),
                                  float(betas[1]), float(eps), float(weight_decay))


def _adam_tensor(p, st, g, lp=None):
    t = K.AdamTensor(p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), g.data_ptr(), p.stride(0), g.stride(0),
                     g[0].numel())
    if lp is not None and lp.dtype != torch.float32:      # reduced-precision copy the kernels read: refreshed by the update
        if lp.shape != p.shape or lp.stride(0) != p.stride(0):
            raise ValueError("reduced-precision copy must mirror the master tensor's layout")
        t.param_lp, t.lp_dtype = lp.data_ptr(), _TORCH_DT[lp.dtype]
    return t


def adam_tensor_arrays(fc, params, state, grads, lp=None):
    """(mlp AdamTensor array in gradient-segment order, lattice AdamTensor or None) for ngm_render_bwd_adam.
    `params` = fp32 master weights; `lp` (optional dict) = their reduced-precision copies, kept in sync by the update."""
    names = [n for n in K.param_names(fc) if n not in K.NO_GRAD_PARAMS]
    mlp = [n for n in names if n not in ("_encoding.lattice_values", "_encoding.plane_coef")]   # these two: own reduction kernels
    arr = (K.AdamTensor * len(mlp))()
    for i, n in enumerate(mlp):
        arr[i] = _adam_tensor(params[n], state[n], grads[n], None if lp is None else lp[n])
    lat = None
    if "_encoding.lattice_values" in names:
        n = "_encoding.lattice_values"
        lat = (K.AdamTensor * 1)(_adam_tensor(params[n], state[n], grads[n], None if lp is None else lp[n]))
    return arr, len(mlp), lat


def adam_sparse_multi_(fc, params, state, grads, field_index, step, step_dev=None, lr=1e-3, betas=(0.9, 0.999),
                       eps=1e-15, weight_decay=1e-5, advance=False, philox_offset_dev=None, lp=None):
    """One launch for every parameter tensor of the field set (rows `field_index` updated in place)."""
    names = [n for n in K.param_names(fc) if n not in K.NO_GRAD_PARAMS]
    arr = (K.AdamTensor * len(names))()
    for i, n in enumerate(names):
        arr[i] = _adam_tensor(params[n], state[n], grads[n], None if lp is None else lp[n])
    K.check(K.lib().ngm_adam_sparse_multi(arr, len(names), _ptr(field_index), grads[names[0]].shape[0], int(step),
                                          _ptr(step_dev), lr, betas[0], betas[1], eps, weight_decay,
                                          int(bool(advance and step_dev is not None)),
                                          _ptr(philox_offset_dev) if advance else None, _stream()),
            "ngm_adam_sparse_multi")


# ------------------------------------------------------------------------------------------------
# training-target sampler, device part (rm.py:1321-1459)
# ------------------------------------------------------------------------------------------------
def keyframes_struct(c2ws, rgbd_store, frame_to_store, fx, fy, cx, cy) -> K.Keyframes:
    """c2ws (Nc,4,4), rgbd_store (N,H,W,4), frame_to_store (Nc,) int64; intrinsics at pixel centre 0."""
    _require_gpu(c2ws, rgbd_store, frame_to_store)
    assert c2ws.is_contiguous() and rgbd_store.is_contiguous() and frame_to_store.dtype == torch.int64
    kf = K.Keyframes()
    kf.num_frames, kf.height, kf.width = c2ws.shape[0], rgbd_store.shape[1], rgbd_store.shape[2]
    kf.c2ws = C.cast(c2ws.data_ptr(), K.f32p)
    kf.rgbd = C.cast(rgbd_store.data_ptr(), K.f32p)
    kf.frame_to_store = frame_to_store.data_ptr()
    kf.fx, kf.fy, kf.cx, kf.cy = float(fx), float(fy), float(cx), float(cy)
    return kf


def target_visibility(kf: K.Keyframes, field_pos, offsets, radius):
    """(kf_mask (F,Nc) bool, bbox (F,Nc,4) [min_x, min_y, max_x, max_y] clamped to the image)."""
    field_pos, offsets = _f32c(field_pos), _f32c(offsets)
    F, Nc = field_pos.shape[0], kf.num_frames
    mask = torch.empty(F, Nc, dtype=torch.uint8, device=field_pos.device)
    bbox = torch.empty(F, Nc, 4, device=field_pos.device)
    K.check(K.lib().ngm_target_visibility(C.byref(kf), F, _ptr(field_pos), offsets.shape[0], _ptr(offsets), float(radius),
                                          _ptr(mask), _ptr(bbox), _stream()), "ngm_target_visibility")
    return mask.bool(), bbox


def target_rays(kf: K.Keyframes, field_pos, radius, bbox, frame_cids, u_xy):
    """Per-ray targets (rm.py:1394-1459) as a dict keyed like the reference's Target record."""
    field_pos, bbox, u_xy = _f32c(field_pos), _f32c(bbox), _f32c(u_xy)
    frame_cids = frame_cids.contiguous()
    F, R = frame_cids.shape
    dev = field_pos.device
    o = dict(ijs=torch.empty(F, R, 2, dtype=torch.int64, device=dev), c2ws=torch.empty(F, R, 4, 4, device=dev),
             near=torch.empty(F, R, device=dev), far=torch.empty(F, R, device=dev), gt=torch.empty(F, R, device=dev),
             rgbds=torch.empty(F, R, 4, device=dev), rgb_mask=torch.empty(F, R, dtype=torch.uint8, device=dev),
             depth_mask=torch.empty(F, R, dtype=torch.uint8, device=dev), term_probs=torch.empty(F, R, device=dev),
             term_mask=torch.empty(F, R, dtype=torch.uint8, device=dev))
    out = K.TargetOut()
    out.ijs = o["ijs"].data_ptr()
    for k in ("c2ws", "near", "far", "gt", "rgbds", "term_probs"):
        setattr(out, k, C.cast(o[k].data_ptr(), K.f32p))
    for k in ("rgb_mask", "depth_mask", "term_mask"):
        setattr(out, k, o[k].data_ptr())
    K.check(K.lib().ngm_target_rays(C.byref(kf), F, R, _ptr(field_pos), float(radius), _ptr(bbox), _ptr(frame_cids),
                                    _ptr(u_xy), C.byref(out), _stream()), "ngm_target_rays")
    for k in ("rgb_mask", "depth_mask", "term_mask"):
        o[k] = o[k].bool()
    return o


def target_sv_intersect(pos_c, points, radius):
    """(F, N) bool: the segment camera origin -> point n passes through the sphere of field f (geometry.py:67-105)."""
    pos_c, points = _f32c(pos_c), _f32c(points)
    F, N = pos_c.shape[0], points.shape[0]
    hit = torch.empty(F, N, dtype=torch.uint8, device=points.device)
    K.check(K.lib().ngm_target_sv_intersect(F, N, _ptr(pos_c), _ptr(points), float(radius), _ptr(hit), _stream()),
            "ngm_target_sv_intersect")
    return hit.bool()


def target_sv_rays(pos_c, radius, pts_ijs, segments, image, fx, fy, cx, cy):
    """Per-ray targets of the single-view sampler (rm.py:1536-1561), keyed like the reference's Target record."""
    pos_c, image = _f32c(pos_c), _f32c(image)
    _require_gpu(pos_c, image, pts_ijs, segments)
    if pts_ijs.dtype != torch.int64 or segments.dtype != torch.int64:
        raise TypeError(f"target_sv_rays: pts_ijs / segments must be int64 (got {pts_ijs.dtype}, {segments.dtype})")
    pts_ijs, segments = pts_ijs.contiguous(), segments.contiguous()
    F, R = segments.shape
    H, W = image.shape[0], image.shape[1]
    if segments.numel() and (int(segments.min()) < 0 or int(segments.max()) >= pts_ijs.shape[0]):
        raise IndexError("target_sv_rays: segment index outside the point list")
    if pts_ijs.numel() and (int(pts_ijs[:, 0].min()) < 0 or int(pts_ijs[:, 0].max()) >= H or int(pts_ijs[:, 1].min()) < 0
                            or int(pts_ijs[:, 1].max()) >= W):
        raise IndexError("target_sv_rays: pixel index outside the frame")
    dev = pos_c.device
    o = dict(ijs=torch.empty(F, R, 2, dtype=torch.int64, device=dev), near=torch.empty(F, R, device=dev),
             far=torch.empty(F, R, device=dev), gt=torch.empty(F, R, device=dev), rgbds=torch.empty(F, R, 4, device=dev),
             rgb_mask=torch.empty(F, R, dtype=torch.uint8, device=dev), depth_mask=torch.empty(F, R, dtype=torch.uint8, device=dev),
             term_probs=torch.empty(F, R, device=dev), term_mask=torch.empty(F, R, dtype=torch.uint8, device=dev))
    out = K.TargetOut()
    out.ijs = o["ijs"].data_ptr()
    for k in ("near", "far", "gt", "rgbds", "term_probs"):
        setattr(out, k, C.cast(o[k].data_ptr(), K.f32p))
    for k in ("rgb_mask", "depth_mask", "term_mask"):
        setattr(out, k, o[k].data_ptr())
    K.check(K.lib().ngm_target_sv_rays(F, R, _ptr(pos_c), float(radius), _ptr(pts_ijs), _ptr(segments), _ptr(image), H, W,
                                       float(fx), float(fy), float(cx), float(cy), C.byref(out), _stream()), "ngm_target_sv_rays")
    for k in ("rgb_mask", "depth_mask", "term_mask"):
        o[k] = o[k].bool()
    return o


# ------------------------------------------------------------------------------------------------
# training-target sampler, whole, on the device (include/ngm_hip.h ngm_target_sample_mv)
# ------------------------------------------------------------------------------------------------
TARGET_SAMPLE_MV_OUT = ("ijs", "c2ws", "near", "far", "gt", "field_ids", "rgbds", "rgb_mask", "depth_mask", "term_probs",
                        "term_mask", "count", "subset_observed", "subset_random", "offsets", "frame_cids", "u_xy")
TARGET_SAMPLE_MV_LIVE_OUT = TARGET_SAMPLE_MV_OUT + ("num_observed", "num_random")


def _target_sample_mv_shapes(n_obs, n_rand, cap, R):
    """(shape, dtype) of every output of torch.ops.ngm355.target_sample_mv, in TARGET_SAMPLE_MV_OUT order"""
    f32, i64, b = torch.float32, torch.int64, torch.bool
    return [((cap, R, 2), i64), ((cap, R, 4, 4), f32), ((cap, R), f32), ((cap, R), f32), ((cap, R), f32), ((cap,), i64),
            ((cap, R, 4), f32), ((cap, R), b), ((cap, R), b), ((cap, R), f32), ((cap, R), b), ((1,), torch.int32),
            ((n_obs,), i64), ((n_rand,), i64), ((20, 3), f32), ((cap, R), i64), ((cap, R, 2), f32)]


def _target_sample_mv_empty(live, num_current, device, num_fields, num_train_fields, num_rays, world_size, rank):
    """(n_obs, n_rand, capacity, outputs): the host-side plan and the unwritten outputs of torch.ops.ngm355.target_sample_mv
    (live: target_sample_mv_live, num_current its maximum) in TARGET_SAMPLE_MV_OUT (TARGET_SAMPLE_MV_LIVE_OUT) order --
    all a fake implementation returns"""
    plan = K.target_sample_mv_live_plan if live else K.target_sample_mv_plan
    n_obs, n_rand, cap = plan(num_current, num_fields, num_train_fields, num_rays, world_size, rank)
    shapes = _target_sample_mv_shapes(n_obs, n_rand, cap, num_rays) + ([((1,), torch.int32)] * 2 if live else [])
    return n_obs, n_rand, cap, [torch.empty(shape, dtype=dt, device=device) for shape, dt in shapes]


def _target_sample_mv_call(current_field_ids, counts, c2ws, rgbd_store, frame_to_store, field_positions, iteration_dev, intrinsics,
                           radius, num_fields, num_train_fields, num_rays, seed, iteration, world_size, rank, num_fields_dev=None):
    """All three ops: counts = None calls ngm_target_sample_mv, counts = (current_count, num_frames) ngm_target_sample_mv_live
    (current_field_ids / c2ws / frame_to_store are then sized for their maxima); with num_fields_dev as well
    ngm_target_sample_mv_grow (num_fields is the capacity max_fields then)"""
    live = counts is not None
    fn = "ngm_target_sample_mv" + ("" if not live else "_live" if num_fields_dev is None else "_grow")
    num_current, dev = current_field_ids.shape[0], field_positions.device
    n_obs, n_rand, cap, outs = _target_sample_mv_empty(live, num_current, dev, num_fields, num_train_fields, num_rays, world_size, rank)
    o = dict(zip(TARGET_SAMPLE_MV_LIVE_OUT, outs))
    kf = keyframes_struct(c2ws, rgbd_store, frame_to_store, *intrinsics)
    ws_bytes = getattr(K.lib(), fn + "_workspace")(kf.num_frames, num_current, num_fields, cap)
    if ws_bytes < 0:
        raise K.NgmError(fn + "_workspace: bad sizes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    s = K.TargetSample(_ptr(current_field_ids), _ptr(field_positions), num_current, num_fields, n_obs, n_rand,
                       num_rays, cap, world_size, rank, float(radius), 0, int(seed), int(iteration), _ptr(iteration_dev))
    for k in ("field_ids", "count", "subset_observed", "subset_random", "offsets", "frame_cids", "u_xy"):
        setattr(s, k, o[k].data_ptr())
    out = K.TargetOut()
    for k in ("ijs", "c2ws", "near", "far", "gt", "rgbds", "rgb_mask", "depth_mask", "term_probs", "term_mask"):
        setattr(out, k, o[k].data_ptr())
    args = [C.byref(kf), C.byref(s), C.byref(out), _ptr(ws), ws_bytes, _stream()]
    if live:
        lv = K.TargetLive(_ptr(counts[0]), _ptr(counts[1]), o["num_observed"].data_ptr(), o["num_random"].data_ptr(),
                          num_train_fields, 0)
        args.insert(2, C.byref(lv))
        if num_fields_dev is not None:
            args.insert(3, _ptr(num_fields_dev))
    K.check(getattr(K.lib(), fn)(*args), fn)
    return outs


@_op("target_sample_mv", mutates_args=("iteration_dev",))
def _target_sample_mv_op(current_field_ids: torch.Tensor, c2ws: torch.Tensor, rgbd_store: torch.Tensor,
                         frame_to_store: torch.Tensor, field_positions: torch.Tensor, iteration_dev: Optional[torch.Tensor],
                         intrinsics: List[float], radius: float, num_fields: int, num_train_fields: int, num_rays: int,
                         seed: int, iteration: int, world_size: int, rank: int) -> List[torch.Tensor]:
    """TARGET_SAMPLE_MV_OUT, every per-field array at the host-known capacity (rows past count: padding)"""
    return _target_sample_mv_call(current_field_ids, None, c2ws, rgbd_store, frame_to_store, field_positions, iteration_dev,
                                  intrinsics, radius, num_fields, num_train_fields, num_rays, seed, iteration, world_size, rank)


@_target_sample_mv_op.register_fake
def _(current_field_ids, c2ws, rgbd_store, frame_to_store, field_positions, iteration_dev, intrinsics, radius, num_fields,
      num_train_fields, num_rays, seed, iteration, world_size, rank):
    return _target_sample_mv_empty(False, current_field_ids.shape[0], field_positions.device, num_fields, num_train_fields,
                                   num_rays, world_size, rank)[3]


# the same sampler with its counts in device memory (include/ngm_hip.h ngm_target_sample_mv_live)
@_op("target_sample_mv_live", mutates_args=("iteration_dev",))
def _target_sample_mv_live_op(current_field_ids: torch.Tensor, current_count: torch.Tensor, c2ws: torch.Tensor,
                              num_frames: torch.Tensor, rgbd_store: torch.Tensor, frame_to_store: torch.Tensor,
                              field_positions: torch.Tensor, iteration_dev: Optional[torch.Tensor], intrinsics: List[float],
                              radius: float, num_fields: int, num_train_fields: int, num_rays: int, seed: int, iteration: int,
                              world_size: int, rank: int) -> List[torch.Tensor]:
    """TARGET_SAMPLE_MV_LIVE_OUT; current_field_ids / c2ws / frame_to_store are sized for their maxima, the counts in force
    are current_count / num_frames (device int32)"""
    return _target_sample_mv_call(current_field_ids, (current_count, num_frames), c2ws, rgbd_store, frame_to_store, field_positions,
                                  iteration_dev, intrinsics, radius, num_fields, num_train_fields, num_rays, seed, iteration,
                                  world_size, rank)


@_target_sample_mv_live_op.register_fake
def _(current_field_ids, current_count, c2ws, num_frames, rgbd_store, frame_to_store, field_positions, iteration_dev, intrinsics,
      radius, num_fields, num_train_fields, num_rays, seed, iteration, world_size, rank):
    return _target_sample_mv_empty(True, current_field_ids.shape[0], field_positions.device, num_fields, num_train_fields,
                                   num_rays, world_size, rank)[3]


# the live sampler over reserved field rows (include/ngm_hip.h ngm_target_sample_mv_grow)
@_op("target_sample_mv_grow", mutates_args=("iteration_dev",))
def _target_sample_mv_grow_op(current_field_ids: torch.Tensor, current_count: torch.Tensor, c2ws: torch.Tensor,
                              num_frames: torch.Tensor, num_fields_dev: torch.Tensor, rgbd_store: torch.Tensor,
                              frame_to_store: torch.Tensor, field_positions: torch.Tensor, iteration_dev: Optional[torch.Tensor],
                              intrinsics: List[float], radius: float, max_fields: int, num_train_fields: int, num_rays: int,
                              seed: int, iteration: int, world_size: int, rank: int) -> List[torch.Tensor]:
    """TARGET_SAMPLE_MV_LIVE_OUT at the sizes of target_sample_mv_live for a map of max_fields fields; the fields in force
    are num_fields_dev (device int32)"""
    return _target_sample_mv_call(current_field_ids, (current_count, num_frames), c2ws, rgbd_store, frame_to_store, field_positions,
                                  iteration_dev, intrinsics, radius, max_fields, num_train_fields, num_rays, seed, iteration,
                                  world_size, rank, num_fields_dev=num_fields_dev)


@_target_sample_mv_grow_op.register_fake
def _(current_field_ids, current_count, c2ws, num_frames, num_fields_dev, rgbd_store, frame_to_store, field_positions, iteration_dev,
      intrinsics, radius, max_fields, num_train_fields, num_rays, seed, iteration, world_size, rank):
    return _target_sample_mv_empty(True, current_field_ids.shape[0], field_positions.device, max_fields, num_train_fields,
                                   num_rays, world_size, rank)[3]


def _check_device_count(fn, name, t):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() != 1:
        raise TypeError(f"{fn}: {name} must be a one-element int32 tensor")


def _target_sample_mv_checked(fn, current_field_ids, counts, c2ws, rgbd_store, frame_to_store, field_positions, intrinsics, radius,
                              num_fields, num_train_fields, num_rays, seed, iteration, iteration_dev, world_size, rank,
                              num_fields_dev=None):
    """The public wrappers' checks under the caller's name `fn`, then its op; the outputs as a dict"""
    live = counts is not None
    if num_fields_dev is not None:
        _check_device_count(fn, "num_fields_dev", num_fields_dev)

    def need(cond, msg, exc=ValueError):
        if not cond:
            raise exc("target_sample_mv: " + msg)
    for name, t, dt in (("current_field_ids", current_field_ids, torch.int64), ("c2ws", c2ws, torch.float32),
                        ("rgbd_store", rgbd_store, torch.float32), ("frame_to_store", frame_to_store, torch.int64),
                        ("field_positions", field_positions, torch.float32)):
        need(isinstance(t, torch.Tensor), f"{name} must be a tensor", TypeError)
        need(t.dtype == dt, f"{name} must be {dt}, got {t.dtype}", TypeError)
        need(t.is_contiguous(), f"{name} must be contiguous")
    need(current_field_ids.dim() == 1, f"current_field_ids must be 1-D, got shape {tuple(current_field_ids.shape)}")
    need(c2ws.dim() == 3 and tuple(c2ws.shape[1:]) == (4, 4) and c2ws.shape[0] >= 1, f"c2ws must be (Nc>=1, 4, 4), got {tuple(c2ws.shape)}")
    need(rgbd_store.dim() == 4 and rgbd_store.shape[3] == 4, f"rgbd_store must be (N, H, W, 4), got {tuple(rgbd_store.shape)}")
    need(tuple(frame_to_store.shape) == (c2ws.shape[0],), f"frame_to_store must be ({c2ws.shape[0]},), got {tuple(frame_to_store.shape)}")
    need(field_positions.dim() == 2 and field_positions.shape[1] == 3 and field_positions.shape[0] >= num_fields,
         f"field_positions must be (>= num_fields = {num_fields}, 3), got {tuple(field_positions.shape)}")
    if iteration_dev is not None:
        need(isinstance(iteration_dev, torch.Tensor) and iteration_dev.dtype == torch.int64 and iteration_dev.numel() == 1,
             "iteration_dev must be a one-element int64 tensor", TypeError)
    for name, t in zip(("current_count", "num_frames"), counts or ()):
        _check_device_count(fn, name, t)
    (K.target_sample_mv_live_plan if live else K.target_sample_mv_plan)(current_field_ids.shape[0], num_fields, num_train_fields,
                                                                        num_rays, world_size, rank)
    if iteration is None and iteration_dev is None:
        raise ValueError(f"{fn}: iteration=None needs iteration_dev (the device counter)")
    if iteration is not None and int(iteration) < 0:
        raise ValueError(f"{fn}: iteration must be >= 0, got {iteration}")
    if not 0 <= int(seed) < 2 ** 63:
        raise ValueError(f"{fn}: seed must be in [0, 2^63), got {seed}")
    _require_gpu(current_field_ids, *(counts or ()), c2ws, rgbd_store, frame_to_store, field_positions, iteration_dev, num_fields_dev)
    tail = (rgbd_store, frame_to_store, field_positions, iteration_dev, intrinsics, float(radius), num_fields, num_train_fields,
            num_rays, int(seed), -1 if iteration is None else int(iteration), world_size, rank)
    if num_fields_dev is not None:
        return dict(zip(TARGET_SAMPLE_MV_LIVE_OUT, torch.ops.ngm355.target_sample_mv_grow(current_field_ids, counts[0], c2ws,
                                                                                          counts[1], num_fields_dev, *tail)))
    if live:
        return dict(zip(TARGET_SAMPLE_MV_LIVE_OUT, torch.ops.ngm355.target_sample_mv_live(current_field_ids, counts[0], c2ws,
                                                                                          counts[1], *tail)))
    return dict(zip(TARGET_SAMPLE_MV_OUT, torch.ops.ngm355.target_sample_mv(current_field_ids, c2ws, *tail)))


def target_sample_mv(current_field_ids, c2ws, rgbd_store, frame_to_store, field_positions, fx, fy, cx, cy, radius, num_fields,
                     num_train_fields, num_rays_per_field, seed=0, iteration=None, iteration_dev=None, world_size=1, rank=0):
    """_sample_target_mv (rm.py:1259-1459) with the draws on the device, three launches, no host synchronisation
    (torch.ops.ngm355.target_sample_mv).  iteration=None: iteration_dev (one-element int64 device tensor) is read and
    advanced by one inside the call; an int uses that iteration and leaves iteration_dev alone.  Returns a dict keyed by
    TARGET_SAMPLE_MV_OUT; per-field arrays have K.target_sample_mv_plan(...)[2] rows, `count` (int32, device) of them valid.
    This and target_sample_mv_live run one implementation."""
    return _target_sample_mv_checked("target_sample_mv", current_field_ids, None, c2ws, rgbd_store, frame_to_store, field_positions,
                                     [float(fx), float(fy), float(cx), float(cy)], radius, int(num_fields), int(num_train_fields),
                                     int(num_rays_per_field), seed, iteration, iteration_dev, int(world_size), int(rank))


def target_sample_mv_live(current_field_ids, current_count, c2ws, num_frames, rgbd_store, frame_to_store, field_positions, fx, fy,
                          cx, cy, radius, num_fields, num_train_fields, num_rays_per_field, seed=0, iteration=None,
                          iteration_dev=None, world_size=1, rank=0):
    """target_sample_mv with the number of current fields and of keyframes read from device memory
    (torch.ops.ngm355.target_sample_mv_live): current_field_ids (max_current,), c2ws (max_frames, 4, 4) and frame_to_store
    (max_frames,) are fixed-capacity buffers, current_count / num_frames one-element int32 device tensors.  Bit for bit
    target_sample_mv(current_field_ids[:n], c2ws[:m], ...) for the counts n, m in force; nothing past them is read.
    Returns a dict keyed by TARGET_SAMPLE_MV_LIVE_OUT: subset_observed / subset_random at their maxima with -1 past
    num_observed / num_random (int32, device)."""
    return _target_sample_mv_checked("target_sample_mv_live", current_field_ids, (current_count, num_frames), c2ws, rgbd_store,
                                     frame_to_store, field_positions, [float(fx), float(fy), float(cx), float(cy)], radius,
                                     int(num_fields), int(num_train_fields), int(num_rays_per_field), seed, iteration, iteration_dev,
                                     int(world_size), int(rank))


def target_sample_mv_grow(current_field_ids, current_count, c2ws, num_frames, num_fields_dev, rgbd_store, frame_to_store,
                          field_positions, fx, fy, cx, cy, radius, max_fields, num_train_fields, num_rays_per_field, seed=0,
                          iteration=None, iteration_dev=None, world_size=1, rank=0):
    """target_sample_mv_live over reserved field rows (torch.ops.ngm355.target_sample_mv_grow): field_positions has
    (>= max_fields, 3) rows, the number of fields in force is num_fields_dev (one-element int32 device tensor, clamped to
    [0, max_fields]).  Every size -- the row capacity K.target_sample_mv_grow_plan(...)[2] included -- follows from
    max_fields; rows below `count` are bit for bit target_sample_mv_live's on a map of exactly that many fields."""
    return _target_sample_mv_checked("target_sample_mv_grow", current_field_ids, (current_count, num_frames), c2ws, rgbd_store,
                                     frame_to_store, field_positions, [float(fx), float(fy), float(cx), float(cy)], radius,
                                     int(max_fields), int(num_train_fields), int(num_rays_per_field), seed, iteration, iteration_dev,
                                     int(world_size), int(rank), num_fields_dev=num_fields_dev)


# ------------------------------------------------------------------------------------------------
# observed fields of one frame, on the device (include/ngm_hip.h ngm_target_observed_fields)
# ------------------------------------------------------------------------------------------------
TARGET_OBSERVED_FIELDS_OUT = ("current_field_ids", "current_count", "pixels", "num_used")


def _target_observed_fields_call(rgbd, c2w, field_positions, frame_dev, subset_in, ids_out, count_out, intrinsics, radius,
                                 num_fields, num_points, seed, frame, num_fields_dev=None):
    """Both ops: ngm_target_observed_fields, or with num_fields_dev ngm_target_observed_fields_grow (num_fields = max_fields)"""
    fn = "ngm_target_observed_fields" + ("" if num_fields_dev is None else "_grow")
    dev = rgbd.device
    H, W = rgbd.shape[0], rgbd.shape[1]
    pixels = torch.empty(num_points, dtype=torch.int64, device=dev)
    used = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = getattr(K.lib(), fn + "_workspace")(H, W)
    if ws_bytes < 0:
        raise K.NgmError(fn + "_workspace: bad sizes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a = K.ObservedFields()
    a.rgbd, a.c2w = C.cast(rgbd.data_ptr(), K.f32p), C.cast(c2w.data_ptr(), K.f32p)
    a.field_positions = C.cast(field_positions.data_ptr(), K.f32p)
    a.height, a.width, a.num_fields, a.num_points = H, W, num_fields, num_points
    a.fx, a.fy, a.cx, a.cy = intrinsics
    a.radius, a.seed, a.frame = float(radius), int(seed), int(frame)
    a.frame_dev, a.subset_in = _ptr(frame_dev), _ptr(subset_in)
    a.current_field_ids, a.current_count = ids_out.data_ptr(), count_out.data_ptr()
    a.pixels, a.num_used = pixels.data_ptr(), used.data_ptr()
    args = [C.byref(a), _ptr(ws), ws_bytes, _stream()]
    if num_fields_dev is not None:
        args.insert(1, _ptr(num_fields_dev))
    K.check(getattr(K.lib(), fn)(*args), fn)
    return [pixels, used]


@_op("target_observed_fields", mutates_args=("frame_dev", "ids_out", "count_out"))
def _target_observed_fields_op(rgbd: torch.Tensor, c2w: torch.Tensor, field_positions: torch.Tensor, frame_dev: Optional[torch.Tensor],
                               subset_in: Optional[torch.Tensor], ids_out: torch.Tensor, count_out: torch.Tensor,
                               intrinsics: List[float], radius: float, num_fields: int, num_points: int, seed: int,
                               frame: int) -> List[torch.Tensor]:
    """(pixels (num_points,) int64, num_used (1,) int32); the observed ids and their count go to ids_out / count_out"""
    return _target_observed_fields_call(rgbd, c2w, field_positions, frame_dev, subset_in, ids_out, count_out, intrinsics, radius,
                                        num_fields, num_points, seed, frame)


@_op("target_observed_fields_grow", mutates_args=("frame_dev", "ids_out", "count_out"))
def _target_observed_fields_grow_op(rgbd: torch.Tensor, c2w: torch.Tensor, field_positions: torch.Tensor, num_fields_dev: torch.Tensor,
                                    frame_dev: Optional[torch.Tensor], subset_in: Optional[torch.Tensor], ids_out: torch.Tensor,
                                    count_out: torch.Tensor, intrinsics: List[float], radius: float, max_fields: int,
                                    num_points: int, seed: int, frame: int) -> List[torch.Tensor]:
    """target_observed_fields over reserved field rows: ids_out has max_fields entries, num_fields_dev fields are tested"""
    return _target_observed_fields_call(rgbd, c2w, field_positions, frame_dev, subset_in, ids_out, count_out, intrinsics, radius,
                                        max_fields, num_points, seed, frame, num_fields_dev=num_fields_dev)


@_target_observed_fields_grow_op.register_fake
def _(rgbd, c2w, field_positions, num_fields_dev, frame_dev, subset_in, ids_out, count_out, intrinsics, radius, max_fields, num_points,
      seed, frame):
    return [torch.empty(num_points, dtype=torch.int64, device=rgbd.device), torch.empty(1, dtype=torch.int32, device=rgbd.device)]


@_target_observed_fields_op.register_fake
def _(rgbd, c2w, field_positions, frame_dev, subset_in, ids_out, count_out, intrinsics, radius, num_fields, num_points, seed, frame):
    return [torch.empty(num_points, dtype=torch.int64, device=rgbd.device), torch.empty(1, dtype=torch.int32, device=rgbd.device)]


def target_observed_fields(rgbd, c2w, field_positions, fx, fy, cx, cy, radius, num_fields, num_points=500, seed=0, frame=None,
                           frame_dev=None, subset_in=None, ids_out=None, count_out=None, num_fields_dev=None):
    """NeuralGraphMap._get_observed_fields (rm.py:1642-1670) on the device (torch.ops.ngm355.target_observed_fields): no host
    synchronisation, fixed shapes.  rgbd (H, W, 4) and c2w (4, 4) are device tensors read when the kernels run.  frame=None:
    frame_dev (one-element int64 device tensor) is read and advanced.  subset_in: num_points linear pixel indices that
    replace the draw.  ids_out (>= num_fields,) int64 / count_out (1,) int32 are written in place when given.  Returns a
    dict keyed by TARGET_OBSERVED_FIELDS_OUT: the observed ids ascending with -1 past current_count, the chosen pixels (order
    unspecified) with -1 past num_used.
    num_fields_dev (one-element int32 device tensor): the map has reserved rows (torch.ops.ngm355.target_observed_fields_grow)
    -- num_fields is then the capacity max_fields (rows of field_positions, entries of ids_out), the fields tested are the
    first clamp(*num_fields_dev, 0, max_fields)."""
    def need(cond, msg, exc=ValueError):
        if not cond:
            raise exc("target_observed_fields: " + msg)
    if num_fields_dev is not None:
        _check_device_count("target_observed_fields", "num_fields_dev", num_fields_dev)
    num_fields, num_points = int(num_fields), int(num_points)
    for name, t in (("rgbd", rgbd), ("c2w", c2w), ("field_positions", field_positions)):
        need(isinstance(t, torch.Tensor), f"{name} must be a tensor", TypeError)
        need(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}", TypeError)
        need(t.is_contiguous(), f"{name} must be contiguous")
    need(rgbd.dim() == 3 and rgbd.shape[2] == 4 and rgbd.shape[0] >= 1 and rgbd.shape[1] >= 1,
         f"rgbd must be (H, W, 4), got {tuple(rgbd.shape)}")
    need(tuple(c2w.shape) == (4, 4), f"c2w must be (4, 4), got {tuple(c2w.shape)}")
    need(num_fields >= 0 and field_positions.dim() == 2 and field_positions.shape[1] == 3 and field_positions.shape[0] >= num_fields,
         f"field_positions must be (>= num_fields = {num_fields}, 3), got {tuple(field_positions.shape)}")
    need(1 <= num_points <= K.NGM_OBSERVED_MAX_POINTS, f"num_points must be in [1, {K.NGM_OBSERVED_MAX_POINTS}], got {num_points}")
    need(frame is not None or frame_dev is not None, "frame=None needs frame_dev (the device counter)")
    need(frame is None or int(frame) >= 0, f"frame must be >= 0, got {frame}")
    need(0 <= int(seed) < 2 ** 63, f"seed must be in [0, 2^63), got {seed}")
    if frame_dev is not None:
        need(isinstance(frame_dev, torch.Tensor) and frame_dev.dtype == torch.int64 and frame_dev.numel() == 1,
             "frame_dev must be a one-element int64 tensor", TypeError)
    if subset_in is not None:
        need(isinstance(subset_in, torch.Tensor) and subset_in.dtype == torch.int64, "subset_in must be an int64 tensor", TypeError)
        need(tuple(subset_in.shape) == (num_points,) and subset_in.is_contiguous(),
             f"subset_in must be a contiguous ({num_points},) tensor, got {tuple(subset_in.shape)}")
    if ids_out is not None:
        need(isinstance(ids_out, torch.Tensor) and ids_out.dtype == torch.int64, "ids_out must be an int64 tensor", TypeError)
        need(ids_out.dim() == 1 and ids_out.shape[0] >= num_fields and ids_out.is_contiguous(),
             f"ids_out must be a contiguous (>= {num_fields},) tensor, got {tuple(ids_out.shape)}")
    if count_out is not None:
        _check_device_count("target_observed_fields", "count_out", count_out)
    _require_gpu(rgbd, c2w, field_positions, frame_dev, subset_in, ids_out, count_out, num_fields_dev)
    dev = rgbd.device
    if ids_out is None:
        ids_out = torch.empty(num_fields, dtype=torch.int64, device=dev)
    if count_out is None:
        count_out = torch.empty(1, dtype=torch.int32, device=dev)
    tail = ([float(fx), float(fy), float(cx), float(cy)], float(radius), num_fields, num_points, int(seed),
            -1 if frame is None else int(frame))
    if num_fields_dev is not None:
        pixels, used = torch.ops.ngm355.target_observed_fields_grow(rgbd, c2w, field_positions, num_fields_dev, frame_dev, subset_in,
                                                                    ids_out, count_out, *tail)
    else:
        pixels, used = torch.ops.ngm355.target_observed_fields(rgbd, c2w, field_positions, frame_dev, subset_in, ids_out, count_out,
                                                               *tail)
    return dict(current_field_ids=ids_out, current_count=count_out, pixels=pixels, num_used=used)


# ------------------------------------------------------------------------------------------------
# single-view training-target sampler, whole, on the device (include/ngm_hip.h ngm_target_sample_sv)
# ------------------------------------------------------------------------------------------------
TARGET_SAMPLE_SV_OUT = ("ijs", "c2ws", "near", "far", "gt", "field_ids", "rgbds", "rgb_mask", "depth_mask", "term_probs",
                        "term_mask", "count", "pixels", "num_used", "hits", "num_candidates", "subset_fields", "segments")


def _target_sample_sv_empty(device, num_active, capacity, num_train_fields, num_rays, num_points):
    """the unwritten outputs of torch.ops.ngm355.target_sample_sv in TARGET_SAMPLE_SV_OUT order -- all a fake implementation
    returns"""
    f32, i64, i32, b = torch.float32, torch.int64, torch.int32, torch.bool
    cap, R = capacity, num_rays
    shapes = [((cap, R, 2), i64), ((cap, R, 4, 4), f32), ((cap, R), f32), ((cap, R), f32), ((cap, R), f32), ((cap,), i64),
              ((cap, R, 4), f32), ((cap, R), b), ((cap, R), b), ((cap, R), f32), ((cap, R), b), ((1,), i32),
              ((num_points,), i64), ((1,), i32), ((num_active,), i32), ((1,), i32), ((num_train_fields,), i64), ((cap, R), i64)]
    return [torch.empty(shape, dtype=dt, device=device) for shape, dt in shapes]


@_op("target_sample_sv", mutates_args=("iteration_dev",))
def _target_sample_sv_op(rgbd: torch.Tensor, c2w: torch.Tensor, slot: Optional[torch.Tensor], active_field_ids: torch.Tensor,
                         field_positions: torch.Tensor, num_fields_dev: Optional[torch.Tensor],
                         iteration_dev: Optional[torch.Tensor], pixels_in: Optional[torch.Tensor],
                         subset_fields_in: Optional[torch.Tensor], segments_in: Optional[torch.Tensor], intrinsics: List[float],
                         radius: float, num_fields: int, num_points: int, num_train_fields: int, num_rays: int, capacity: int,
                         seed: int, iteration: int, world_size: int, rank: int) -> List[torch.Tensor]:
    """TARGET_SAMPLE_SV_OUT, every per-row array at `capacity` (rows past count: padding); rgbd (S,H,W,4), c2w (S,4,4)"""
    dev = rgbd.device
    S, H, W = rgbd.shape[0], rgbd.shape[1], rgbd.shape[2]
    A = active_field_ids.shape[0]
    outs = _target_sample_sv_empty(dev, A, capacity, num_train_fields, num_rays, num_points)
    o = dict(zip(TARGET_SAMPLE_SV_OUT, outs))
    ws_bytes = K.lib().ngm_target_sample_sv_workspace(H, W, A, num_points, capacity)
    if ws_bytes < 0:
        raise K.NgmError("ngm_target_sample_sv_workspace: bad sizes")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a = K.TargetSampleSv()
    a.rgbd, a.c2w = C.cast(rgbd.data_ptr(), K.f32p), C.cast(c2w.data_ptr(), K.f32p)
    a.field_positions = C.cast(field_positions.data_ptr(), K.f32p)
    a.slot_dev, a.active_field_ids, a.num_fields_dev = _ptr(slot), _ptr(active_field_ids), _ptr(num_fields_dev)
    a.num_slots, a.height, a.width, a.num_active, a.num_fields = S, H, W, A, num_fields
    a.num_points, a.num_train_fields, a.num_rays, a.capacity = num_points, num_train_fields, num_rays, capacity
    a.world_size, a.rank = world_size, rank
    a.fx, a.fy, a.cx, a.cy = intrinsics
    a.radius, a.seed, a.iteration, a.iteration_dev = float(radius), int(seed), int(iteration), _ptr(iteration_dev)
    a.pixels_in, a.subset_fields_in, a.segments_in = _ptr(pixels_in), _ptr(subset_fields_in), _ptr(segments_in)
    for k in ("field_ids", "count", "pixels", "num_used", "hits", "num_candidates", "subset_fields", "segments"):
        setattr(a, k, o[k].data_ptr())
    out = K.TargetOut()
    for k in ("ijs", "c2ws", "near", "far", "gt", "rgbds", "rgb_mask", "depth_mask", "term_probs", "term_mask"):
        setattr(out, k, o[k].data_ptr())
    K.check(K.lib().ngm_target_sample_sv(C.byref(a), C.byref(out), _ptr(ws), ws_bytes, _stream()), "ngm_target_sample_sv")
    return outs


@_target_sample_sv_op.register_fake
def _(rgbd, c2w, slot, active_field_ids, field_positions, num_fields_dev, iteration_dev, pixels_in, subset_fields_in, segments_in,
      intrinsics, radius, num_fields, num_points, num_train_fields, num_rays, capacity, seed, iteration, world_size, rank):
    return _target_sample_sv_empty(rgbd.device, active_field_ids.shape[0], capacity, num_train_fields, num_rays, num_points)


def target_sample_sv(rgbd, c2w, active_field_ids, field_positions, fx, fy, cx, cy, radius, num_fields, num_train_fields,
                     num_rays_per_field, num_points=50000, seed=0, iteration=None, iteration_dev=None, world_size=1, rank=0,
                     slot=None, num_fields_dev=None, capacity=None, pixels_in=None, subset_fields_in=None, segments_in=None):
    """_sample_target_sv (rm.py:1461-1583) with the draws on the device, no host synchronisation, fixed shapes
    (torch.ops.ngm355.target_sample_sv; include/ngm_hip.h ngm_target_sample_sv is the contract).  rgbd (H, W, 4) with c2w
    (4, 4), or a frame stack (S, H, W, 4) / (S, 4, 4) with slot = a one-element int32 device tensor naming the frame read.
    active_field_ids (A,) int64, duplicate-free; entries < 0 or past the field count are skipped.  iteration=None:
    iteration_dev (one-element int64 device tensor) is read and advanced by one inside the call.  num_fields_dev: the count in
    force is read on the device (reserved rows; num_fields is the capacity then).  capacity: rows of the outputs, at least
    (and by default) K.target_sample_sv_plan(...).  pixels_in / subset_fields_in / segments_in replay recorded draws
    (world_size 1).  Returns a dict keyed by TARGET_SAMPLE_SV_OUT; `count` (int32, device) rows are valid."""
    def need(cond, msg, exc=ValueError):
        if not cond:
            raise exc("target_sample_sv: " + msg)
    for name, t, dt in (("rgbd", rgbd, torch.float32), ("c2w", c2w, torch.float32), ("field_positions", field_positions, torch.float32),
                        ("active_field_ids", active_field_ids, torch.int64)):
        need(isinstance(t, torch.Tensor), f"{name} must be a tensor", TypeError)
        need(t.dtype == dt, f"{name} must be {dt}, got {t.dtype}", TypeError)
        need(t.is_contiguous(), f"{name} must be contiguous")
    if rgbd.dim() == 3:
        need(slot is None, "slot needs a frame stack: rgbd (S, H, W, 4) and c2w (S, 4, 4)")
        rgbd, c2w = rgbd[None], c2w[None]
    need(rgbd.dim() == 4 and rgbd.shape[3] == 4 and min(rgbd.shape[:3]) >= 1, f"rgbd must be ([S,] H, W, 4), got {tuple(rgbd.shape)}")
    need(tuple(c2w.shape) == (rgbd.shape[0], 4, 4), f"c2w must be ({rgbd.shape[0]}, 4, 4) for this rgbd, got {tuple(c2w.shape)}")
    need(active_field_ids.dim() == 1, f"active_field_ids must be 1-D, got shape {tuple(active_field_ids.shape)}")
    num_fields, T, R, num_points = int(num_fields), int(num_train_fields), int(num_rays_per_field), int(num_points)
    need(field_positions.dim() == 2 and field_positions.shape[1] == 3 and field_positions.shape[0] >= num_fields,
         f"field_positions must be (>= num_fields = {num_fields}, 3), got {tuple(field_positions.shape)}")
    rows = K.target_sample_sv_plan(active_field_ids.shape[0], num_fields, T, R, num_points, int(world_size), int(rank))
    capacity = rows if capacity is None else int(capacity)
    need(rows <= capacity <= K.NGM_TARGET_MAX_DRAW, f"capacity must be in [{rows}, {K.NGM_TARGET_MAX_DRAW}], got {capacity}")
    for name, t in (("slot", slot), ("num_fields_dev", num_fields_dev)):
        if t is not None:
            _check_device_count("target_sample_sv", name, t)
    if iteration_dev is not None:
        need(isinstance(iteration_dev, torch.Tensor) and iteration_dev.dtype == torch.int64 and iteration_dev.numel() == 1,
             "iteration_dev must be a one-element int64 tensor", TypeError)
    need(iteration is not None or iteration_dev is not None, "iteration=None needs iteration_dev (the device counter)")
    need(iteration is None or int(iteration) >= 0, f"iteration must be >= 0, got {iteration}")
    need(0 <= int(seed) < 2 ** 63, f"seed must be in [0, 2^63), got {seed}")
    for name, t, shape in (("pixels_in", pixels_in, (num_points,)), ("subset_fields_in", subset_fields_in, (T,)),
                           ("segments_in", segments_in, (capacity, R))):
        if t is not None:
            need(isinstance(t, torch.Tensor) and t.dtype == torch.int64, f"{name} must be an int64 tensor", TypeError)
            need(tuple(t.shape) == shape and t.is_contiguous(), f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
            need(int(world_size) == 1, "recorded draws are for world_size 1")
    need(segments_in is None or pixels_in is not None, "segments_in indexes pixels_in: give both")
    _require_gpu(rgbd, c2w, active_field_ids, field_positions, slot, num_fields_dev, iteration_dev, pixels_in, subset_fields_in,
                 segments_in)
    outs = torch.ops.ngm355.target_sample_sv(rgbd, c2w, slot, active_field_ids, field_positions, num_fields_dev, iteration_dev,
                                             pixels_in, subset_fields_in, segments_in, [float(fx), float(fy), float(cx), float(cy)],
                                             float(radius), num_fields, num_points, T, R, capacity, int(seed),
                                             -1 if iteration is None else int(iteration), int(world_size), int(rank))
    return dict(zip(TARGET_SAMPLE_SV_OUT, outs))


def field_counts_add(field_ids, count, training_iterations, num_fields):
    """training_iterations[field_ids[i]] += 1 for i < count (device int32, or None: every row), skipping -1: one launch
    (ngm_field_counts_add), no synchronisation."""
    if field_ids.dtype != torch.int64 or training_iterations.dtype != torch.int64:
        raise TypeError("field_counts_add: field_ids and training_iterations must be int64")
    if count is not None:
        _check_device_count("field_counts_add", "count", count)
    if training_iterations.shape[0] < int(num_fields) or not training_iterations.is_contiguous() or not field_ids.is_contiguous():
        raise ValueError("field_counts_add: training_iterations must be a contiguous (>= num_fields,) tensor, field_ids contiguous")
    _require_gpu(field_ids, count, training_iterations)
    K.check(K.lib().ngm_field_counts_add(_ptr(field_ids), _ptr(count), int(field_ids.shape[0]), _ptr(training_iterations),
                                         int(num_fields), _stream()), "ngm_field_counts_add")


# ------------------------------------------------------------------------------------------------
# reserved field rows: a keyframe's growth as one launch (include/ngm_hip.h ngm_fields_append)
# ------------------------------------------------------------------------------------------------
@_op("fields_append", mutates_args=("params", "exp_avgs", "exp_avg_sqs", "lps", "positions", "orientations", "training_iterations",
                                    "num_fields_dev"))
def _fields_append_op(params: List[torch.Tensor], exp_avgs: List[torch.Tensor], exp_avg_sqs: List[torch.Tensor],
                      lps: List[torch.Tensor], lp_index: List[int], prototypes: List[torch.Tensor], new_positions: torch.Tensor,
                      new_orientations: torch.Tensor, positions: torch.Tensor, orientations: torch.Tensor,
                      training_iterations: Optional[torch.Tensor], num_fields_dev: torch.Tensor, first: int) -> None:
    n = len(params)
    arr = (K.AppendTensor * max(n, 1))()
    lp_of = dict(zip(lp_index, lps))
    for i, (p, m, v, proto) in enumerate(zip(params, exp_avgs, exp_avg_sqs, prototypes)):
        lp = lp_of.get(i)
        arr[i] = K.AppendTensor(C.cast(p.data_ptr(), K.f32p), C.cast(m.data_ptr(), K.f32p), C.cast(v.data_ptr(), K.f32p),
                                C.cast(proto.data_ptr(), K.f32p), p.stride(0), proto.numel(), _ptr(lp),
                                0 if lp is None else _TORCH_DT[lp.dtype], 0)
    a = K.FieldsAppendArgs(arr, n, int(first), int(new_positions.shape[0]), int(positions.shape[0]),
                           C.cast(new_positions.data_ptr(), K.f32p), C.cast(new_orientations.data_ptr(), K.f32p),
                           C.cast(positions.data_ptr(), K.f32p), C.cast(orientations.data_ptr(), K.f32p),
                           _ptr(training_iterations), num_fields_dev.data_ptr())
    K.check(K.lib().ngm_fields_append(C.byref(a), _stream()), "ngm_fields_append")


def fields_append(tensors, new_positions, new_orientations, positions, orientations, training_iterations, num_fields_dev, first):
    """Fill rows [first, first + num_new) of a map with reserved rows and raise its device field count: one launch on the
    current stream (torch.ops.ngm355.fields_append, ngm_fields_append), no host synchronisation.
    tensors: a list of dicts(param=, exp_avg=, exp_avg_sq= (max_fields, ...) float32, prototype= (...) float32, lp= the
    optional (max_fields, ...) bfloat16 / float16 copy); new_positions (num_new, 3), new_orientations (num_new, 4);
    positions (max_fields, 3), orientations (max_fields, 4), training_iterations (max_fields,) int64 or None,
    num_fields_dev a one-element int32 tensor.  Every tensor is a contiguous device tensor."""
    def need(cond, msg, exc=ValueError):
        if not cond:
            raise exc("fields_append: " + msg)
    _check_device_count("fields_append", "num_fields_dev", num_fields_dev)
    need(len(tensors) <= K.NGM_APPEND_MAX_TENSORS, f"at most {K.NGM_APPEND_MAX_TENSORS} tensors per call")
    for name, t, w in (("new_positions", new_positions, 3), ("new_orientations", new_orientations, 4), ("positions", positions, 3),
                       ("orientations", orientations, 4)):
        need(isinstance(t, torch.Tensor) and t.dtype == torch.float32, f"{name} must be a float32 tensor", TypeError)
        need(t.dim() == 2 and t.shape[1] == w and t.is_contiguous(), f"{name} must be a contiguous (n, {w}) tensor, got {tuple(t.shape)}")
    max_fields, num_new, first = positions.shape[0], new_positions.shape[0], int(first)
    need(orientations.shape[0] == max_fields, f"positions has {max_fields} rows, orientations {orientations.shape[0]}")
    need(new_orientations.shape[0] == num_new, f"{num_new} new positions but {new_orientations.shape[0]} new orientations")
    need(first >= 0 and first + num_new <= max_fields, f"rows [{first}, {first + num_new}) do not fit the capacity of {max_fields} fields")
    if training_iterations is not None:
        need(training_iterations.dtype == torch.int64, "training_iterations must be int64", TypeError)
        need(tuple(training_iterations.shape) == (max_fields,) and training_iterations.is_contiguous(),
             f"training_iterations must be a contiguous ({max_fields},) tensor, got {tuple(training_iterations.shape)}")
    params, ms, vs, lps, lp_index, protos = [], [], [], [], [], []
    for i, t in enumerate(tensors):
        p, proto, lp = t["param"], t["prototype"], t.get("lp")
        for name in ("param", "exp_avg", "exp_avg_sq"):
            x = t[name]
            need(x.dtype == torch.float32, f"tensor {i}: {name} must be float32, got {x.dtype}", TypeError)
            need(x.is_contiguous() and tuple(x.shape) == (max_fields,) + tuple(proto.shape),
                 f"tensor {i}: {name} must be a contiguous {(max_fields,) + tuple(proto.shape)} tensor (capacity mismatch), got {tuple(x.shape)}")
        need(proto.dtype == torch.float32 and proto.is_contiguous() and proto.numel() >= 1, f"tensor {i}: prototype must be contiguous float32")
        if lp is not None:
            need(lp.dtype in (torch.bfloat16, torch.float16), f"tensor {i}: the 16-bit copy must be bfloat16 or float16, got {lp.dtype}", TypeError)
            need(lp.is_contiguous() and lp.shape == p.shape, f"tensor {i}: the 16-bit copy must have the shape of param (capacity mismatch)")
            lps.append(lp)
            lp_index.append(i)
        params.append(p), ms.append(t["exp_avg"]), vs.append(t["exp_avg_sq"]), protos.append(proto)
    _require_gpu(*params, *ms, *vs, *lps, *protos, new_positions, new_orientations, positions, orientations, training_iterations,
                 num_fields_dev)
    if num_new == 0:
        return
    torch.ops.ngm355.fields_append(params, ms, vs, lps, lp_index, protos, new_positions, new_orientations, positions, orientations,
                                   training_iterations, num_fields_dev, first)


# ------------------------------------------------------------------------------------------------
# fields anchored to keyframes: the map re-posed in place after a pose-graph update (include/ngm_hip.h ngm_fields_repose)
# ------------------------------------------------------------------------------------------------
@_op("fields_repose_", mutates_args=("positions", "orientations", "prev_poses"))
def _fields_repose_op(positions: torch.Tensor, orientations: torch.Tensor, anchor_slot: torch.Tensor, prev_poses: torch.Tensor,
                      new_poses: torch.Tensor, num_fields_dev: Optional[torch.Tensor], num_fields: int, advance_prev: bool) -> None:
    a = K.FieldsReposeArgs(C.cast(positions.data_ptr(), K.f32p), C.cast(orientations.data_ptr(), K.f32p), anchor_slot.data_ptr(),
                           C.cast(prev_poses.data_ptr(), K.f32p), C.cast(new_poses.data_ptr(), K.f32p), _ptr(num_fields_dev),
                           int(num_fields), int(new_poses.shape[0]), int(bool(advance_prev)), 0)
    K.check(K.lib().ngm_fields_repose(C.byref(a), _stream()), "ngm_fields_repose")


def fields_repose_(positions, orientations, anchor_slot, prev_poses, new_poses, num_fields_dev=None, num_fields=None,
                   advance_prev=True):
    """Move every field with the keyframe it is anchored to, in place (torch.ops.ngm355.fields_repose_, ngm_fields_repose): on
    the current stream, no host synchronisation.  positions (n, 3), orientations (n, 4) float32; anchor_slot (n,) int32, row
    of the pose tables or -1; prev_poses / new_poses (num_poses, 4, 4) float32.  The first num_fields rows are processed (all
    n by default), or clamp(num_fields_dev, 0, num_fields) with the one-element int32 device tensor.  advance_prev: prev_poses
    := new_poses afterwards.  Fields whose anchor did not move (bitwise), is -1 / out of range, or has a non-finite pose are
    not touched."""
    def need(cond, msg, exc=ValueError):
        if not cond:
            raise exc("fields_repose_: " + msg)
    for name, t, tail in (("positions", positions, (3,)), ("orientations", orientations, (4,)), ("prev_poses", prev_poses, (4, 4)),
                          ("new_poses", new_poses, (4, 4))):
        need(isinstance(t, torch.Tensor) and t.dtype == torch.float32, f"{name} must be a float32 tensor", TypeError)
        need(t.dim() == 1 + len(tail) and tuple(t.shape[1:]) == tail and t.is_contiguous(),
             f"{name} must be a contiguous (n, {', '.join(map(str, tail))}) tensor, got {tuple(t.shape)}")
    need(isinstance(anchor_slot, torch.Tensor) and anchor_slot.dtype == torch.int32, "anchor_slot must be an int32 tensor", TypeError)
    n = positions.shape[0]
    need(orientations.shape[0] == n and tuple(anchor_slot.shape) == (n,) and anchor_slot.is_contiguous(),
         f"positions has {n} rows, orientations {orientations.shape[0]}, anchor_slot {tuple(anchor_slot.shape)}")
    need(prev_poses.shape == new_poses.shape, f"prev_poses {tuple(prev_poses.shape)} and new_poses {tuple(new_poses.shape)} differ")
    num_fields = n if num_fields is None else int(num_fields)
    need(0 <= num_fields <= n, f"num_fields {num_fields} outside [0, {n}]")
    if num_fields_dev is not None:
        _check_device_count("fields_repose_", "num_fields_dev", num_fields_dev)
    _require_gpu(positions, orientations, anchor_slot, prev_poses, new_poses, num_fields_dev)
    torch.ops.ngm355.fields_repose_(positions, orientations, anchor_slot, prev_poses, new_poses, num_fields_dev, num_fields,
                                    bool(advance_prev))


# ------------------------------------------------------------------------------------------------
# covering a keyframe's depth with new fields (include/ngm_hip.h ngm_cover_depth)
# ------------------------------------------------------------------------------------------------
def cover_cell(radius: float) -> float:
    """The grid's edge 2 r / sqrt 3 (rm.py:299: the cube inscribed in a field's sphere), formed in double and rounded to
    float32 once -- what torch makes of the reference's Python scalar when it meets a float32 tensor."""
    import math
    return float(torch.tensor(2.0 * float(radius) / math.sqrt(3.0), dtype=torch.float64).to(torch.float32))


@_op("cover_depth")
def _cover_depth_op(depth: torch.Tensor, c2w: torch.Tensor, shift: torch.Tensor, field_positions: Optional[torch.Tensor],
                    field_ids: Optional[torch.Tensor], num_active: int, intrinsics: List[float], radius: float, cell: float,
                    max_new: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """depth: an (H, W) float32 view whose rows are dense (stride(0) == W stride(1)); intrinsics = fx, fy, cx, cy"""
    L = K.lib()
    h, w = int(depth.shape[0]), int(depth.shape[1])
    wsb = L.ngm_cover_depth_workspace(h, w, int(num_active), int(max_new))
    if wsb < 0:
        raise K.NgmError(f"cover_depth: {h} x {w} pixels, {num_active} active fields, max_new {max_new} refused "
                         f"(height * width < 2^31, 1 <= max_new <= {K.NGM_COVER_MAX_NEW})", code=int(wsb))
    ws = torch.empty(wsb, device=depth.device, dtype=torch.uint8)
    new_positions = torch.zeros(max_new, 3, device=depth.device, dtype=torch.float32)
    counts = torch.zeros(4, device=depth.device, dtype=torch.int32)
    fx, fy, cx, cy = intrinsics
    a = K.CoverDepthArgs(depth.data_ptr(), c2w.data_ptr(), shift.data_ptr(), _ptr(field_positions), _ptr(field_ids),
                         new_positions.data_ptr(), counts.data_ptr(), int(depth.stride(1)),
                         0 if field_positions is None else int(field_positions.shape[0]), int(num_active), h, w, int(max_new),
                         fx, fy, cx, cy, radius, cell)
    K.check(L.ngm_cover_depth(C.byref(a), ws.data_ptr(), wsb, _stream()), "ngm_cover_depth")
    return new_positions, counts


@_cover_depth_op.register_fake
def _(depth, c2w, shift, field_positions, field_ids, num_active, intrinsics, radius, cell, max_new):
    return depth.new_empty(max_new, 3, dtype=torch.float32), depth.new_empty(4, dtype=torch.int32)


COVER_STATUS = {0: "ok", 1: "more than max_new new cells", 2: "a cell index outside (-2^20, 2^20)"}


def cover_depth(depth_or_rgbd, c2w, shift, field_positions, radius, fx, fy, cx, cy, max_new, field_ids=None, num_active=None,
                cell=None):
    """Where new fields go so that a keyframe's depth is covered (torch.ops.ngm355.cover_depth, ngm_cover_depth;
    NeuralGraphMap._extend_global_map_dict, rm.py:265-345): on the current stream, no host synchronisation.
    depth_or_rgbd: (H, W) float32 depth or (H, W, 4) float32 r g b depth (read in place, no copy); c2w (4, 4) and shift (3)
    float32 DEVICE tensors; field_positions (rows, 3) float32 or None; the active fields are its first num_active rows
    (default: all), or with field_ids (int64, device) the rows it names, entries < 0 or >= rows skipped.  cell: the grid's
    edge, default cover_cell(radius).
    Returns new_positions (max_new, 3) float32 and counts (4,) int32 = num_new, status, uncovered valid pixels, valid pixels:
    status 0 = rows [0, num_new) hold the centres of the new cells in ascending (i, j, k) order (the other rows are zero);
    1 = more than max_new (num_new = the number needed, no row written); 2 = a cell index outside (-2^20, 2^20)."""
    def need(cond, msg, exc=ValueError):
        if not cond:
            raise exc("cover_depth: " + msg)
    _require_gpu(depth_or_rgbd, c2w, shift, field_positions, field_ids)
    img = depth_or_rgbd
    need(isinstance(img, torch.Tensor) and img.dtype == torch.float32, "the image must be a float32 tensor", TypeError)
    need(img.dim() == 2 or (img.dim() == 3 and img.shape[2] == 4), f"the image must be (H, W) or (H, W, 4), got {tuple(img.shape)}")
    depth = img if img.dim() == 2 else img[..., 3]
    h, w = depth.shape
    need(h >= 1 and w >= 1, "the image has no pixels")
    if not (depth.stride(1) >= 1 and depth.stride(0) == w * depth.stride(1)):      # rows must follow each other densely
        depth = depth.contiguous()
    for name, t, shape in (("c2w", c2w, (4, 4)), ("shift", shift, (3,))):
        need(isinstance(t, torch.Tensor) and t.dtype == torch.float32, f"{name} must be a float32 device tensor", TypeError)
        need(tuple(t.shape) == shape and t.is_contiguous(), f"{name} must be a contiguous {shape} tensor, got {tuple(t.shape)}")
    rows = 0
    if field_positions is not None:
        need(field_positions.dtype == torch.float32, "field_positions must be float32", TypeError)
        need(field_positions.dim() == 2 and field_positions.shape[1] == 3 and field_positions.is_contiguous(),
             f"field_positions must be a contiguous (rows, 3) tensor, got {tuple(field_positions.shape)}")
        rows = field_positions.shape[0]
    if field_ids is not None:
        need(field_ids.dtype == torch.int64, "field_ids must be int64", TypeError)
        need(field_ids.dim() == 1 and field_ids.is_contiguous(), "field_ids must be a contiguous 1-D tensor")
        need(num_active is None or num_active == field_ids.shape[0], "num_active and field_ids disagree")
        num_active = field_ids.shape[0]
        if rows == 0:
            field_ids, num_active = None, 0
    elif num_active is None:
        num_active = rows
    num_active = int(num_active)
    need(0 <= num_active and (field_ids is not None or num_active <= rows), f"num_active {num_active} outside [0, {rows}]")
    if num_active == 0:
        field_ids = None
    need(0 < float(radius) < float("inf"), "radius must be finite and > 0")
    cell = cover_cell(radius) if cell is None else float(cell)              # from the double, as the reference forms it
    radius = float(radius)
    need(cell > 0 and cell != float("inf"), "cell must be finite and > 0")
    need(isinstance(max_new, int) and max_new >= 1, f"max_new must be an integer >= 1, got {max_new!r}")
    return torch.ops.ngm355.cover_depth(depth, c2w, shift, field_positions, field_ids, num_active,
                                        [float(fx), float(fy), float(cx), float(cy)], radius, cell, max_new)
