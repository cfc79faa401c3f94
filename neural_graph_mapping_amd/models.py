"""Drop-in counterparts of the reference's field model classes, backed by the gfx950 kernels.

Mirrors ``neural_graph_mapping/models.py`` (NeuralField :66-182, NeuralFieldSet :185-411) and
``positional_encodings.py`` (:164-276): same constructor kwargs, same parameter names
("_encoding._linear.weight", "_linears.{i}.weight/bias", "_neus_sd"), same stacked
``all_fields_params`` / ``vmap_fields_params`` dictionaries, same forward signature.  The arithmetic
is NOT torch.vmap over nn.Modules: ``forward`` launches the hand-written HIP kernels through
``ops`` (no CPU fallback).
"""
import math
from pydoc import locate
from typing import Dict, Literal, Optional

import torch

from . import _capi as K
from . import ops

_ALIASES = {"neural_graph_mapping.": "neural_graph_mapping_amd."}


def str_to_object(name):
    """Resolve a class given by (reference or local) dotted name (utils.py:114-138 semantics)."""
    if not isinstance(name, str):
        return name
    for old, new in _ALIASES.items():
        if name.startswith(old):
            name = new + name[len(old):]
    obj = globals().get(name.rsplit(".", 1)[-1]) if name.startswith("neural_graph_mapping_amd.") else None
    return obj or locate(name)


# ------------------------------------------------------------------------------------------------
# encodings (descriptors + parameters; evaluated inside the fused kernels)
# ------------------------------------------------------------------------------------------------
class PositionalEncoding(torch.nn.Module):
    def get_out_dim(self) -> int:
        raise NotImplementedError()

    def spec(self) -> dict:
        raise NotImplementedError()

    def forward(self, points):
        raise NotImplementedError("encodings are evaluated inside the fused field kernels; call the "
                                  "owning NeuralField / NeuralFieldSet")


class PositionalEncodingFourier(PositionalEncoding):
    """cat(x, sin(W x)) with learnable W (positional_encodings.py:164-216)."""

    def __init__(self, dim_in: int, dim_out: int, mu: float, sigma: float, raw_coords: bool) -> None:
        super().__init__()
        if dim_in not in (2, 3):
            raise NotImplementedError("only 2D and 3D fields are supported")
        self._dim_in = dim_in
        self._linear = torch.nn.Linear(dim_in, dim_out - dim_in if raw_coords else dim_out, False)
        self._dim_out = dim_out
        self._raw_coords = raw_coords
        torch.nn.init.normal_(self._linear.weight, mu, sigma)

    def get_out_dim(self) -> int:
        return self._dim_out

    def spec(self):
        # a 2-D encoding is evaluated as the 3-D one with a zero third matrix column (and, raw_coords, one more raw feature
        # whose layer-0 weights are zero): Embed2D below
        extra = 1 if (self._dim_in == 2 and self._raw_coords) else 0
        return dict(encoding="fourier", dim_enc=self._dim_out + extra, raw_coords=self._raw_coords)


class PositionalEncodingNeRF(PositionalEncoding):
    """sin / cos(2^i pi x) octaves, sines first (positional_encodings.py:219-276)."""

    def __init__(self, dim_in: int, num_octaves: int = 8, start_octave: int = 0) -> None:
        super().__init__()
        if dim_in not in (2, 3):
            raise NotImplementedError("only 2D and 3D fields are supported")
        self.num_octaves, self.start_octave, self.dim_in = num_octaves, start_octave, dim_in

    def get_out_dim(self) -> int:
        return self.dim_in * self.num_octaves * 2

    def spec(self):
        return dict(encoding="nerf", num_octaves=self.num_octaves, start_octave=self.start_octave)


class PermutohedralEncoding(PositionalEncoding):
    """Multi-resolution permutohedral-lattice hash encoding (positional_encodings.py:19-66).

    Same constructor kwargs as the reference wrapper (including its ``appply_random_shift_per_level``
    spelling).  The reference delegates the arithmetic to the un-vendored CUDA package
    ``permutohedral_encoding`` -> PARITY UNPINNED; the HIP kernels implement the published
    lattice algorithm as restated in oracle/ngm_oracle.py:encode_permuto.  Parameters: the hash table
    ``lattice_values`` (nr_levels, 2**log2_hashmap_size, nr_feat_per_level) ~ N(0, init_scale) and the
    constant per-level shifts ``random_shift_per_level`` (nr_levels, 3) ~ 10 N(0,1)."""

    def __init__(self, pos_dim, log2_hashmap_size, nr_levels, nr_feat_per_level, coarsest_scale, finest_scale,
                 appply_random_shift_per_level=True, concat_points=False, concat_points_scaling=1.0,
                 init_scale=1e-5) -> None:
        super().__init__()
        if pos_dim != 3 or nr_feat_per_level != 2 or nr_levels > 16 or concat_points:
            raise NotImplementedError("permutohedral encoding: pos_dim 3, 2 features/level, <= 16 levels, no concat_points")
        self.kw = dict(log2_hashmap_size=log2_hashmap_size, nr_levels=nr_levels, nr_feat_per_level=nr_feat_per_level,
                       coarsest_scale=float(coarsest_scale), finest_scale=float(finest_scale))
        capacity = 2 ** log2_hashmap_size
        lattice = torch.randn(capacity, nr_levels, nr_feat_per_level) * init_scale
        self.lattice_values = torch.nn.Parameter(lattice.permute(1, 0, 2).contiguous())
        shift = 10.0 * torch.randn(nr_levels, 3) if appply_random_shift_per_level else torch.zeros(nr_levels, 3)
        self.random_shift_per_level = torch.nn.Parameter(shift, requires_grad=False)
        self._out = nr_levels * nr_feat_per_level

    def get_out_dim(self) -> int:
        return self._out

    def spec(self):
        return dict(encoding="permuto", **self.kw)


class TriplaneEncoding(PositionalEncoding):
    """Learned triplane encoding (positional_encodings.py:69-161): three (C, res, res) feature planes, bilinear lookup of
    the (x,y), (x,z), (y,z) projections (grid_sample, align_corners=True, border padding; points expected in [-1,1]),
    summed / multiplied / concatenated.  Same constructor kwargs and parameter name (`plane_coef`) as the reference."""

    def __init__(self, resolution: int = 32, num_components: int = 64, init_scale: float = 0.1,
                 mode: Literal["sum", "product", "concat"] = "sum") -> None:
        super().__init__()
        if mode not in K.TRI:
            raise ValueError(f"{mode=} is not supported.")
        self.resolution, self.num_components, self.init_scale, self.mode = resolution, num_components, init_scale, mode
        self.plane_coef = torch.nn.Parameter(init_scale * torch.randn((3, num_components, resolution, resolution)))

    def get_out_dim(self) -> int:
        return self.num_components * (3 if self.mode == "concat" else 1)

    def spec(self):
        return dict(encoding="triplane", resolution=self.resolution, num_components=self.num_components, tri_mode=self.mode)


# ------------------------------------------------------------------------------------------------
class NeuralField(torch.nn.Module):
    """Positional encoding + MLP prototype (models.py:66-182); holds ONE field's parameters."""

    def __init__(self, encoding_type, encoding_kwargs: dict, num_layers: int, dim_out: int,
                 dim_mlp_out: Optional[int] = None, skip_mode: Literal["no", "add", "concat", "rezero"] = "no",
                 initial_geometry_bias: float = 0.0, neus_initial_sd: Optional[float] = None) -> None:
        super().__init__()
        if skip_mode not in K.SKIP:
            raise NotImplementedError(f"skip_mode={skip_mode!r}: 'no', 'add' and 'concat' have kernels (the reference's own "
                                      "constructor raises for 'rezero', models.py:131-132)")
        self._encoding = str_to_object(encoding_type)(**encoding_kwargs)
        self._dim_encoding = self._encoding.get_out_dim()
        self._dim_out = dim_out
        self._dim_mlp_out = dim_mlp_out if dim_mlp_out is not None else self._dim_encoding
        self._num_layers = num_layers
        self._skip_mode = skip_mode
        if neus_initial_sd is not None:
            self._neus_sd = torch.nn.Parameter(torch.tensor(float(neus_initial_sd)))
        dim_mlp_in = self._dim_mlp_out + (self._dim_encoding if skip_mode == "concat" else 0)      # models.py:105-110
        dims_in = [self._dim_encoding] + [dim_mlp_in] * num_layers
        dims_out = [self._dim_mlp_out] * num_layers + [dim_out]
        self._linears = torch.nn.ModuleList(torch.nn.Linear(i, o) for i, o in zip(dims_in, dims_out))
        with torch.no_grad():
            self._linears[-1].bias[-1] += initial_geometry_bias

    def field_cfg(self, scale_mode="no", field_radius=1.0) -> K.FieldCfg:
        return K.field_cfg(num_layers=self._num_layers, dim_hidden=self._dim_mlp_out, dim_out=self._dim_out,
                           scale_mode=scale_mode, field_radius=field_radius or 1.0, skip_mode=self._skip_mode,
                           **self._encoding.spec())

    def numel(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def forward(self, query_points: torch.Tensor) -> torch.Tensor:
        """Single field, points already in the field frame: (...,3) -> (...,dim_out)  ((...,2) with a 2-D encoding)."""
        fc = self.field_cfg()
        lead = query_points.shape[:-1]
        params = {k: v.unsqueeze(0) for k, v in self.state_dict(keep_vars=True).items() if k != "_neus_sd"}
        if query_points.shape[-1] == 2:
            e2 = Embed2D(self)
            params, query_points = e2.params(params), e2.points(query_points)
        return ops.field_eval(fc, params, query_points.reshape(1, -1, 3)).view(*lead, self._dim_out)


# ------------------------------------------------------------------------------------------------
class Embed2D:
    """`dim_points == 2` (models.py:236-238: complex numbers as orientations, `complex_apply` :48-62) on the 3-D kernels.

    A planar field set IS a 3-D one restricted to z = 0: points and centres get a zero third coordinate (distances, the
    kNN ranking and the inside test are unchanged: + 0^2 is exact), the orientation c = a + ib becomes the quaternion
    (q_w, 0, 0, q_z) with (q_w + i q_z)^2 = c -- pytorch3d's un-normalised `quaternion_apply(quaternion_invert(q), v)`, which
    is what the kernels compute (ngm_device.h: quat_rotate_inv), then maps (x, y, 0) to (a x + b y, a y - b x, 0) =
    conj(c) (x + iy), the reference's `complex_apply(complex_invert(c), .)`, for any modulus -- and every place where the
    encoding of the third coordinate would enter the network carries a ZERO weight: the third column of the Fourier matrix,
    and the layer-0 columns of the raw z feature (Fourier, `raw_coords`) or of the z octaves (NeRF).  A zero weight times
    a finite feature is exactly 0 on every matmul path (fp32 MFMA and the bf16 split alike), so the result differs from
    the reference's 2-D arithmetic only by the rounding of the rotation (fixture G22, from the real reference).  The zero
    blocks are inserted with differentiable torch ops, so gradients arrive at the 2-D parameters; the blocks' own
    gradients are dropped."""

    def __init__(self, proto: "NeuralField") -> None:
        enc = proto._encoding
        if proto._skip_mode != "no":
            raise NotImplementedError("dim_points=2: skip connections are not built for planar field sets (the encoding "
                                      "width of the embedded 3-D problem differs from the 2-D one)")
        d2 = enc.get_out_dim()
        if isinstance(enc, PositionalEncodingFourier) and enc._dim_in == 2:
            cols = [0, 1, -1] + list(range(2, d2)) if enc._raw_coords else list(range(d2))
        elif isinstance(enc, PositionalEncodingNeRF) and enc.dim_in == 2:
            n = enc.num_octaves                       # sines (x octaves, y octaves), cosines likewise (positional_encodings.py:268-274)
            cols = list(range(0, 2 * n)) + [-1] * n + list(range(2 * n, 4 * n)) + [-1] * n
        else:
            raise NotImplementedError("dim_points=2 needs a 2-D Fourier or NeRF-octave encoding (dim_in=2); the permutohedral "
                                      "and triplane encodings are 3-D constructions")
        self._d2 = d2
        self._cols = [c if c >= 0 else d2 for c in cols]          # d2 = the appended zero column

    def params(self, params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        out = dict(params)
        w0 = params["_linears.0.weight"]
        idx = torch.as_tensor(self._cols, device=w0.device)
        out["_linears.0.weight"] = torch.cat((w0, w0.new_zeros(*w0.shape[:-1], 1)), -1).index_select(-1, idx)
        k = "_encoding._linear.weight"
        if k in params:
            out[k] = torch.cat((params[k], params[k].new_zeros(*params[k].shape[:-1], 1)), -1)
        return out

    @staticmethod
    def points(p: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        return None if p is None else torch.cat((p, p.new_zeros(*p.shape[:-1], 1)), -1)

    @staticmethod
    def orientations(c: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        """principal complex square root, in fp64: q_w = sqrt((|c| + a) / 2), q_z = sign(b) sqrt((|c| - a) / 2)"""
        if c is None:
            return None
        a, b = c[..., 0].double(), c[..., 1].double()
        r = torch.sqrt(a * a + b * b)
        qw = torch.sqrt(torch.clamp((r + a) * 0.5, min=0.0))
        qz = torch.where(b < 0, -1.0, 1.0) * torch.sqrt(torch.clamp((r - a) * 0.5, min=0.0))
        z = torch.zeros_like(qw)
        return torch.stack((qw, z, z, qz), -1).to(c.dtype)


class NeuralFieldSet(torch.nn.Module):
    """Set of posed neural fields (models.py:185-411) evaluated by the HIP kernels."""

    def __init__(self, dim_points: int, field_type, field_kwargs: dict, num_knn: int, distance_factor: float,
                 outside_value: float, field_radius: Optional[float] = None,
                 scale_mode: Literal["no", "unit_ball", "unit_cube"] = "no",
                 weight_dtype: Optional[str] = None) -> None:
        """`weight_dtype` (not in the reference, which is fp32 only): "bfloat16" / "float16" keep a reduced-precision COPY
        of every field's weights (`lp_fields_params`) that the evaluation and training kernels read (half the bytes
        staged / gathered per field; arithmetic stays fp32).  `all_fields_params` remains the fp32 master set: what
        Adam updates, what checkpoints hold, what the differentiable ops take.  The fused training step refreshes the
        copy inside its Adam kernels; after editing the masters by hand call `refresh_lp()`."""
        super().__init__()
        if weight_dtype not in (None, "float32", "bfloat16", "float16"):
            raise ValueError(f"{weight_dtype=}: float32, bfloat16 or float16")
        self._weight_dtype = None if weight_dtype in (None, "float32") else getattr(torch, weight_dtype)
        self.lp_fields_params: Optional[Dict[str, torch.Tensor]] = None
        if scale_mode != "no" and field_radius is None:
            raise ValueError(f"{scale_mode=} requires field_radius to be specified.")
        if dim_points not in (2, 3):
            raise NotImplementedError("Only 2D and 3D spaces are supported.")      # models.py:236-243
        if scale_mode not in K.SCALE:
            raise NotImplementedError(f"{scale_mode=} is not available.")
        if not 1 <= int(num_knn) <= 16:
            # the reference takes any num_knn (models.py:354-366: knn_points + a softmax over K); the assignment kernel keeps the K
            # best in registers: unrolled instances for K = 1..8, one 16-slot instance for K = 9..16 (include/ngm_hip.h,
            # ngm_field_eval_knn; the one-call image path blends up to 8 and hands K > 8 to the staged entry points) -- fail here,
            # not at the first render
            raise NotImplementedError(f"num_knn={num_knn}: the kNN evaluation kernels are compiled for 1 <= K <= 16")
        self._scale_mode, self._field_radius, self._dim_points = scale_mode, field_radius, dim_points
        self._num_knn, self._distance_factor, self._outside_value = num_knn, distance_factor, outside_value
        self._prototype_field = str_to_object(field_type)(**field_kwargs)
        # planar sets run on the 3-D kernels (Embed2D); the render / training path (rays) is 3-D only, as in the reference
        self._embed2d = Embed2D(self._prototype_field) if dim_points == 2 else None
        if self._embed2d is not None and self._weight_dtype is not None:
            raise NotImplementedError("weight_dtype (16-bit weight storage) is not built for dim_points=2")
        if self._weight_dtype is not None and isinstance(getattr(self._prototype_field, "_encoding", None), TriplaneEncoding):
            # the plane gradient is a fixed-point scatter into fp32 planes and their Adam launch has no 16-bit copy to
            # refresh: fail here, not at the first kernel call
            raise NotImplementedError("weight_dtype (16-bit weight storage) is not built for the triplane encoding")
        self.all_fields_params: Optional[Dict[str, torch.Tensor]] = None
        self.vmap_fields_params: Optional[Dict[str, torch.Tensor]] = None
        # reserve_fields: dict(max=, num=, params={name: (max, ...)}, lp={name: (max, ...) 16-bit} or None); None = not reserved
        self._reserved: Optional[dict] = None

    # -- parameter store -----------------------------------------------------------------------
    def field_cfg(self, field_radius=None) -> K.FieldCfg:
        r = self._field_radius if field_radius is None else field_radius
        return self._prototype_field.field_cfg(self._scale_mode, r)

    def _lp_names(self):
        """the parameters that have a 16-bit copy of their own (the others' "copy" is the master tensor itself)"""
        return [k for k in self._prototype_field.state_dict() if not (k in K.NO_GRAD_PARAMS or k == "_neus_sd")]

    def reserve_fields(self, max_fields: int) -> None:
        """Allocate every stacked parameter (and its 16-bit copy, with `weight_dtype`) ONCE for max_fields rows; the fields
        the set holds are copied over.  From here on all_fields_params / lp_fields_params are leading-row views of that
        storage (their shapes stay (num, ...), their data never moves) and add_fields appends in place -- up to max_fields,
        beyond which it raises ValueError and changes nothing.  Not in the reference (whose _add_fields concatenates); what
        it buys is that device code holding the addresses (a captured training graph) survives the growth."""
        max_fields = int(max_fields)
        old = self.all_fields_params
        num = 0 if old is None else next(iter(old.values())).shape[0]
        if max_fields < max(num, 1):
            raise ValueError(f"reserve_fields({max_fields}): the set already holds {num} fields (and needs room for one)")
        proto = self._prototype_field.state_dict()
        params = {k: torch.zeros((max_fields,) + tuple(v.shape), dtype=v.dtype, device=v.device if old is None else old[k].device)
                  for k, v in proto.items()}
        if old is not None:
            for k, v in old.items():
                params[k][:num] = v.detach()
        lp = None
        if self._weight_dtype is not None:
            lp = {k: torch.zeros_like(params[k], dtype=self._weight_dtype) for k in self._lp_names()}
        self._reserved = dict(max=max_fields, num=num, params=params, lp=lp)
        self._set_num(num)
        self.refresh_lp()

    def _set_num(self, num: int) -> None:
        """reserved mode: the public dictionaries as views of the first `num` rows"""
        rs = self._reserved
        rs["num"] = num
        self.all_fields_params = {k: v[:num] for k, v in rs["params"].items()}
        if rs["lp"] is not None:
            self.lp_fields_params = {k: (rs["lp"][k][:num] if k in rs["lp"] else v) for k, v in self.all_fields_params.items()}

    def _check_room(self, num_new: int) -> int:
        rs = self._reserved
        if num_new < 0 or rs["num"] + num_new > rs["max"]:
            raise ValueError(f"add_fields({num_new}): {rs['num']} of the {rs['max']} reserved field rows are in use; reserve more "
                             "(reserve_fields reallocates: anything that holds the old addresses must be rebuilt)")
        return rs["num"]

    def add_fields(self, num_fields: int) -> None:
        """Append clones of the prototype's state (models.py:245-264).  After reserve_fields: in place, into the next
        reserved rows (plain slice assignment, on any device; NeuralGraphRenderer.add_fields does the same on the GPU in
        one launch together with the optimiser state and the poses)."""
        if self._reserved is not None:
            first = self._check_room(num_fields)
            rs = self._reserved
            for k, v in self._prototype_field.state_dict().items():
                rs["params"][k][first:first + num_fields] = v.detach().to(rs["params"][k].device)
                if rs["lp"] is not None and k in rs["lp"]:
                    rs["lp"][k][first:first + num_fields] = rs["params"][k][first:first + num_fields]     # copy_: round to nearest even
            self._set_num(first + num_fields)
            return
        new = {k: v.detach().unsqueeze(0).repeat(num_fields, *([1] * v.dim())).clone()
               for k, v in self._prototype_field.state_dict().items()}
        if self.all_fields_params is None:
            self.all_fields_params = new
        else:
            self.all_fields_params = {k: torch.cat((v, new[k])) for k, v in self.all_fields_params.items()}
        self.refresh_lp()

    def refresh_lp(self) -> None:
        """(re)build the reduced-precision copy from the fp32 masters (no-op without `weight_dtype`)"""
        if self._weight_dtype is None or self.all_fields_params is None:
            self.lp_fields_params = None
            return
        if self._reserved is not None:                     # in place: the copy's storage is part of the reservation
            for k, dst in self._reserved["lp"].items():
                dst[:self._reserved["num"]].copy_(self.all_fields_params[k])
            self._set_num(self._reserved["num"])
            return
        self.lp_fields_params = {k: (v if (k in K.NO_GRAD_PARAMS or k == "_neus_sd") else v.to(self._weight_dtype))
                                 for k, v in self.all_fields_params.items()}

    def kernel_params(self) -> Dict[str, torch.Tensor]:
        """what the evaluation / training kernels read: the reduced-precision copy when there is one, else the masters"""
        src = self.lp_fields_params if self.lp_fields_params is not None else self.all_fields_params
        return {k: v for k, v in src.items() if k != "_neus_sd"}

    def set_vmap_fields(self, field_ids: Optional[torch.Tensor]) -> None:
        if field_ids is None:
            self.vmap_fields_params = self.all_fields_params
        else:
            self.vmap_fields_params = {k: v[field_ids] for k, v in self.all_fields_params.items()}

    def _apply(self, fn, *a, **kw):
        super()._apply(fn, *a, **kw)
        if self._reserved is not None:                     # the whole reservation moves (a new storage: re-capture what held it)
            rs = self._reserved
            rs["params"] = {k: fn(v) for k, v in rs["params"].items()}
            if rs["lp"] is not None:
                rs["lp"] = {k: torch.zeros_like(rs["params"][k], dtype=self._weight_dtype) for k in rs["lp"]}
            self._set_num(rs["num"])
            self.refresh_lp()
            return self
        if self.all_fields_params is not None:
            self.all_fields_params = {k: fn(v) for k, v in self.all_fields_params.items()}
            self.refresh_lp()
        return self

    def numel(self) -> int:
        # reference quirk kept: multiplies by the number of parameter NAMES (models.py:407-411)
        return self._prototype_field.numel() * len(self.all_fields_params)

    # -- evaluation ----------------------------------------------------------------------------
    def forward(self, query_points, field_positions=None, field_orientations=None, field_ids=None,
                use_vmap: bool = True, field_radius: Optional[float] = None) -> torch.Tensor:
        """models.py:287-405.  The `field_radius` ARGUMENT only widens / narrows the inside test of the kNN branch
        (`knn_dists[:, 0] < field_radius`, models.py:333-334, 368); the local coordinates are always scaled with the
        radius the set was constructed with (`_scale_local_points`, models.py:278-285), and the vmap branch never reads
        the argument at all (models.py:336-345).  Caller that relies on it: the colour pass of `_extract_mesh`,
        run_mapping.py:2320-2332 (`field_radius=self._field_radius + 0.1`)."""
        fc = self.field_cfg()                       # scaling: the set's own radius, whatever the argument says
        e2 = self._embed2d
        if e2 is not None:
            query_points, field_positions = e2.points(query_points), e2.points(field_positions)
            field_orientations = e2.orientations(field_orientations)
        if use_vmap:
            params = {k: v for k, v in self.vmap_fields_params.items() if k != "_neus_sd"}
            if e2 is not None:
                params = e2.params(params)
            return ops.field_eval(fc, params, query_points, field_positions, field_orientations)
        if field_radius is None:
            field_radius = self._field_radius
        if field_radius is None:
            # the reference compares `knn_dists[:, 0] < None` here (models.py:368) and raises a TypeError
            raise TypeError("forward(use_vmap=False) needs a field radius (constructor or argument): the reference's "
                            "inside test `knn_dists[:, 0] < field_radius` fails on None (models.py:368)")
        lead = query_points.shape[:-1]
        params = self.kernel_params() if e2 is None else e2.params(self.kernel_params())
        out = ops.field_eval_knn(fc, params, query_points.reshape(-1, 3), field_positions, field_orientations,
                                 self._num_knn, self._distance_factor, self._outside_value, field_ids,
                                 mask_radius=float(field_radius))
        return out.reshape(*lead, -1)
