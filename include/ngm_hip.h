/*
 * ngm_hip.h -- C ABI of the MI355X-native (gfx950) render/train hot path of Neural Graph Mapping.
 *
 * The reference (KTH-RPL/neural_graph_mapping) is pure Python and has no FFI; its boundary is a
 * Python method contract.  Each entry point below replaces the reference interface cited next to
 * it (paths relative to /root/reference/src/neural_graph_mapping, rm.py = run_mapping.py).  The
 * reference-side binding (a ctypes stub a maintainer would add) is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, opaque device pointers + explicit sizes; no torch types, no allocation inside:
 *    the caller owns and pre-allocates every output and the workspace;
 *  - all floating point tensors are contiguous row-major fp32, indices int64 (as the reference);
 *  - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *  - return value: 0 = ok, negative = NGM_E_* (ngm_last_error() holds a message); never throws.
 *  - F = active fields in the batch, R = rays per field, S = S_c + S_g samples per ray,
 *    P = points per field, D = encoding width, H = hidden width, L = hidden layers.
 */
#ifndef NGM_HIP_H
#define NGM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGM_ABI_VERSION 11 /* 11 (+ addition, number unchanged: ngm_fields_repose / struct ngm_fields_repose_args, the map re-posed in place after a pose-graph update; nothing existing changed); 11 (+ addition, number unchanged: ngm_target_sample_mv_live(_workspace) / struct ngm_target_live, ngm_target_observed_fields(_workspace) / struct ngm_observed_fields, ngm_field_counts_add: the sampler with its counts in device memory, the observed-field test and the per-field iteration counts on the device; nothing existing changed); 11 (+ addition, number unchanged: ngm_render_fwd_counted / ngm_render_bwd_counted / ngm_render_bwd_adam_counted, the training step launched at a capacity with the number of active rows in device memory; nothing existing changed); 11 (+ addition, number unchanged: ngm_target_sample_mv_workspace / ngm_target_sample_mv and struct ngm_target_sample, the device-side training-target sampler; nothing existing changed); 11: ngm_field_eval_stash_bytes / ngm_field_eval_fwd_train / ngm_field_eval_bwd_stash (training forward of the point evaluation writes the activation stash, its backward is the fused step's kernel); 10: ngm_field_cfg.activation_stash / .hash_grad_atomics (per configuration, no process-wide switch), empty loss selections report NaN like the reference; 9: ngm_sample_rays_weighted; 8: ngm_peer_set_timeout (a time-out now also poisons the sums with NaN); 7: ngm_encode_bwd; 6: ngm_render_eval_knn; 5: ngm_encode_fwd, ngm_render_bwd_seeded_vars, *_nll loss modes (+ loss-sum slot 10), peer status bits; 11 (+ addition, number unchanged: ngm_grid_eval_knn(_workspace), the kNN evaluation on a lattice given by its axes -- one block of the mesh grid as one call; nothing existing changed) */
/* Array bound of the per-layer pointers below (hidden layers; +1 output layer).  NOT the depth every entry point takes -- the
 * kernels are compiled per depth L = num_layers and padded width class (dim_enc and dim_hidden both <= 32, or both 33..64):
 *   L = 1, 2   every entry point, both width classes (forward, backward, fused step, kNN evaluation)
 *   L = 3      forward only and 33..64-wide only: ngm_field_eval_fwd, ngm_render_fwd (no targets' backward), ngm_field_eval_knn,
 *              ngm_render_eval_knn, ngm_grid_eval_knn; always exact-fp32 MFMA (NGM_MATMUL_AUTO resolves to it, an explicit NGM_MATMUL_BF16X3 is
 *              refused by the fused forward).  Every backward entry point (ngm_field_eval_bwd, ngm_render_bwd*, the *_adam and
 *              *_seeded forms) returns NGM_E_UNSUPPORTED before its first launch: workspace, gradients, parameters, Adam state
 *              and the device-side iteration counter are left as they were.
 *   L = 3 at <= 32 units, L = 4   nothing: refused by the configuration check of every entry point (NGM_E_UNSUPPORTED), the
 *              standalone encoding stages excepted (ngm_encode_fwd / ngm_encode_bwd never run the hidden layers).
 * tests/_config_matrix.py holds the table these lines are tested against. */
#define NGM_MAX_LAYERS 4
#define NGM_NUM_LOSS_SUMS 16

enum ngm_status {
  NGM_OK = 0,
  NGM_E_INVALID = -1,     /* bad argument / inconsistent sizes          */
  NGM_E_UNSUPPORTED = -2, /* configuration has no compiled kernel       */
  NGM_E_WORKSPACE = -3,   /* workspace too small                        */
  NGM_E_HIP = -4          /* HIP runtime error (launch / device)        */
};

enum ngm_encoding { NGM_ENC_NONE = 0, NGM_ENC_FOURIER = 1, NGM_ENC_NERF = 2, NGM_ENC_PERMUTO = 3, NGM_ENC_TRIPLANE = 4 };
enum ngm_triplane_mode { NGM_TRI_SUM = 0, NGM_TRI_PRODUCT = 1, NGM_TRI_CONCAT = 2 };   /* positional_encodings.py:152-161 */
enum ngm_skip_mode { NGM_SKIP_NO = 0, NGM_SKIP_ADD = 1, NGM_SKIP_CONCAT = 2 }; /* models.py:159-180; rezero: the reference's constructor raises */
/* Arithmetic of the hidden layers' matrix products: forward kernels (fused render, point evaluation, kNN evaluation)
 * and the fused training step's MLP backward.
 * NGM_MATMUL_F32: exact-fp32 MFMA.  NGM_MATMUL_BF16X3: every fp32 operand is split exactly into three bf16
 * (hi + mid + lo) and the six leading cross products are summed in fp32 on the bf16 matrix pipe -- fp32-level accuracy
 * (dropped terms < 2^-23 relative), not narrower arithmetic; bitwise deterministic; compiled for 33..64-wide layers,
 * <= 2 hidden layers, Fourier / no encoding, skip_mode no.  As an explicit request ngm_render_fwd returns
 * NGM_E_UNSUPPORTED where it is not compiled or its weight planes (24 KB of LDS per layer) do not fit -- never a silent
 * fallback.  NGM_MATMUL_AUTO: the split wherever it is compiled and fits, exact-fp32 MFMA otherwise (resolved per batch
 * shape by the same plan in forward and backward).  The fused step's MLP backward follows the mode on its own terms:
 * F32 -> fp32 MFMA; BF16X3 / AUTO -> the split kernel where it is compiled (49..64-wide layers, 1-2 hidden layers,
 * Fourier / NeRF / no encoding, skip_mode no, activation stash present), fp32 MFMA otherwise. */
enum ngm_matmul_mode { NGM_MATMUL_F32 = 0, NGM_MATMUL_BF16X3 = 1, NGM_MATMUL_AUTO = 2 };
enum ngm_param_dtype { NGM_DT_F32 = 0, NGM_DT_BF16 = 1, NGM_DT_F16 = 2 };   /* storage type of the weights (ngm_params.dtype) */
enum ngm_scale_mode { NGM_SCALE_NO = 0, NGM_SCALE_UNIT_BALL = 1, NGM_SCALE_UNIT_CUBE = 2 };
enum ngm_geometry_mode { NGM_GEO_NRGBD = 0, NGM_GEO_OCCUPANCY = 1, NGM_GEO_DENSITY = 2, NGM_GEO_NEUS = 3 };

/* slots of the loss partial-sum vector (rm.py:1769-1872); counts are stored as floats */
enum ngm_loss_slot {
  NGM_LS_PHOTO_SUM = 0, /* sum |rgb - rgb*| over masked rays, 3 channels     */
  NGM_LS_PHOTO_CNT = 1, /* number of masked rays (mean divides by 3*cnt)      */
  NGM_LS_DEPTH_SUM = 2, /* sum huber(depth - depth*)                          */
  NGM_LS_DEPTH_CNT = 3,
  NGM_LS_FS_SUM = 4,    /* sum (g*tau - tau)^2 over free-space samples        */
  NGM_LS_FS_CNT = 5,
  NGM_LS_TSDF_SUM = 6,  /* sum (g*tau - (gt - t))^2 over truncation samples   */
  NGM_LS_TSDF_CNT = 7,
  NGM_LS_TERM_SUM = 8,  /* sum (term - term*)^2 over term_mask rays           */
  NGM_LS_TERM_CNT = 9,
  NGM_LS_PHOTO_L1_SUM = 10 /* photometric gaussian_nll only: sum |rgb - rgb*| for its L1 branch (losses.py:34-35) */
};

/* NeuralField architecture: models.py:69-128, positional_encodings.py:167-195,222-243 */
typedef struct ngm_field_cfg {
  int32_t encoding;     /* ngm_encoding */
  int32_t dim_enc;      /* D: encoding output width (Fourier: dim_out; NeRF: 6*octaves)      */
  int32_t raw_coords;   /* Fourier: 1 -> cat(x, sin(Wx)), W is (D-3,3); 0 -> sin(Wx), (D,3)  */
  int32_t num_octaves;  /* NeRF */
  int32_t start_octave; /* NeRF */
  int32_t num_layers;   /* L hidden Linear+ReLU layers (skip_mode "no")                     */
  int32_t dim_hidden;   /* H (= D when dim_mlp_out is null, models.py:99-100)               */
  int32_t dim_out;      /* 4: r,g,b,geometry                                                */
  int32_t scale_mode;   /* ngm_scale_mode, models.py:278-285                                */
  float field_radius;
  /* permutohedral hash encoding (positional_encodings.py:19-66, config/neural_graph_map.yaml:6-14).
   * PARITY UNPINNED: the arithmetic of the reference lives in an un-vendored CUDA package; the kernels
   * implement the published lattice algorithm as restated in oracle/ngm_oracle.py:encode_permuto. */
  int32_t nr_levels;          /* L <= 16; dim_enc = L * nr_feat_per_level                          */
  int32_t nr_feat_per_level;  /* 2                                                                 */
  int32_t log2_hashmap_size;  /* table entries per level T = 2^log2                                */
  float coarsest_scale, finest_scale; /* sigma_l = geomspace(coarsest, finest, L)                  */
  float level_scale[16 * 3];  /* per level, per axis i: 1 / (sqrt((i+1)(i+2)) * sigma_l); fill with    */
                              /* ngm_permuto_fill_scales() (or from numpy.geomspace, as _capi.py does)  */
  int32_t skip_mode;          /* ngm_skip_mode: "add" adds the encoding to the first D units after every       */
                              /* hidden layer (models.py:162-169); needs dim_hidden >= dim_enc.  "concat"       */
                              /* appends it (models.py:159-161): layers 1..L (incl. the output layer) then have */
                              /* H + D inputs, "_linears.{i}.weight" is (out_i, H + D) for i >= 1               */
  int32_t matmul_mode;        /* ngm_matmul_mode of the hidden layers' matrix products (see the enum)             */
  /* triplane encoding (positional_encodings.py:69-161): three (C, res, res) feature planes per field, bilinear lookup
   * (grid_sample, align_corners, border padding) of the (x,y), (x,z), (y,z) projections of a point in [-1,1]^3,
   * combined per ngm_triplane_mode; dim_enc = C (sum, product) or 3 C (concat) */
  int32_t tri_resolution;
  int32_t tri_mode;
  /* ABI 10: two choices that used to be process-wide switches, now part of the configuration (two renderers of one process
   * may differ; ngm_render_workspace sizes the workspace for the configuration it is handed) */
  int32_t activation_stash;   /* ngm_activation_stash: what the training forward of a two-hidden-layer network on the split
                               * path stashes for the backward                                                            */
  int32_t hash_grad_atomics;  /* ngm_hash_grad_atomics: accumulation of the hash-table gradient (k_hash_grad)               */
} ngm_field_cfg;
/* NGM_STASH_FULL: both hidden layers' outputs (512 B per sample; fastest).  NGM_STASH_HALF: layer 0's output only (256 B
 * per sample: half the stash memory and HBM traffic); k_field_bwd_b3<HS> recomputes the output layer's input on the matrix
 * pipe.  Same results at the same tolerances, each bitwise reproducible. */
enum ngm_activation_stash { NGM_STASH_FULL = 0, NGM_STASH_HALF = 1 };
/* NGM_HASH_ATOMICS_EXACT (default): Q23.40 fixed-point integer LDS atomics -- order-independent, the table gradient is
 * bitwise reproducible.  NGM_HASH_ATOMICS_FLOAT (opt-in): fp32 LDS atomics, what the reference's CUDA package does with its
 * global float atomics -- the same sums up to the rounding of the order the adds happen to land in (NOT reproducible run
 * to run), half the LDS per workgroup, no fixed-point conversion.
 * The table gradient keeps one level's accumulators in LDS: every backward (ngm_encode_bwd, ngm_field_eval_bwd*, the render
 * backward) takes log2_hashmap_size <= 13 with EXACT, <= 14 with FLOAT, and returns NGM_E_UNSUPPORTED before it launches
 * anything for a larger table.  The forward entry points take every table size check_field_cfg accepts. */
enum ngm_hash_grad_atomics { NGM_HASH_ATOMICS_EXACT = 0, NGM_HASH_ATOMICS_FLOAT = 1 };

/* fills cfg->level_scale from nr_levels / coarsest_scale / finest_scale (double precision) */
int ngm_permuto_fill_scales(ngm_field_cfg* cfg);

/* Stacked per-field parameters, models.py:245-276 (`all_fields_params` / `vmap_fields_params`).
 * One device pointer per tensor plus the element stride between consecutive fields, so both a
 * dict of separate (N,...) tensors and views into one arena are accepted.  `field_index`
 * (optional, int64[F]) selects rows: batch field f uses row field_index[f] (NULL: row f). */
typedef struct ngm_params {
  const float* enc_w; /* "_encoding._linear.weight" (N, D-3|D, 3); NULL unless Fourier */
  int64_t enc_w_stride;
  const float* w[NGM_MAX_LAYERS + 1]; /* "_linears.{i}.weight" (N, out_i, in_i) */
  int64_t w_stride[NGM_MAX_LAYERS + 1];
  const float* b[NGM_MAX_LAYERS + 1]; /* "_linears.{i}.bias" (N, out_i) */
  int64_t b_stride[NGM_MAX_LAYERS + 1];
  const int64_t* field_index;
  const float* lattice; /* "_encoding.lattice_values" (N, L, T, 2); NULL unless permutohedral */
  int64_t lattice_stride;
  const float* shift;   /* "_encoding.random_shift_per_level" (N, L, 3); always fp32 (constants) */
  int64_t shift_stride;
  int32_t dtype;        /* ngm_param_dtype: STORAGE type of enc_w, w[], b[] and lattice.  NGM_DT_BF16 / NGM_DT_F16: the
                         * pointers above address 16-bit elements (strides stay element counts); the kernels widen
                         * them to fp32 when they stage a field's weights into LDS / gather the hash table, and
                         * compute in fp32 exactly as for fp32 storage (BASELINE configs 1 and 4: bf16 / fp16 weights;
                         * the reference itself is fp32 only).  Gradients and Adam moments stay fp32.            */
  int32_t reserved_;
  const float* planes;  /* "_encoding.plane_coef" (N, 3, C, res, res), fp32; NULL unless triplane */
  int64_t planes_stride;
  const float* neus_sd; /* "_neus_sd" (N,), fp32: per-field standard deviation of the neus geometry mode (rm.py:641-644); */
  int64_t neus_sd_stride; /* required by the fused render entry points in that mode, ignored otherwise                      */
} ngm_params;

/* Gradient outputs, same layout rules as ngm_params (row f of each tensor = batch field f). */
typedef struct ngm_grads {
  float* enc_w;
  int64_t enc_w_stride;
  float* w[NGM_MAX_LAYERS + 1];
  int64_t w_stride[NGM_MAX_LAYERS + 1];
  float* b[NGM_MAX_LAYERS + 1];
  int64_t b_stride[NGM_MAX_LAYERS + 1];
  float* lattice;       /* (F, L, T, 2): fully overwritten by the backward entry points                */
  int64_t lattice_stride;
  float* neus_sd;       /* (F,) d loss / d "_neus_sd" (neus geometry mode, fused render backward) or NULL */
  float* planes;        /* (F, 3, C, res, res): fully overwritten by the backward entry points (triplane) */
  int64_t planes_stride;
} ngm_grads;

/* Loss modes of losses.py built into the fused kernels: all of them.
 * losses.py:26-36.  GAUSSIAN_NLL: 0.5 e^2 / var + log sqrt(var) over the rendered colour variances (rm.py:781-785, no epsilon),
 * replaced by the L1 loss whenever its global mean exceeds 2 (the reference's data-dependent switch). */
typedef enum ngm_photometric_mode { NGM_PHOTO_L1 = 0, NGM_PHOTO_L2 = 1, NGM_PHOTO_GAUSSIAN_NLL = 2 } ngm_photometric_mode;
/* losses.py:60-75.  GAUSSIAN_NLL: 0.5 e^2 / (var + 1e-15) + log sqrt(var + 1e-15); LAPLACIAN_NLL: |e| / sqrt(0.5 var + 1e-6)
 * + 0.5 log(2 var + 1e-6), var = the rendered depth variance (rm.py:786-790).  The variance-weighted modes differentiate
 * through the variances; they run the compositing backward as a launch of its own (k_stash_bwd). */
typedef enum ngm_depth_mode { NGM_DEPTH_HUBER = 0, NGM_DEPTH_GAUSSIAN_NLL = 1, NGM_DEPTH_LAPLACIAN_NLL = 2 } ngm_depth_mode;

/* Renderer + loss constants: rm.py:116-220, config/neural_graph_map.yaml */
typedef struct ngm_render_cfg {
  int32_t geometry_mode;       /* ngm_geometry_mode, rm.py:746-762            */
  int32_t num_samples_coarse;  /* S_c                                         */
  int32_t num_samples_guided;  /* S_g (0: single stratum, eval style)         */
  int32_t overwrite_behind_camera; /* != 0: samples with z_cam > 0 get a constant geometry value and no
                                    * gradient (rm.py:614-622: -100 occupancy/density, 1.0 neus/nrgbd)  */
  float geometry_factor;       /* gamma                                       */
  float color_factor;
  float truncation_distance;   /* tau                                         */
  float range_depth_guided;    /* rho (rm.py:169-170)                         */
  float fx, fy, cx, cy;        /* intrinsics at pixel centre 0 (camera.py:188) */
  float w_termination, w_photometric, w_depth, w_freespace, w_tsdf; /* rm.py:129-135 */
  float huber_delta;           /* 0.05, losses.py:63                          */
  float term_threshold;        /* 0.8, rm.py:1787                             */
  int32_t photometric_mode;    /* ngm_photometric_mode (config key photometric_loss, losses.py:26-29); ABI 3 */
  int32_t depth_mode;          /* ngm_depth_mode (config key depth_loss, losses.py:60-75)                    */
} ngm_render_cfg;

/* One batch of rays: the reference's Target record (rm.py:43-58) in device memory. */
typedef struct ngm_rays {
  int32_t F, R;
  const int64_t* ijs;      /* (F,R,2) [row, col]                                            */
  const float* c2ws;       /* (F,R,4,4) when c2w_per_ray != 0 else (4,4) shared              */
  int32_t c2w_per_ray;
  int32_t philox_offset_autoinc; /* != 0 (training forward with targets only): *philox_offset_dev is incremented once
                                  * after every workgroup of the forward has read it (the loss-reduction kernel does
                                  * it), i.e. the counter counts iterations; ngm_adam_sparse_multi can read the same
                                  * counter as its device-side step.  The pointer is then written through.         */
  const float* near;       /* (F,R) or NULL -> near_const                                    */
  const float* far;        /* (F,R) or NULL -> far_const                                     */
  const float* gt;         /* (F,R) or NULL; 0.0 = no depth                                  */
  float near_const, far_const;
  const float* field_pos;  /* (F,3) field positions in the world frame                       */
  const float* field_quat; /* (F,4) real-first quaternions, applied like pytorch3d's quaternion_apply (raw        */
                           /* Hamilton products, models.py:338-339: a norm != 1 scales the local frame by |q|^2) */
  const float* u_coarse;   /* (F,R,S_c) torch.rand draws of camera.py:274, or NULL -> Philox */
  const float* u_guided;   /* (F,R,S_g) or NULL -> Philox                                    */
  const float* lin_coarse; /* (S_c+1) torch.linspace(0,1) table of camera.py:271 or NULL     */
  const float* lin_guided; /* (S_g+1) or NULL                                                */
  uint64_t philox_seed;    /* used when u_* is NULL                                          */
  uint64_t philox_offset;
  const int64_t* pose_index;          /* optional (F,): batch field f uses field_pos/field_quat row pose_index[f] */
  const uint64_t* philox_offset_dev;  /* optional device counter added to philox_offset (hipGraph replay:  */
                                      /* a captured step draws fresh jitter every replay)                   */
} ngm_rays;

/* Supervision of one batch (rm.py:43-58, 1769-1872); masks are uint8 0/1. */
typedef struct ngm_targets {
  const float* rgbds;        /* (F,R,4) r,g,b,depth                 */
  const uint8_t* depth_mask; /* (F,R)                               */
  const uint8_t* term_mask;  /* (F,R) or NULL (all false)           */
  const float* term_probs;   /* (F,R) or NULL                       */
} ngm_targets;

/* Per-ray outputs: the reference's Prediction (rm.py:59-69) minus the data-dependent vectors. */
typedef struct ngm_prediction {
  float* rgbds;      /* (F,R,4) */
  float* color_vars; /* (F,R,3) */
  float* depth_vars; /* (F,R)   */
  float* term_probs; /* (F,R)   */
} ngm_prediction;

/* ---- library ------------------------------------------------------------------------------ */
int ngm_abi_version(void);
const char* ngm_last_error(void);
/* number of compute units / device name of the current device (for launch sizing, bench) */
int ngm_device_info(int* num_cus, char* name, int name_len);

/* ---- K1: ray sampler ----------------------------------------------------------------------
 * Replaces Camera.ijs_to_directions + Camera.sample_ijs_uniform (camera.py:186-292), the
 * depth-guided merge + sort + gather (rm.py:521-545).  Outputs the sorted samples in the camera
 * frame: points_cam (F,R,S,3), distances (F,R,S), dirs (F,R,3) (any may be NULL). */
int ngm_sample_rays(const ngm_render_cfg* cfg, const ngm_rays* rays, float* points_cam,
                    float* distances, float* dirs, void* stream);
/* same, additionally the samples in the WORLD frame (utils.transform_points, utils.py:276-286 via
 * rm.py:547): points_world (F,R,S,3) = R(c2w) p_cam + t(c2w). */
int ngm_sample_rays_world(const ngm_render_cfg* cfg, const ngm_rays* rays, float* points_cam,
                          float* points_world, float* distances, float* dirs, void* stream);
/* Camera.sample_ijs_uniform with `weights` / `boundaries` (camera.py:227-244, 277-289; no caller inside run_mapping.py, part of
 * the Camera interface): weighted sampling from distance bins given per ray by sorted boundaries (F,R,num_bins+1) and bin
 * probabilities weights (F,R,num_bins): bin = searchsorted(cumsum(weights) + 1e-3, u_bin), distance = boundaries[bin] +
 * (boundaries[bin+1] - boundaries[bin]) * u_off; cfg->num_samples_coarse samples per ray, in DRAW order (the reference does
 * not sort this branch).  rays->u_coarse = the first torch.rand draw (bins), rays->u_guided = the second (offsets), both
 * (F,R,S), or both NULL = words 0 / 1 of Philox block (ray * S + sample, stream 0); rays->near / far / gt are not read.  The running sum is torch.cumsum's on the
 * CPU (sequential, fp64 accumulator, every prefix rounded to fp32); a draw beyond the last cumulative weight takes the last bin (the reference's gather is out
 * of range there).  Outputs as ngm_sample_rays (any may be NULL). */
int ngm_sample_rays_weighted(const ngm_render_cfg* cfg, const ngm_rays* rays, int32_t num_bins, const float* boundaries,
                             const float* weights, float* points_cam, float* distances, float* dirs, void* stream);

/* ---- K2+K3: NeuralFieldSet.forward(use_vmap=True) -----------------------------------------
 * models.py:329-345: world -> field-local transform, scaling, encoding, MLP; points (F,P,3)
 * (world frame when field_pos/field_quat are given, local otherwise), out (F,P,4). */
int ngm_field_eval_fwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                       const float* points, const float* field_pos, const float* field_quat,
                       float* out, void* stream);
/* The positional encoding of the same points ALONE (standalone stage entry point for roofline accounting;
 * positional_encodings.py:19-66 permutohedral hash, :164-276 Fourier / NeRF octaves): out (F,P,dim_enc).  The fused kernels
 * never materialise this tensor.  Triplane: NGM_E_UNSUPPORTED. */
int ngm_encode_fwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                   const float* points, const float* field_pos, const float* field_quat,
                   float* out, void* stream);
/* Backward of the encoding alone: d_enc (F,P,dim_enc) -> the encoding's parameter gradients, fully overwritten.  Fourier
 * (positional_encodings.py:197-212): grads->enc_w (F, dim_enc - 3, 3) = sum_p d_enc cos(W x) x; permutohedral hash
 * (:19-66): grads->lattice (F, L, T, 2) through the table-gradient kernel of the training step.  NeRF octaves / no encoding
 * have no parameters (returns NGM_OK, nothing written); the triplane encoding returns NGM_E_UNSUPPORTED (its gradient exists
 * inside ngm_field_eval_bwd only).  Other members of `grads` are ignored. */
int64_t ngm_encode_bwd_workspace(const ngm_field_cfg* fcfg, int32_t F, int64_t P);
int ngm_encode_bwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                   const float* field_pos, const float* field_quat, const float* d_enc, const ngm_grads* grads,
                   void* workspace, int64_t workspace_bytes, void* stream);
/* Backward of the above w.r.t. every parameter: d_out (F,P,4) -> grads.  workspace: see
 * ngm_field_eval_bwd_workspace(). */
int ngm_field_eval_bwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                       const float* points, const float* field_pos, const float* field_quat,
                       const float* d_out, const ngm_grads* grads, void* workspace,
                       int64_t workspace_bytes, void* stream);
int64_t ngm_field_eval_bwd_workspace(const ngm_field_cfg* fcfg, int32_t F, int64_t P);
/* Training pair of the above (ABI 11; models.py:329-345 under autograd -- the path the reference's unchanged
 * _optimization_iteration takes, rm.py:1164-1177).  ngm_field_eval_fwd_train computes what ngm_field_eval_fwd computes (same
 * kernel, same bits) and also writes the hidden activations of every sample into the caller-owned `stash`
 * (ngm_field_eval_stash_bytes: 256 B per sample and hidden layer + one tile); ngm_field_eval_bwd_stash reads them back instead
 * of recomputing the hidden layers and runs the MLP backward of the fused training step (bf16-split matrix products, fp32
 * accumulate) on the explicit points.  ngm_field_eval_stash_bytes returns 0 when the configuration has no stash-reading
 * backward (anything but 33..64-wide encoding and hidden layers, 1-2 layers, Fourier / NeRF / no encoding, skip_mode no,
 * matmul_mode auto / bf16x3): the pair then returns NGM_E_UNSUPPORTED and ngm_field_eval_fwd / ngm_field_eval_bwd serve the
 * call.  `points`, poses and parameters passed to the backward must be those of the forward that wrote the stash.
 * workspace of the backward: ngm_field_eval_bwd_workspace(). */
int64_t ngm_field_eval_stash_bytes(const ngm_field_cfg* fcfg, int32_t F, int64_t P);
int ngm_field_eval_fwd_train(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                             const float* points, const float* field_pos, const float* field_quat,
                             float* out, void* stash, int64_t stash_bytes, void* stream);
int ngm_field_eval_bwd_stash(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                             const float* points, const float* field_pos, const float* field_quat,
                             const float* d_out, const ngm_grads* grads, const void* stash, int64_t stash_bytes,
                             void* workspace, int64_t workspace_bytes, void* stream);

/* ---- K4: volume renderer -------------------------------------------------------------------
 * NeuralGraphMap._quadrature (rm.py:709-799) on N rays x S samples: colors (N,S,3), geoms (N,S),
 * dists (N,S), depths (N,S), neus_isds (N) or NULL.  Outputs: C (N,3), D (N), Cvar (N,3),
 * Dvar (N), term (N), weights (N,S_eff) (any may be NULL). */
int ngm_composite_fwd(const ngm_render_cfg* cfg, int64_t N, int32_t S, const float* colors,
                      const float* geoms, const float* dists, const float* depths,
                      const float* neus_isds, float* C, float* D, float* Cvar, float* Dvar,
                      float* term, float* weights, void* stream);
/* Same quadrature fed directly by the (N,S,4) field outputs [r,g,b,geometry] (colour scaled by
 * cfg->color_factor, rm.py:610-612) and the camera-frame sample points (depth = -z): the eval path
 * render_image -> _render_ijs(use_vmap=False) -> _quadrature (rm.py:402-437, 586-595, 650-656). */
int ngm_composite_fwd_packed(const ngm_render_cfg* cfg, int64_t N, int32_t S, const float* field_out4,
                             const float* dists, const float* points_cam, float* rgbd, float* Cvar,
                             float* Dvar, float* term, void* stream);
/* Backward of C, D, term w.r.t. colors (N,S,3), geoms (N,S) and, in neus mode, the per-ray inverse
 * standard deviations (N) (d_neus_isds may be NULL).  All four geometry modes. */
int ngm_composite_bwd(const ngm_render_cfg* cfg, int64_t N, int32_t S, const float* colors,
                      const float* geoms, const float* dists, const float* depths,
                      const float* neus_isds, const float* dC, const float* dD,
                      const float* dterm, float* d_colors, float* d_geoms, float* d_neus_isds,
                      void* stream);

/* ---- fused render / train step -------------------------------------------------------------
 * ngm_render_fwd replaces NeuralGraphMap._render_ijs(use_vmap=True) (rm.py:439-666): sampler ->
 * world->local -> encoding -> MLP -> compositing in ONE kernel.  When `targets` is non-NULL it
 * also accumulates the loss partial sums of _compute_losses (rm.py:1769-1872) into
 * loss_sums[NGM_NUM_LOSS_SUMS] (device, overwritten) and fills the saved-for-backward part of
 * the workspace.  loss_sums == NULL with targets = DEFERRED reduction: the per-workgroup partial sums
 * stay in the workspace and the matching ngm_render_bwd / ngm_render_bwd_adam call (also with
 * loss_sums == NULL) sums them itself -- one launch less per step on a single GPU, where nothing
 * (no all-reduce) happens between forward and backward; the philox_offset_autoinc counter is then
 * advanced by the backward.  sample_stash (optional, (F,R,S,6): r,g,b,geometry,t,T) exposes the per-sample
 * values for callers that need the compacted free-space / TSDF vectors of the Prediction. */
int64_t ngm_render_workspace(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t F,
                             int32_t R, int32_t train);
int ngm_render_fwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg,
                   const ngm_params* params, const ngm_rays* rays, const ngm_targets* targets,
                   const ngm_prediction* pred, float* loss_sums, void* workspace,
                   int64_t workspace_bytes, void* stream);
/* Backward of loss["combined"] (rm.py:1871) w.r.t. every field parameter.  loss_sums are the
 * GLOBAL sums/counts (after the caller's cross-GPU all-reduce of ngm_render_fwd's output);
 * workspace must be the one filled by the matching ngm_render_fwd call.  The workspace is
 * SINGLE-USE: every ngm_render_bwd* call overwrites the saved forward values with the per-sample
 * gradients in place, so a second backward needs a new ngm_render_fwd.  loss_out (optional,
 * device float[8]): combined, termination, photometric, depth, freespace, tsdf. */
int ngm_render_bwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg,
                   const ngm_params* params, const ngm_rays* rays, const ngm_targets* targets,
                   const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                   float* loss_out, void* workspace, int64_t workspace_bytes, void* stream);
/* Generic-seed variant used by the autograd wrapper of render_ijs: explicit dL/d(rgbds) (F,R,4),
 * dL/d(term_probs) (F,R) and optional per-sample dL/d(geometry) (F,R,S). */
int ngm_render_bwd_seeded(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg,
                          const ngm_params* params, const ngm_rays* rays, const float* d_rgbds,
                          const float* d_term, const float* d_geom_samples,
                          const ngm_grads* grads, void* workspace, int64_t workspace_bytes,
                          void* stream);
/* The same with seeds on the rendered variances as well (rm.py:781-790: V = sum_k w_k (c_k - C)^2): dL/d(color_vars) (F,R,3)
 * and dL/d(depth_vars) (F,R), either may be NULL; `pred` = the forward's outputs (rgbds and term_probs are read: the means and
 * the weight sum the variances are taken around).  What the reference's autograd does for losses.py's *_nll modes. */
int ngm_render_bwd_seeded_vars(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg,
                               const ngm_params* params, const ngm_rays* rays, const ngm_prediction* pred,
                               const float* d_rgbds, const float* d_color_vars, const float* d_depth_vars,
                               const float* d_term, const float* d_geom_samples, const ngm_grads* grads,
                               void* workspace, int64_t workspace_bytes, void* stream);
/* read access to the per-sample values saved by ngm_render_fwd(train): copies geometry (F,R,S)
 * and sorted distances (F,R,S) out of the workspace (for Prediction.freespace_geometry /
 * tsdf_residuals, rm.py:624-639).  S = the samples per ray the forward ran with: S_c + S_g when
 * its rays carried gt, S_c otherwise (anything else: NGM_E_INVALID); geoms / dists hold F*R*S floats. */
int ngm_render_read_samples(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t F,
                            int32_t R, int32_t S, const void* workspace, float* geoms, float* dists,
                            void* stream);

/* ---- sparse per-field Adam (rm.py:347-389, 668-707, 1183-1221) ---------------
 * torch.optim.Adam (L2-coupled weight decay) applied in place to rows field_index[f] of one
 * stacked tensor of `numel_per_field` elements: param/exp_avg/exp_avg_sq have `stride` elements
 * between fields, grad is (F, numel_per_field) with grad_stride.  `step` is the NEW shared step
 * count (one counter for all fields, rm.py:380-385). */
int ngm_adam_sparse(float* param, float* exp_avg, float* exp_avg_sq, int64_t stride,
                    const float* grad, int64_t grad_stride, const int64_t* field_index, int32_t F,
                    int64_t numel_per_field, int64_t step, float lr, float beta1, float beta2,
                    float eps, float weight_decay, void* stream);

/* All parameter tensors of a field set in ONE launch.  `step_dev` (optional device int64) overrides
 * `step` so that a captured hipGraph advances the bias correction on every replay.  End-of-iteration
 * bookkeeping can ride along: with advance_step_dev != 0 the kernel does ++*step_dev, and with a non-NULL
 * advance_philox_offset_dev ++*that, once every block has finished (same effect as ngm_step_advance, but
 * measured slower than the separate launch on MI355X: every block fences its stores first). */
typedef struct ngm_adam_tensor {
  float* param; float* exp_avg; float* exp_avg_sq; /* (N, numel) rows with `stride` elements between fields */
  const float* grad;                               /* (F, numel) rows with `grad_stride`                    */
  int64_t stride, grad_stride, numel;
  void* param_lp;                                  /* optional reduced-precision copy of `param` (same row layout,  */
  int32_t lp_dtype;                                /* 16-bit elements, ngm_param_dtype): refreshed with every update */
  int32_t reserved_;                               /* (fp32 master weights + the copy the kernels read)              */
} ngm_adam_tensor;
int ngm_adam_sparse_multi(const ngm_adam_tensor* tensors, int32_t num_tensors, const int64_t* field_index,
                          int32_t F, int64_t step, int64_t* step_dev, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int32_t advance_step_dev,
                          uint64_t* advance_philox_offset_dev, void* stream);
/* ngm_render_bwd + the sparse Adam update of the active fields (rm.py:1183-1221) with the MLP tensors updated by the
 * gradient-reduction kernel itself (no Adam launch, no gradient round trip; the gradients are still written to `grads`).
 * mlp_tensors: one entry per gradient segment, in the order enc_w (Fourier encoding only), w_0, b_0, ..., w_L, b_L
 * (their `grad` members are ignored); lattice_tensor: the hash tables (permutohedral encoding only, NULL otherwise),
 * updated by the table-gradient reduction kernel.  step / step_dev as in ngm_adam_sparse_multi. */
int ngm_render_bwd_adam(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params,
                        const ngm_rays* rays, const ngm_targets* targets, const ngm_prediction* pred,
                        const float* loss_sums, const ngm_grads* grads, const ngm_adam_tensor* mlp_tensors,
                        int32_t num_mlp_tensors, const ngm_adam_tensor* lattice_tensor, const int64_t* field_index,
                        int64_t step, int64_t* step_dev, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float* loss_values, void* workspace, int64_t workspace_bytes, void* stream);
/* ---- counted step: the training step launched at a CAPACITY, the number of active rows in device memory -------------
 * ngm_render_fwd / ngm_render_bwd / ngm_render_bwd_adam with one more argument: num_active, a DEVICE int32 (for instance
 * ngm_target_out.count of ngm_target_sample_mv) with 0 <= *num_active <= rays->F.  Plans, workspace size
 * (ngm_render_workspace(fcfg, rcfg, rays->F, R, 1)) and validation are those of the un-suffixed call with the same rays->F;
 * no kernel launch depends on the count, so the sequence can be captured in a graph whose replays see a new count each.
 * Rows 0 .. *num_active - 1 are the batch.  For rows f >= *num_active:
 *   - nothing of theirs is READ: not params->field_index[f] / rays->pose_index[f] / the Adam field_index[f], not their rays,
 *     targets or masks -- the result of the call is bitwise independent of what those rows hold;
 *   - nothing of theirs is WRITTEN: prediction rows, gradient rows (hash `lattice` rows included), parameter / Adam moment /
 *     reduced-precision rows stay as they were (gradient and prediction rows >= *num_active are therefore unspecified
 *     leftovers of earlier calls); no parameter row other than field_index[0 .. *num_active - 1] changes;
 *   - they contribute exactly nothing to the loss sums and counts.
 * Bookkeeping happens once per call whatever the count: loss_sums / loss_values written, the philox_offset_autoinc counter
 * (and with it the Adam step it doubles as) advanced.  *num_active == 0 is a legal call: zero sums, hence the loss values of
 * empty selections (NaN terms, as the reference's empty .mean()), no parameter touched.  *num_active == rays->F computes
 * bit for bit what the un-suffixed call computes.
 * num_active == NULL: NGM_E_INVALID.  The neus geometry mode, the triplane encoding (both run launches over all F rows)
 * and the *_nll loss modes: NGM_E_UNSUPPORTED.  These two checks come before every other and read only fcfg and rcfg. */
int ngm_render_fwd_counted(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg,
                           const ngm_params* params, const ngm_rays* rays, const ngm_targets* targets,
                           const ngm_prediction* pred, float* loss_sums, void* workspace,
                           int64_t workspace_bytes, void* stream, const int32_t* num_active);
int ngm_render_bwd_counted(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg,
                           const ngm_params* params, const ngm_rays* rays, const ngm_targets* targets,
                           const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                           float* loss_out, void* workspace, int64_t workspace_bytes, void* stream,
                           const int32_t* num_active);
int ngm_render_bwd_adam_counted(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params,
                                const ngm_rays* rays, const ngm_targets* targets, const ngm_prediction* pred,
                                const float* loss_sums, const ngm_grads* grads, const ngm_adam_tensor* mlp_tensors,
                                int32_t num_mlp_tensors, const ngm_adam_tensor* lattice_tensor, const int64_t* field_index,
                                int64_t step, int64_t* step_dev, float lr, float beta1, float beta2, float eps,
                                float weight_decay, float* loss_values, void* workspace, int64_t workspace_bytes, void* stream,
                                const int32_t* num_active);
/* ++*step_dev, ++*philox_offset_dev on the stream (either may be NULL): end-of-iteration bookkeeping
 * for graph-captured training loops. */
int ngm_step_advance(int64_t* step_dev, uint64_t* philox_offset_dev, void* stream);

/* ---- eval path: kNN-blended field evaluation (models.py:347-405) --------------------------
 * points (P,3) world; all N_f fields' poses; params cover all N_f fields (field_index optional,
 * maps field slot -> parameter row).  out (P,4).  K = min(num_knn, N_f) <= 16 (unrolled neighbour lists for K <= 8, one 16-slot instance above); N_f unbounded (the centres are binned into a
 * uniform grid in the workspace per call; exact K nearest, distance ties to the lower field index).
 * mask_radius: the `field_radius` ARGUMENT of NeuralFieldSet.forward (models.py:293, 368): a point is evaluated when its
 * nearest field centre is closer than this; the local coordinates are still scaled with fcfg->field_radius
 * (models.py:278-285, 378) -- _extract_mesh colours its vertices with radius + 0.1 (rm.py:2324-2336).  <= 0: fcfg->field_radius. */
int64_t ngm_field_eval_knn_workspace(int32_t num_fields, int64_t P, int32_t num_knn);
int ngm_field_eval_knn(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t num_fields,
                       int64_t P, const float* points, const float* field_pos,
                       const float* field_quat, int32_t num_knn, float distance_factor,
                       float outside_value, float mask_radius, float* out, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ---- eval path on a lattice: one block of _extract_mesh's dense grid (rm.py:2236-2261) as one call -----------------------
 * = ngm_field_eval_knn on torch.cartesian_prod(xs, ys, zs) followed by "take channel `channel`, reshape to (nx, ny, nz),
 * negate when `negate`", bit for bit, without the (P,3) point array and the (P,4) output: point p is
 * (xs[p / (ny nz)], ys[(p / nz) % ny], zs[p % nz]), formed from the three device axes inside the neighbour assignment and again
 * inside the evaluation (the axes are read as they are: uniform or not), and the blend writes the one channel marching cubes
 * needs into volume (nx, ny, nz) fp32.  The occupancy mode's sigmoid is the caller's (a torch op on the volume).
 * mask_radius, K <= 16, params->field_index and the forward plan as in ngm_field_eval_knn; the workspace is that entry's for
 * nx ny nz points.  Checked before any launch: a side < 1, a NULL axis / volume / pose, channel outside 0..3 ->
 * NGM_E_INVALID; nx ny nz K > 2^31 - 1, num_fields < 1 or K > 16 -> NGM_E_UNSUPPORTED (the workspace query returns the same
 * codes); workspace_bytes below the query's answer -> NGM_E_WORKSPACE. */
int64_t ngm_grid_eval_knn_workspace(int32_t num_fields, int32_t nx, int32_t ny, int32_t nz, int32_t num_knn);
int ngm_grid_eval_knn(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t num_fields, const float* field_pos,
                      const float* field_quat, const float* xs, int32_t nx, const float* ys, int32_t ny, const float* zs,
                      int32_t nz, int32_t num_knn, float distance_factor, float outside_value, float mask_radius,
                      int32_t channel, int32_t negate, float* volume, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- eval path, whole: render_image's loop over pixel blocks (rm.py:402-437) -------------------------------------------
 * = per block of `ray_block` rays: Camera.sample_ijs_uniform + transform_points (rm.py:513-547, eval-style: one stratum of
 * rcfg->num_samples_coarse samples, no depth guidance -- rays->gt / u_guided are ignored), NeuralFieldSet.forward(
 * use_vmap=False) (models.py:347-405) and _quadrature (rm.py:709-799) on the blended outputs.  The same arithmetic as
 * ngm_sample_rays_world -> ngm_field_eval_knn -> ngm_composite_fwd_packed per block, without their intermediates in memory:
 * the samples are drawn inside the neighbour assignment, the blend happens inside the quadrature, the grid over the field
 * centres is built once per call.  rays: rays->F * rays->R rays in all (field_pos / field_quat / pose_index unused); block b
 * draws its jitter from u_coarse, or from the Philox stream (philox_seed + b * ray_block, ray index within the block).
 * pred: (F*R, .) outputs, any may be NULL.  mask_radius as in ngm_field_eval_knn; K <= 8; S <= 1024. */
int64_t ngm_render_eval_knn_workspace(const ngm_render_cfg* rcfg, int32_t num_fields, int32_t ray_block, int32_t num_knn);
int ngm_render_eval_knn(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params,
                        int32_t num_fields, const float* field_pos, const float* field_quat, const ngm_rays* rays,
                        int32_t num_knn, float distance_factor, float outside_value, float mask_radius, int32_t ray_block,
                        const ngm_prediction* pred, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- training-target sampler -------------------------------------------------------
 * Device part of NeuralGraphMap._sample_target_mv (rm.py:1259-1459).  The random draws stay with the caller
 * (torch.multinomial / randn / rand on its generator, as in the reference); the keyframe store is read in place. */
typedef struct ngm_keyframes {
  int32_t num_frames;            /* len(_c_c2w_tensor)                                              */
  int32_t height, width;         /* keyframe image size                                              */
  int32_t reserved0;
  const float* c2ws;             /* (num_frames,4,4) current keyframe poses, rm.py:1711-1713          */
  const float* rgbd;             /* (N_store,height,width,4) keyframe RGB-D store [r,g,b,depth]       */
  const int64_t* frame_to_store; /* (num_frames) _frame_cid_to_ncid, rm.py:1703                       */
  float fx, fy, cx, cy;          /* intrinsics at pixel centre 0 (camera.py:188)                      */
} ngm_keyframes;

/* outputs of ngm_target_rays = the reference's Target record (rm.py:43-58) for F fields x R rays */
typedef struct ngm_target_out {
  int64_t* ijs;        /* (F,R,2) [row, col]        */
  float* c2ws;         /* (F,R,4,4) or NULL         */
  float* near;         /* (F,R)                     */
  float* far;          /* (F,R)                     */
  float* gt;           /* (F,R) ray distance of the keyframe depth, 0 = missing */
  float* rgbds;        /* (F,R,4)                   */
  uint8_t* rgb_mask;   /* (F,R)                     */
  uint8_t* depth_mask; /* (F,R)                     */
  float* term_probs;   /* (F,R)                     */
  uint8_t* term_mask;  /* (F,R)                     */
} ngm_target_out;

/* rm.py:1321-1392: kf_mask (F,num_frames) u8 = keyframe sees the field; bbox (F,num_frames,4) =
 * (min_x, min_y, max_x, max_y) of the projected sphere samples, clamped to the image. */
int ngm_target_visibility(const ngm_keyframes* kf, int32_t F, const float* field_pos, int32_t num_offsets,
                          const float* offsets, float radius, uint8_t* kf_mask, float* bbox, void* stream);
/* rm.py:1394-1459: frame_cids (F,R) i64 = sampled keyframe per ray, u_xy (F,R,2) = pixel uniforms. */
int ngm_target_rays(const ngm_keyframes* kf, int32_t F, int32_t R, const float* field_pos, float radius,
                    const float* bbox, const int64_t* frame_cids, const float* u_xy,
                    const ngm_target_out* out, void* stream);

/* ---- training-target sampler, whole, on the device (opt-in) ---------------------------------------
 * _sample_target_mv (rm.py:1259-1459) with the random draws made on the device from Philox4x32-10 (NOT torch's stream):
 * three launches, no host synchronisation, fixed output capacity, the number of surviving fields left in device memory --
 * so a captured graph draws fresh targets at every replay.  Distribution as in the reference:
 *   n_obs fields uniformly without replacement from current_field_ids (random order), n_rand uniformly without replacement
 *   from the other fields of [0, num_fields); field order = the union sorted ascending if n_rand > 0, else the observed draw
 *   order; 20 Gaussian sphere offsets, normalised; fields no keyframe sees are dropped (the others keep their order); per ray
 *   a keyframe uniform among the field's visible ones, pixel uniforms inside its box.
 * Keying (stream ids 0x54470001-4, distinct from the ray samplers' 0 / 1; Philox offset = iteration):
 *   observed draw: key_j = (word 0 of block ctr=current_field_ids[j], stream ..01) << 32 | j, the n_obs smallest keys;
 *   random draw:   key_f = (word 0 of block ctr=f, stream ..02) << 32 | f over fields not drawn above, the n_rand smallest;
 *   offsets:       Box-Muller on blocks 0..14 of stream ..03 (exact-rounding arithmetic only, restated on the host);
 *   ray k of field id g: block ctr=(g << 32 | k), stream ..04: keyframe = list[(word0 * count) >> 32], u_x / u_y = words 1 / 2
 *   as 24-bit uniforms.  A ray depends on (seed, iteration, g, k) only: not on its row, F, the rank or the other fields.
 * Sharding (world_size W, rank r): every rank draws the same set; only drawn fields with id % W == r get rows, in draw order.
 * Precondition (not checked, as in the reference): current_field_ids duplicate-free, ids in [0, num_fields); ids outside
 * that range are dropped.  capacity must be min(num_observed + num_random, #{id in [0, num_fields): id % W == r}) and
 * num_observed + num_random <= NGM_TARGET_MAX_DRAW.  Every ngm_target_out array is (capacity, R, ...): rows past *count hold
 * field_ids = -1, masks 0 and zeros (frame_cids / u_xy too). */
#define NGM_TARGET_MAX_DRAW 2048
typedef struct ngm_target_sample {
  const int64_t* current_field_ids; /* (num_current)                                                     */
  const float* field_positions;     /* (>= num_fields, 3) map field centres                               */
  int32_t num_current, num_fields;
  int32_t num_observed;             /* min(num_train_fields / 2, num_current)                              */
  int32_t num_random;               /* min(num_train_fields - num_observed, num_fields - num_observed)     */
  int32_t num_rays, capacity;       /* R; output rows                                                      */
  int32_t world_size, rank;
  float radius;                     /* _field_radius                                                       */
  int32_t reserved0;
  uint64_t seed;
  int64_t iteration;                /* >= 0: this iteration; < 0: read *iteration_dev once and advance it by one */
  int64_t* iteration_dev;
  int64_t* field_ids;               /* out (capacity)                                                      */
  int32_t* count;                   /* out (1): surviving fields                                           */
  int64_t* subset_observed;         /* out (num_observed): positions in current_field_ids, draw order     */
  int64_t* subset_random;           /* out (num_random): field ids, draw order                             */
  float* offsets;                   /* out (20,3) normalised sphere offsets                                */
  int64_t* frame_cids;              /* out (capacity,R) keyframe per ray                                   */
  float* u_xy;                      /* out (capacity,R,2) pixel uniforms                                   */
} ngm_target_sample;
int64_t ngm_target_sample_mv_workspace(int32_t num_frames, int32_t num_current, int32_t num_fields, int32_t capacity);
int ngm_target_sample_mv(const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_out* out, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ---- the same sampler with its counts in device memory (opt-in; additive to ABI 11) ---------------------------------
 * ngm_target_sample_mv whose num_current and num_frames are read from DEVICE int32s at run time, so that one captured graph
 * serves every frame (a new observed set) and every keyframe (a longer pose list) -- same three kernels, same keying, and
 * bit for bit the result of ngm_target_sample_mv called with those counts.  The host gives the maxima only:
 *   kf->num_frames = max_frames (row stride of the workspace, grids, the LDS / workspace decision for the keyframe lists),
 *   s->num_current = max_current, s->num_observed = min(T / 2, max_current), s->num_random = min(T, num_fields)  (the
 *   sizes of subset_observed / subset_random), s->capacity = min(min(T, num_fields), fields of this rank)
 * with T = live->num_train_fields.  On the device: nc = clamp(*num_current, 0, max_current), nf = clamp(*num_frames, 0,
 * max_frames), n_obs = min(T / 2, nc), n_rand = max(min(T - n_obs, num_fields - n_obs), 0) -- their sum is min(T, num_fields)
 * whatever nc is, hence the host-known capacity.  *num_observed / *num_random receive n_obs / n_rand; subset_observed /
 * subset_random hold -1 past them.  Nothing past nc in current_field_ids, or past nf in kf->c2ws / kf->frame_to_store, is
 * read.  nf == 0 is legal: no field is seen, *count = 0. */
typedef struct ngm_target_live {
  const int32_t* num_current;   /* device (1)                                                          */
  const int32_t* num_frames;    /* device (1)                                                          */
  int32_t* num_observed;        /* device out (1)                                                      */
  int32_t* num_random;          /* device out (1)                                                      */
  int32_t num_train_fields;     /* T                                                                   */
  int32_t reserved0;
} ngm_target_live;
int64_t ngm_target_sample_mv_live_workspace(int32_t max_frames, int32_t max_current, int32_t num_fields, int32_t capacity);
int ngm_target_sample_mv_live(const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_live* live,
                              const ngm_target_out* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- observed fields of one RGB-D frame, on the device (NeuralGraphMap._get_observed_fields, rm.py:1642-1670) ---------
 * Which fields does the frame see?  num_points pixels are drawn uniformly without replacement among those with depth != 0
 * (camera.py:374 + rm.py:1651), back-projected (OpenGL camera frame), and a field is observed when its sphere's AABB meets
 * the points' AABB (geometry.py:26-42) and some segment camera origin -> point passes through the sphere (geometry.py:67-105).
 * No host synchronisation, fixed output shapes: 11 launches (3 with subset_in).
 * Draw: key_p = (word 0 of Philox block ctr = linear pixel index p, stream 0x54470005, offset = frame) << 32 | p over the
 * pixels with depth; the num_points smallest keys (radix select across workgroups, integer atomics: the chosen SET is
 * deterministic, the order of `pixels` is not).  Fewer valid pixels than num_points: all of them; none: *current_count = 0.
 * frame >= 0: this frame; < 0: *frame_dev is read and advanced by one.  subset_in (num_points linear pixel indices, entries
 * outside [0, H*W) unused) replaces the draw.  1 <= num_points <= NGM_OBSERVED_MAX_POINTS, H*W < 2^31. */
#define NGM_OBSERVED_MAX_POINTS 2048
typedef struct ngm_observed_fields {
  const float* rgbd;              /* (H,W,4) the frame [r,g,b,depth]                                    */
  const float* c2w;               /* DEVICE (4,4) row-major camera pose, read at run time               */
  const float* field_positions;   /* (>= num_fields, 3)                                                 */
  int32_t height, width;
  int32_t num_fields, num_points;
  float fx, fy, cx, cy;           /* intrinsics at pixel centre 0                                       */
  float radius;                   /* _field_radius                                                      */
  int32_t reserved0;
  uint64_t seed;
  int64_t frame;
  int64_t* frame_dev;
  const int64_t* subset_in;       /* (num_points) or NULL                                               */
  int64_t* current_field_ids;     /* out (num_fields): observed ids ascending, -1 past *current_count   */
  int32_t* current_count;         /* out (1)                                                            */
  int64_t* pixels;                /* out (num_points): chosen linear pixel indices, -1 past *num_used   */
  int32_t* num_used;              /* out (1): min(num_points, valid pixels)                             */
} ngm_observed_fields;
int64_t ngm_target_observed_fields_workspace(int32_t height, int32_t width);
int ngm_target_observed_fields(const ngm_observed_fields* a, void* workspace, int64_t workspace_bytes, void* stream);

/* training_iterations[field_ids[i]] += 1 for i < min(rows, *count) (count == NULL: rows), skipping -1 (padding rows) and
 * ids outside [0, num_fields): the reference's `training_iterations[field_ids] += 1` (rm.py:1188) as one launch that a
 * captured iteration can hold.  field_ids duplicate-free, as the sampler's are. */
int ngm_field_counts_add(const int64_t* field_ids, const int32_t* count, int32_t rows, int64_t* training_iterations,
                         int32_t num_fields, void* stream);

/* ---- a map that grows under a live graph: reserved field rows (opt-in; additive to ABI 11) ------------------------------
 * Every per-field array (stacked parameters, their 16-bit copies, both Adam moments, positions, orientations,
 * training_iterations) is allocated once for max_fields rows, and the number of fields in force lives in device memory
 * (num_fields_dev, one int32).  Adding fields is then one launch that fills the next rows and raises that count
 * (ngm_fields_append); the sampler and the observed-field search read the count on the device (the *_grow entry points
 * below), so a graph captured over them keeps replaying while the map grows up to max_fields.
 *
 * ngm_fields_append: for rows [first, first + num_new) of every tensor of the table: param = prototype, the 16-bit copy =
 * the prototype rounded as ngm_adam_sparse_multi rounds an updated weight (round to nearest even; bit for bit what the
 * refresh from the fp32 masters gives), exp_avg = exp_avg_sq = 0 (either may be NULL); training_iterations (optional) = 0;
 * positions / orientations rows = new_positions / new_orientations; then *num_fields_dev = first + num_new.  One kernel on
 * `stream`, no host synchronisation: whatever runs next on that stream sees complete fields.  first + num_new <= max_fields
 * is checked on the host; rows outside [first, first + num_new) are not touched. */
#define NGM_APPEND_MAX_TENSORS 16
typedef struct ngm_append_tensor {
  float* param;                    /* (max_fields, numel) rows with `stride` elements between fields             */
  float* exp_avg;                  /* same layout, or NULL                                                       */
  float* exp_avg_sq;               /* same layout, or NULL                                                       */
  const float* prototype;          /* DEVICE (numel): the row every new field starts from                        */
  int64_t stride, numel;
  void* param_lp;                  /* optional 16-bit copy of `param` (same row layout), as in ngm_adam_tensor   */
  int32_t lp_dtype;                /* ngm_param_dtype of the copy                                                */
  int32_t reserved_;
} ngm_append_tensor;
typedef struct ngm_fields_append_args {
  const ngm_append_tensor* tensors; /* HOST array of num_tensors descriptors                                     */
  int32_t num_tensors;              /* 0 .. NGM_APPEND_MAX_TENSORS                                               */
  int32_t first, num_new;           /* rows [first, first + num_new)                                             */
  int32_t max_fields;               /* rows every array below and every tensor above is allocated for            */
  const float* new_positions;       /* DEVICE (num_new, 3)                                                       */
  const float* new_orientations;    /* DEVICE (num_new, 4)                                                       */
  float* positions;                 /* (max_fields, 3)                                                           */
  float* orientations;              /* (max_fields, 4)                                                           */
  int64_t* training_iterations;     /* (max_fields) or NULL                                                      */
  int32_t* num_fields_dev;          /* device (1): receives first + num_new                                      */
} ngm_fields_append_args;
int ngm_fields_append(const ngm_fields_append_args* a, void* stream);

/* ngm_target_sample_mv_live with the number of fields read from device memory as well: s->num_fields is the CAPACITY
 * max_fields (stride, grid, workspace, the maxima of num_random and capacity exactly as the live entry point derives them
 * from num_fields), the count in force is nf = clamp(*num_fields_dev, 0, max_fields), read block-uniformly by the draw
 * kernel.  On the device nc = clamp(*num_current, 0, min(max_current, nf)), n_obs = min(T / 2, nc), n_rand = max(min(T - n_obs,
 * nf - n_obs), 0): n_obs + n_rand = min(T, nf) <= the host-known row capacity min(min(T, max_fields), fields of this rank
 * among max_fields).  Every key is a function of the field id alone, so the result is bit for bit that of
 * ngm_target_sample_mv_live on a map of exactly nf fields (rows below *count; the arrays here may have more padding rows).
 * No id >= nf is ever emitted, which is why ngm_field_counts_add needs no twin: give it max_fields.
 * Precondition, as before: current_field_ids duplicate-free with ids in [0, nf). */
int64_t ngm_target_sample_mv_grow_workspace(int32_t max_frames, int32_t max_current, int32_t max_fields, int32_t capacity);
int ngm_target_sample_mv_grow(const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_live* live,
                              const int32_t* num_fields_dev, const ngm_target_out* out, void* workspace, int64_t workspace_bytes,
                              void* stream);
/* ngm_target_observed_fields with a->num_fields = max_fields (the length of current_field_ids, -1 past *current_count up to
 * there) and the fields tested bounded by clamp(*num_fields_dev, 0, max_fields). */
int64_t ngm_target_observed_fields_grow_workspace(int32_t height, int32_t width);
int ngm_target_observed_fields_grow(const ngm_observed_fields* a, const int32_t* num_fields_dev, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/* ---- fields anchored to keyframes: re-pose the map after a pose-graph update (opt-in; additive to ABI 11) ---------------
 * NeuralGraphMap._update_field_poses (rm.py:937-952): every field belongs to a keyframe (map_dict["kf_ids"]) and moves with
 * it.  anchor_slot[f] is the row of the two pose tables that field f follows; prev_poses holds the keyframe poses at the
 * last re-pose, new_poses the poses in force.  Per field f with anchor a, in fp32, the reference's two steps in its order
 * (rm.py:864-885, then :844-862; utils.transform_points / transform_quaternions, utils.py:270-286):
 *   W = inverse(prev[a])       affine, last row (0,0,0,1): 3x3 inverse by adjugate and determinant, no orthonormality assumed
 *   p_rel = W.R p + W.t        q_rel = quat(W.R) (x) q
 *   p'    = new[a].R p_rel + new[a].t        q' = quat(new[a].R) (x) q_rel
 * quat = pytorch3d's matrix_to_quaternion (the best-conditioned of its four candidates, so a rotation by pi is accurate;
 * real part >= 0), (x) = the raw Hamilton product: no standardisation, no normalisation -- a quaternion's norm scales the
 * field's frame here and is carried through unchanged up to rounding.
 * Deliberately stricter than the reference, which sends every field through inverse x forward at every update:
 *   - a field whose anchor's prev and new rows are BITWISE EQUAL is not touched: not one bit of its pose changes;
 *   - a field with anchor -1 (unanchored), an anchor outside [0, num_poses), or a non-finite entry in either row of its
 *     anchor is not touched (a lost pose must not poison the map); nor is a field whose result would be non-finite
 *     (a singular prev row);
 *   - rows at or beyond the field count in force are not touched: the count is num_fields, or with num_fields_dev
 *     clamp(*num_fields_dev, 0, num_fields), as in the *_grow entry points.
 * advance_prev != 0: prev_poses := new_poses after the re-pose, stream-ordered inside the same call (a second small launch:
 * the first still reads prev); rows of new_poses with a non-finite entry are not copied, so prev keeps the pose the fields
 * of that row still stand at.  One thread per field, the tables are read through the cache; no atomics, no host
 * synchronisation; the result is bitwise deterministic (every rank of a field-sharded run computes the same map with no
 * exchange).  NULL pointers and negative sizes give NGM_E_INVALID before anything is launched. */
typedef struct ngm_fields_repose_args {
  float* positions;                 /* (max_fields, 3), updated in place                                          */
  float* orientations;              /* (max_fields, 4) real-first quaternions, updated in place                   */
  const int32_t* anchor_slot;       /* (max_fields): row of the pose tables, -1 = unanchored                      */
  float* prev_poses;                /* DEVICE (num_poses, 4, 4) row-major: poses at the last re-pose              */
  const float* new_poses;           /* DEVICE (num_poses, 4, 4) row-major: poses in force                         */
  const int32_t* num_fields_dev;    /* device (1) or NULL                                                         */
  int32_t num_fields;               /* rows processed (the capacity max_fields when num_fields_dev is given)      */
  int32_t num_poses;
  int32_t advance_prev;
  int32_t reserved0;
} ngm_fields_repose_args;
int ngm_fields_repose(const ngm_fields_repose_args* a, void* stream);

/* Device part of NeuralGraphMap._sample_target_sv (rm.py:1461-1583), the single-view variant (`update_mode: single_view`):
 * hit (F,N) u8 = the segment camera origin -> point n of the (subsampled) back-projected depth image passes through the
 * sphere of field f (geometry.py:67-105); field centres and points in the camera frame. */
int ngm_target_sv_intersect(int32_t F, int64_t N, const float* field_pos_cam, const float* points_cam, float radius,
                            uint8_t* hit, void* stream);
/* rm.py:1536-1561: segments (F,R) i64 = sampled point indices, pts_ijs (N,2) i64 their pixels, image (H,W,4) the RGB-D
 * frame; near / far are not clamped at 0 in this variant, rgb_mask = depth_mask = (gt < far), term_mask = 1, out->c2ws
 * is not written (one pose for all rays). */
int ngm_target_sv_rays(int32_t F, int32_t R, const float* field_pos_cam, float radius, const int64_t* pts_ijs,
                       const int64_t* segments, const float* image, int32_t height, int32_t width, float fx, float fy, float cx,
                       float cy, const ngm_target_out* out, void* stream);

/* ---- single-view training-target sampler, whole, on the device (opt-in; additive to ABI 11) -----------------------------
 * _sample_target_sv (rm.py:1461-1583) with every draw made on the device from Philox4x32-10 (NOT torch's stream): no host
 * synchronisation, fixed output capacity, no data-dependent shape, the number of rows left in device memory -- so a captured
 * graph draws fresh single-view targets at every replay, and the counted step takes `out` as it takes ngm_target_sample_mv's.
 * In the reference's order (Philox offset = iteration throughout):
 *   1. points: num_points pixels uniformly without replacement among those with depth != 0: key_p = (word 0 of block
 *      ctr = linear pixel p, stream 0x54470007) << 32 | p, the num_points smallest keys (the radix select of
 *      ngm_target_observed_fields: the SET is deterministic, the order of `pixels` is not, and nothing below depends on it).
 *      Fewer valid pixels than num_points: all of them (the reference's multinomial would raise); none: *count = 0.
 *      Back-projection (camera.py:374-390, OpenGL): x = ((col - cx) * d) / fx, y = ((-(row - cy)) * d) / fy, z = -d; the
 *      points' AABB is their exact min / max.
 *   2. candidates: per entry of active_field_ids the centre in the camera frame (R^T (p - t), products summed left to
 *      right), the sphere AABB against the points' AABB (geometry.py:26-42), then hits = the number of points whose segment
 *      origin -> point crosses the sphere (ngm_target_sv_intersect's arithmetic; integer counts, no hit matrix in memory).
 *      A field is a candidate when it is in the box and hits >= num_rays.  Entries < 0 or >= the field count in force are
 *      skipped (hits 0), so a fixed-length list padded with -1 works; the other entries must be duplicate-free.
 *   3. fields: at most T = num_train_fields candidates: all of them in the order of active_field_ids -- else the T smallest
 *      of key_g = (word 0 of block ctr = field id g, stream 0x54470008) << 32 | g, in key order.  subset_fields = their
 *      positions in the candidate list (0, 1, ... when no draw was needed), -1 past them.
 *      Sharding (world_size W, rank r): every rank makes the same draw; rows are made only for drawn fields with
 *      g % W == r, in draw order.  capacity >= min(T, num_active, #{id in [0, num_fields): id % W == r}) is required.
 *   4. rays: per row, num_rays of the field's hit points uniformly without replacement: for the hit point at pixel p
 *      key = (word 0 of block ctr = (g << 32 | p), stream 0x54470009) << 32 | p, the num_rays smallest, ray k = the k-th
 *      smallest.  A row depends on (seed, iteration, frame, g) only: not on its index, the rank or the other fields.
 *   5. targets: ngm_target_sv_rays' arithmetic per ray (near / far not clamped, rgb_mask = depth_mask = gt < far,
 *      term_mask = 1); out->c2ws (when given) receives the frame's pose in every ray slot.
 *   6. rows past *count: field_ids = -1, masks 0, zeros elsewhere (segments -1).
 * Frame stack: num_slots >= 1 frames in rgbd (num_slots,H,W,4) / c2w (num_slots,4,4); the frame read is
 * clamp(*slot_dev, 0, num_slots - 1), slot 0 when slot_dev is NULL.  num_fields_dev (or NULL): the count in force is
 * clamp(*num_fields_dev, 0, num_fields), as in the *_grow entry points.  iteration >= 0: this iteration; < 0: *iteration_dev
 * is read, and advanced by one by the last kernel, after every read of it.
 * Replay of recorded draws (world_size 1): pixels_in (num_points linear pixel indices, used in the given order, entries
 * outside [0, H*W) unused) replaces draw 1; subset_fields_in (T positions in the candidate list) replaces draw 3 when there
 * are more than T candidates; segments_in (capacity, num_rays) indices into pixels_in replaces draw 4 (needs pixels_in).
 * 1 <= num_points <= NGM_SV_MAX_POINTS, num_train_fields and num_rays <= NGM_TARGET_MAX_DRAW, H*W < 2^31.
 * `hits` of a field outside the points' box is 0: its segments are not tested, as in the reference.
 * No float atomics; bitwise repeatable from call to call.  15 launches (6 with pixels_in).
 * Workspace: 8 bytes per pixel of the frame (the pixel keys) + 16 bytes per point + 28 bytes per active entry + the ray keys,
 * capacity x num_points x 8 bytes -- 12.8 MB at 32 rows x 50 000 points, but 1 GiB at the largest sizes this entry point
 * accepts (2048 rows x 65 536 points): a caller with a large num_train_fields should size num_points with that in mind and
 * keep the workspace between calls. */
#define NGM_SV_MAX_POINTS 65536
typedef struct ngm_target_sample_sv_args {
  const float* rgbd;                /* (num_slots,H,W,4) frames [r,g,b,depth]                              */
  const float* c2w;                 /* DEVICE (num_slots,4,4) row-major camera poses, read at run time     */
  const int32_t* slot_dev;          /* device (1) or NULL                                                  */
  const int64_t* active_field_ids;  /* (num_active)                                                        */
  const float* field_positions;     /* (>= num_fields, 3)                                                  */
  const int32_t* num_fields_dev;    /* device (1) or NULL                                                  */
  int32_t num_slots, height, width;
  int32_t num_active, num_fields;
  int32_t num_points, num_train_fields, num_rays, capacity;
  int32_t world_size, rank;
  int32_t reserved0;
  float fx, fy, cx, cy;             /* intrinsics at pixel centre 0                                        */
  float radius;                     /* _field_radius                                                       */
  int32_t reserved1;
  uint64_t seed;
  int64_t iteration;
  int64_t* iteration_dev;
  const int64_t* pixels_in;         /* (num_points) or NULL                                                */
  const int64_t* subset_fields_in;  /* (num_train_fields) or NULL                                          */
  const int64_t* segments_in;       /* (capacity,num_rays) or NULL                                         */
  int64_t* field_ids;               /* out (capacity)                                                      */
  int32_t* count;                   /* out (1): rows                                                       */
  int64_t* pixels;                  /* out (num_points): chosen linear pixel indices, -1 past *num_used    */
  int32_t* num_used;                /* out (1): valid chosen pixels                                        */
  int32_t* hits;                    /* out (num_active): crossing segments per entry, 0 for skipped ones   */
  int32_t* num_candidates;          /* out (1)                                                             */
  int64_t* subset_fields;           /* out (num_train_fields): positions in the candidate list, -1 padded  */
  int64_t* segments;                /* out (capacity,num_rays): the chosen points as linear pixel indices  */
} ngm_target_sample_sv_args;
int64_t ngm_target_sample_sv_workspace(int32_t height, int32_t width, int32_t num_active, int32_t num_points, int32_t capacity);
int ngm_target_sample_sv(const ngm_target_sample_sv_args* a, const ngm_target_out* out, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* ---- mesh extraction -------------------------------------------------------------------
 * Marching cubes on a dense grid of field values: replaces the pytorch3d.ops.marching_cubes call of
 * NeuralGraphMap._extract_mesh (rm.py:2255-2298; the grid itself is filled by ngm_field_eval_knn, rm.py:2255-2261).
 * volume (nx,ny,nz) fp32 row-major (z fastest), "inside" = value > isolevel (the caller negates nrgbd / neus volumes,
 * rm.py:2277-2289).  Two passes over the same volume / workspace:
 *   _count: classifies edges and cells, scans; counts (device int64[2]) = number of vertices, number of faces;
 *   _emit : verts (V,3) fp32 in GRID-INDEX coordinates (x in [0,nx-1], ...; the caller maps them to world
 *           coordinates as rm.py:2304-2317 does), faces (T,3) int64 vertex indices, outward normals
 *           (inside -> outside).  Entries beyond max_verts / max_faces are dropped.
 * Output order is deterministic: vertices by (grid point ((x*ny)+y)*nz+z, axis x<y<z) of the crossed edge's lower end,
 * faces by cell index ((x*(ny-1))+y)*(nz-1)+z.  One vertex per crossed edge (indexed, watertight mesh).
 * PARITY UNPINNED against pytorch3d (un-vendored): the triangulation table is derived from the cube topology
 * (oracle/mesh_oracle.py restates it); vertex positions are the same linear interpolation.
 * ngm_marching_cubes_tables copies the derived table (host call, no device): tri_table[256*15] edge ids (-1 padded),
 * tri_count[256]. */
int64_t ngm_marching_cubes_workspace(int32_t nx, int32_t ny, int32_t nz);
int ngm_marching_cubes_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float isolevel,
                             int64_t* counts, void* workspace, int64_t workspace_bytes, void* stream);
int ngm_marching_cubes_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float isolevel, float* verts,
                            int64_t max_verts, int64_t* faces, int64_t max_faces, void* workspace,
                            int64_t workspace_bytes, void* stream);
int ngm_marching_cubes_tables(int8_t* tri_table, int32_t* tri_count);

/* ---- scoring a mesh: surface samples and exact nearest points (additive to ABI 11) --------------------------------------
 * The device parts of evaluation._evaluate_postprocessed_meshes (evaluation.py:163-208): the two
 * trimesh.sample.sample_surface calls (evaluation.py:190-191) and the scipy.spatial.KDTree build + query behind every one
 * of the ten numbers (evaluation.py:75-130).  Culling and the subdivision before it are the next two blocks', ICP alignment the one after them.
 * ngm_surface_sample: verts (V,3) fp32, faces (F,3) int64 -> points (N,3) fp32, face_ids (N) int64.  trimesh's sampler
 * restated from its public definition: a face with probability proportional to its area (fp32 area, fp64 inclusive scan,
 * binary search for the first cum[k] > u * total), then the point v0 + u (v1 - v0) + v (v2 - v0) with (u, v) reflected to
 * (1 - u, 1 - v) where u + v > 1.  Sample i draws Philox block i of a stream of its own under `seed`: words 0 and 1 form the
 * 53-bit face draw, words 2 and 3 the 24-bit u and v; the result is a function of (mesh, seed, i) alone.  A face with a
 * non-finite vertex or an index outside [0, V) has area 0, and a face of area 0 is never returned.  Nothing is read back:
 * when the total area is not > 0 every point is NaN and every face id -1.
 * ngm_nearest_point: refs (M,3), queries (N,3) fp32 -> dist (N) fp32, index (N) int64: the EXACT nearest reference of
 * every query (a uniform grid over the references built per call on the device, searched ring by ring until the best
 * distance found is provably the smallest), dist = sqrtf(dx*dx + dy*dy + dz*dz) of fp32 differences; equal distances may
 * go to any of the tied indices.  A non-finite reference is nobody's neighbour; a non-finite query gets dist NaN, index -1;
 * with no finite reference every dist is +inf and every index -1.  Queries need no order.
 * Both: the caller owns the workspace (the *_workspace functions: bytes, or NGM_E_INVALID for sizes the calls refuse);
 * no host synchronisation.  NGM_E_INVALID before anything is launched for a NULL array, a negative count, num_faces == 0,
 * num_refs == 0, a count >= 2^31 or a workspace that is too small; num_samples == 0 / num_queries == 0 return NGM_OK and
 * launch nothing (the outputs may be NULL then). */
int64_t ngm_surface_sample_workspace(int64_t num_faces);
int ngm_surface_sample(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, int64_t num_samples,
                       uint64_t seed, float* points, int64_t* face_ids, void* workspace, int64_t workspace_bytes, void* stream);
int64_t ngm_nearest_point_workspace(int64_t num_refs, int64_t num_queries);
int ngm_nearest_point(const float* refs, int64_t num_refs, const float* queries, int64_t num_queries, float* dist,
                      int64_t* index, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- culling a mesh: depth rasteriser and per-vertex visibility (additive to ABI 11) -----------------------------------
 * The device parts of mesh_culling._cull_mesh (mesh_culling.py:228-352), the step evaluation.evaluate_raw_mesh
 * (evaluation.py:211-251) runs on both meshes before it scores them.
 * ngm_mesh_depth: verts (V,3) fp32, faces (F,3) int64, c2w (P,4,4) fp32 row-major camera-to-world in the OpenGL convention
 * (what _cull_mesh hands on), intrinsics with cx, cy in the 0.5-pixel-centre convention
 * (Camera.get_pinhole_camera_parameters(0.5)) -> depth (P,H,W) fp32: the camera-space z of the nearest surface, 0.0 where
 * nothing is hit.  THE RULE (the contract; tests/_mesh_cull_host.py restates it in fp64):
 *   - columns 1 and 2 of the pose's rotation are negated (mesh_culling.py:164-167), the affine part is inverted by adjugate
 *     and determinant (no orthonormality assumed; the last row is taken as 0 0 0 1), the three corners go to camera space;
 *   - the triangle is clipped against z >= near: 0, 3 or 4 corners, hence at most two triangles (0 1 2 and 0 2 3; a crossing
 *     is formed from the corner in front towards the one behind and has z = near);
 *   - projection sx = fx X / Z + cx, sy = fy Y / Z + cy; pixel (u, v) is sampled at (u + 0.5, v + 0.5) and is covered when
 *     the sample lies inside or ON the triangle, in either winding -- the reference's two renders with flipped winding,
 *     merged by minimum (mesh_culling.py:102-120);
 *   - the depth at the sample is the perspective-correct camera z (1 / z interpolated linearly on the screen); samples with
 *     z > far are rejected; the stored value is the minimum over all faces.
 * Skipped, as the surface sampler skips them: a face with an index outside [0, V), with a non-finite vertex, or with zero
 * projected area (each of the two clipped triangles on its own; also one whose projection is not finite in fp32).  A pose
 * with a non-finite entry gives an all-zero map.  Not reproduced: GL's top-left fill rule and the quantisation of its depth
 * buffer, both far inside the eps = 0.03 the maps are compared with.
 * The minimum is an integer atomic on the bit pattern of the positive float: independent of the order of the faces, so the
 * map is bitwise deterministic.  A lane draws its own triangle when its bounding box holds at most 32 pixels; larger ones
 * are drawn one at a time by all 64 lanes of the wave; a mesh of few faces is drawn in bands of rows, so that many
 * workgroups share its screen-filling triangles.  No workspace.
 * ngm_mesh_visibility: _cull_from_one_pose for all P poses of the call plus the accumulation of _apply_culling_strategy
 * (mesh_culling.py:143-225).  ADDS into in_frustum (V) and observed (V) int32 (the caller zeroes them; calls over chunks
 * of the poses add up to one call over all of them).  Per (vertex, pose), in fp32: camera space as above, uvz = K camera
 * space, pz = z + 1e-8, px = u / pz, py = v / pz; inside = 0 <= px <= width - 1 and 0 <= py <= height - 1 (the reference's
 * bound, kept) and pz > 0; the pixel is (clamp, then truncate) of (px, py); seen = inside and pz < depth[pose, v, u] + eps.
 * inside counts into in_frustum for poses [0, num_frustum_poses) only (virtual cameras, mesh_culling.py:220-223), seen into
 * observed for all.  depth == NULL: seen = inside (the frustum-only method).  One thread per vertex, no atomics.
 * Both: no host synchronisation.  NGM_E_INVALID before anything is launched for a NULL array, a negative count, a count
 * >= 2^31, width or height < 1, and (ngm_mesh_depth) near <= 0 or far <= near.  num_poses == 0 or num_verts == 0 return
 * NGM_OK and launch nothing (ngm_mesh_depth then leaves `depth` untouched); num_faces == 0 gives all-zero maps. */
int ngm_mesh_depth(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, const float* c2w, int64_t num_poses,
                   int32_t width, int32_t height, float fx, float fy, float cx, float cy, float near, float far, float* depth,
                   void* stream);
int ngm_mesh_visibility(const float* verts, int64_t num_verts, const float* c2w, int64_t num_poses, int32_t width, int32_t height,
                        float fx, float fy, float cx, float cy, const float* depth, float eps, int64_t num_frustum_poses,
                        int32_t* in_frustum, int32_t* observed, void* stream);

/* ---- subdividing a mesh to a maximum edge length (additive to ABI 11) ----------------------------------------------------
 * The first step of mesh_culling._cull_mesh (mesh_culling.py:260-261): trimesh's subdivide_to_size, which splits every face
 * with an edge longer than max_edge into four by its edge midpoints and repeats on the children.  The children are similar to
 * the parent at half its size, so they share its fate in every round and the result per INPUT face is closed-form: the face
 * becomes the uniform split into 4^k children, n = 2^k segments per edge, k its LEVEL.  Two calls, like marching cubes:
 * ngm_mesh_subdivide_count: verts (V,3) fp32, faces (F,3) int64 -> totals_dev, three int64 on the device: the number of new
 *   vertices, the number of output faces, the largest level.  THE LEVEL: the three edge lengths in fp64 from the fp32
 *   vertices, sqrt((dx*dx + dy*dy) + dz*dz), no fused multiply-add (what numpy computes on a float64 copy of the vertices);
 *   L = the longest; k = the number of exact halvings of L until `L > max_edge` is false.  An edge equal to max_edge is not
 *   split.  A NaN length makes L NaN, which compares false: level 0.  A +inf length never passes; it, and every length that
 *   needs more than max_iter halvings, gets level max_iter + 1, which the caller reads from totals_dev[2] and refuses -- such
 *   a face counts one output face and no new vertex, so the totals stay bounded.  A face with an index outside [0, V) has
 *   level 0 and is never dereferenced.  A face that needs exactly max_iter halvings is accepted.
 *   The workspace (ngm_mesh_subdivide_workspace(F) bytes) holds, from its first 256-byte boundary on: level (F) int32, then
 *   -- each rounded up to 256 bytes -- the exclusive int64 scans (F + 1) of the new vertices and of the output faces per face.
 * ngm_mesh_subdivide_emit: the same mesh and workspace, the two totals as the host read them, attrs (V,C) fp32 or NULL ->
 *   out_verts (V + new_vertices, 3) fp32: the V originals unchanged in [0, V), then per split face, in face order, its
 *     lattice points that are not corners.  Lattice point (i, j), i + j <= n, of face (a, b, c) is a w0 + b w1 + c w2 with
 *     w = ((n - i - j) / n, i / n, j / n); the points of a face are numbered row by row, j = 0 .. n, i = 0 .. n - j, the
 *     three corners (0, 0), (n, 0), (0, n) left out.  Every face that is split stores its own points: a point on an edge
 *     two faces share is stored by both, under two indices;
 *   out_faces_idx (out_faces, 3) int64: children in parent order; inside a parent row by row, j = 0 .. n - 1, in row j the
 *     2 (n - j) - 1 children u = 0, 1, ..: for even u, i = u / 2, the upright ((i, j), (i + 1, j), (i, j + 1)), for odd u the
 *     inverted ((i + 1, j), (i + 1, j + 1), (i, j + 1)).  Every child has the parent's winding; a corner of a child that is a
 *     corner of the parent keeps the original index; a level-0 face is copied as it is, whatever its indices;
 *   out_parent (out_faces) int64: the input face of every output face (trimesh's return_index);
 *   out_attrs (V + new_vertices, C) fp32: attrs interpolated with the same weights (attrs NULL: not written).
 *   EXACTNESS: a point is evaluated in fp64 and rounded once to fp32, and a term whose weight is 0 is left out of the sum.
 *   The weights are multiples of 2^-10 (max_iter <= 10) and the inputs have 24 bits, so every product is exact in fp64.  On
 *   an edge of the parent one weight is 0: the point is ONE fp64 rounding of the exact sum of two products that depend on
 *   the edge's two end points and the position along it alone, then one rounding to fp32.  It is therefore bit-identical
 *   from both faces that share the edge, whatever their levels, the order of their indices or FMA contraction (a contracted
 *   sum of an exact product is the same single rounding) -- the rasteriser's occlusion test relies on it: cracks along shared
 *   edges would let depth leak through.
 *   One thread per output element finds its parent by binary search in the scans (the first and the last thread of a workgroup
 *   over all faces, the others between those two) and its lattice coordinates by a row formula with an integer fix-up; no
 *   thread loops over the children of a face.
 * Both: no host synchronisation.  NGM_E_INVALID before anything is launched for a NULL array, a negative count, V or F >= 2^31,
 * max_edge not finite or not > 0, max_iter outside [0, 10], a workspace that is too small; NGM_E_UNSUPPORTED (emit) when
 * V + new_vertices, out_faces or C (V + new_vertices) reach 2^31.  F == 0: the totals are zero, nothing else is launched. */
int64_t ngm_mesh_subdivide_workspace(int64_t num_faces);
int ngm_mesh_subdivide_count(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, double max_edge,
                             int32_t max_iter, void* workspace, int64_t workspace_bytes, int64_t* totals_dev, void* stream);
int ngm_mesh_subdivide_emit(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, const float* attrs,
                            int32_t num_channels, const void* workspace, int64_t new_vertices, int64_t out_faces, float* out_verts,
                            int64_t* out_faces_idx, float* out_attrs, int64_t* out_parent, void* stream);

/* ---- aligning a mesh to the ground truth: vertex normals and point-to-plane ICP (additive to ABI 11) ---------------------
 * evaluation._align_mesh (evaluation.py:133-160), the step evaluation.evaluate_raw_mesh runs between culling the ground truth
 * and culling the estimate: Open3D's registration_icp from the estimate's vertices to the culled ground truth's vertices and
 * vertex normals, threshold 0.1, identity start, TransformationEstimationPointToPlane, at most 100 iterations.
 * PARITY UNPINNED against Open3D (not installed here): both entry points are restated from Open3D's public definitions, and
 * the yardstick is the fp64 host mirror tests/_mesh_align_host.py, written to the rules below.
 * ngm_mesh_vertex_normals: verts (V,3) fp32, faces (F,3) int64 -> normals (V,3) fp32, Open3D's compute_vertex_normals: every
 *   face adds its unnormalised normal (v1 - v0) x (v2 - v0) (fp64 from the fp32 vertices: area weighting) to its three vertices,
 *   the sum is normalised in fp64 and rounded to fp32.  A vertex whose sum has length 0 (no face refers to it, or exact
 *   cancellation) gets (0, 0, 1); so does a vertex with a non-finite coordinate.  A face with an index outside [0, V) or a
 *   non-finite vertex adds nothing.  The sums are int64 fixed-point sums at a per-vertex scale (the largest exponent among the
 *   vertex's incident normals and its valence, found by a first pass, make 2^62 the bound of the sum): integer addition is
 *   associative, so the result does not depend on the order of the faces and is bitwise equal from call to call; the
 *   fixed-point rounding is below 2^-40 of the largest term.  One atomic per (face, corner, component) and pass; no thread
 *   loops over the faces of a vertex.
 * ngm_icp_point_to_plane: source (N,3), target (M,3), target_normals (M,3) fp32; init: 16 doubles, row-major, on the HOST
 *   (read before the call returns; NULL = identity; its last row is taken as 0 0 0 1); state: 64 doubles on the DEVICE.
 *   Pass k = 0 .. max_iteration works at the current transformation T_k (fp64, in `state`):
 *   - p = R s + t in fp64, ((R0 sx + R1 sy) + R2 sz) + t per row, no fused multiply-add; the search runs from (float)p on a
 *     uniform grid over the finite target points, built ONCE per call, ring by ring as ngm_nearest_point does, with fp32
 *     distances; EQUAL DISTANCES GO TO THE SMALLEST TARGET INDEX; the search stops where no unseen point can be within
 *     `threshold` (plus rounding slack) of p;
 *   - the found target q is a correspondence iff d = sqrt((dx dx + dy dy) + dz dz) < threshold, in fp64 from the fp64 p;
 *   - a non-finite source point (or p), a call without a finite target, and a correspondence whose normal n is not finite take no part;
 *   - with r = (p - q) . n and J = [p x n, n]: the 21 upper entries of J^T J (row by row), the 6 of J^T r, sum d^2 and the
 *     count are summed in fp64: per thread over a grid-stride loop of a fixed grid, per wave, per workgroup, then over the
 *     workgroups' rows, every step in a fixed order -- bitwise equal from call to call;
 *   - fitness_k = count / N (the denominator is always N), rmse_k = sqrt(sum d^2 / count), 0 without correspondences;
 *   - k >= 1 and |fitness_k - fitness_{k-1}| < relative_fitness and |rmse_k - rmse_{k-1}| < relative_rmse: converged, stop at T_k;
 *     else k == max_iteration: stop, not converged; else J^T J x = -J^T r by Cholesky in fp64,
 *     U = Rz(x2) Ry(x1) Rx(x0) with translation (x3, x4, x5), T_{k+1} = U T_k.
 *   - No correspondence gives the identity update.  SINGULAR SYSTEMS (OUR RULE -- Open3D's LDLT has no check): a Cholesky pivot
 *     that is not above 1e-12 x the largest diagonal entry of J^T J, or a solution that is not finite, gives the identity update
 *     (a planar target leaves three columns of J^T J exactly zero; the next pass then converges at the unchanged T).
 *   All max_iteration + 1 passes (two launches each) are enqueued at once; a `done` flag in `state` turns the launches after
 *   the stop into immediate exits.  No host synchronisation: the call can be captured in a graph (init is read at capture).
 *   state: [0, 16) T row-major; [16] fitness; [17] inlier rmse; [18] iterations = the k it stopped at = updates applied; [19]
 *   converged (0 / 1); [20, 49) the last pass's sums -- J^T J upper (21), J^T r (6), sum d^2, count (with max_iteration = 0:
 *   the sums at init); [49] done (internal); [50, 64) zero.
 * Both: the caller owns the workspace (the *_workspace functions: bytes, or NGM_E_INVALID for sizes the calls refuse; stale
 * contents are never read).  NGM_E_INVALID before anything is launched for a NULL array, a negative count, a count >= 2^31, a
 * workspace that is too small, and (ICP) M == 0, a threshold that is not finite or not > 0, max_iteration outside [0, 1000].
 * V == 0 launches nothing; N == 0 writes state (T = init, fitness 0, converged 0) and returns NGM_OK. */
int64_t ngm_mesh_vertex_normals_workspace(int64_t num_verts);
int ngm_mesh_vertex_normals(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, float* normals,
                            void* workspace, int64_t workspace_bytes, void* stream);
int64_t ngm_icp_point_to_plane_workspace(int64_t num_target, int64_t num_source);
int ngm_icp_point_to_plane(const float* source, int64_t num_source, const float* target, const float* target_normals,
                           int64_t num_target, double threshold, int32_t max_iteration, double relative_fitness,
                           double relative_rmse, const double* init, double* state, void* workspace, int64_t workspace_bytes,
                           void* stream);

/* ---- scoring rendered frames: PSNR, SSIM and depth L1 in fp64 (additive to ABI 11) ---------------------------------------
 * The per-frame render metrics of NeuralGraphMap._evaluate_frame (run_mapping.py:1977-2020): evaluation.psnr, evaluation.ssim
 * and evaluation.depthl1 (evaluation.py:20-30, 46-62) over a batch of frames in one call.  LPIPS is not built (its network
 * weights are not part of this project).
 * PARITY UNPINNED against torchmetrics (not installed here): the definitions below restate its public algorithm
 * (structural_similarity_index_measure and peak_signal_noise_ratio with data_range = 1.0 and their defaults), evaluated in
 * fp64 where torchmetrics works in fp32; the yardstick is the fp64 host mirror tests/_image_metrics_host.py.
 * pred, target: (batch, height, width, 4) fp32, contiguous, 16-byte aligned, r g b depth interleaved (what render_image returns
 * and a keyframe holds).  crop is the reference's eval_crop.  EVERY OPERATION AFTER THE LOAD IS IN fp64; "clamped" keeps NaN as
 * torch.clamp does (v < 0 ? 0 : v > 1 ? 1 : v).  Per frame:
 * - depth L1 over the WHOLE image (the reference's depthl1 takes crop and never uses it): a pixel takes part iff
 *   target depth != 0 (a NaN target depth takes part, -0.0 does not); depth_l1 = sum |pred - target| / count, NaN without one.
 * - PSNR over the region R = rows and columns crop .. size - crop - 1: x = clamped pred rgb, y = clamped target rgb,
 *   mse = sum (x - y)^2 / (3 |R|), psnr = 10 log10(1 / mse): +inf where mse == 0, NaN where R is empty (2 crop >= height or width).
 * - SSIM: weights g_i proportional to exp(-((i - 5) / 1.5)^2 / 2), i = 0..10, normalised to sum 1 in fp64 on the host; the 2-D
 *   weights are g_i g_j.  For every channel and every 11 x 11 window that lies wholly inside R the five weighted sums mu_x, mu_y,
 *   E[xx], E[yy], E[xy] (separable: 11 taps along the row, then 11 down the column, each sum = fma(g, value, sum) from 0);
 *   var_x = max(E[xx] - mu_x^2, 0), likewise var_y (NaN kept), cov = E[xy] - mu_x mu_y; c1 = 1e-4, c2 = 9e-4;
 *   s = ((2 mu_x mu_y + c1)(2 cov + c2)) / ((mu_x^2 + mu_y^2 + c1)(var_x + var_y + c2)), formed without fused multiply-add:
 *   identical finite images with var > 0 give exactly 1.0 per window.  ssim = mean of s over the 3 (h - 10)(w - 10) windows, h, w
 *   the sides of R.  OUR RULE: fewer than 11 rows or columns in R gives NaN (torchmetrics fails or returns an empty mean
 *   there).  torchmetrics pads by reflection and cuts the padded border off again, which equals the valid windows: no padding.
 * out: (batch, 8) doubles on the device: [0] psnr, [1] ssim, [2] depth_l1, [3] mse, [4] colour terms 3 |R|, [5] SSIM windows,
 *   [6] depth pixels, [7] 0.
 * At most three launches (pixel sums, SSIM tiles with their 5-pixel halo staged in LDS, a closing kernel), no host
 * synchronisation, capturable in a graph.  No floating-point atomics: per-wave, then per-workgroup sums land as rows in the
 * caller's workspace and are added in a fixed order, so two calls on the same inputs agree bit for bit, and frame b of a batch
 * equals the same frame scored alone (a frame's grid depends on height, width and crop only).
 * ngm_image_metrics_workspace: bytes, or NGM_E_INVALID for what the call refuses; stale contents are never read.
 * NGM_E_INVALID before anything is launched for a NULL or misaligned array, batch, height, width or crop < 0,
 * batch * height * width >= 2^31, and a workspace that is too small.  batch == 0 launches nothing and returns NGM_OK;
 * height * width == 0 reads no pixel: only the closing kernel runs and writes every row as NaN with zero counts. */
int64_t ngm_image_metrics_workspace(int32_t batch, int32_t height, int32_t width, int32_t crop);
int ngm_image_metrics(const float* pred, const float* target, int32_t batch, int32_t height, int32_t width, int32_t crop,
                      double* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- covering a keyframe's depth with new fields (additive to ABI 11) ------------------------------------------------------
 * NeuralGraphMap._extend_global_map_dict (run_mapping.py:265-345) up to the positions of the new fields: where do new fields
 * go so that every back-projected pixel of a keyframe lies inside one?  fp32, operations in the reference's order.
 * - pixel (i, j) is valid iff its depth d = depth[(i width + j) pixel_stride] is finite and != 0 (camera.py:374; OUR RULE: a
 *   non-finite depth is skipped, the reference would carry NaN on);
 * - camera point (OpenGL frame, pixel centre 0): x = (j - cx) d / fx, y = -(i - cy) d / fy, z = -d (camera.py:382-384); world
 *   point p = R (x y z) + t of c2w, row r as ((R_r0 x + R_r1 y) + R_r2 z) + t_r without fused multiply-add (utils.py:283-286;
 *   the reference's einsum does not define its order).  OUR RULE: a pixel whose p is non-finite (a lost pose) is skipped;
 * - p is covered iff an ACTIVE field centre c has |p - c|^2 < radius^2, strictly, both sides in fp32, the squares added x, y, z
 *   (pytorch3d's ball_query with K = 1, restated from its public definition).  Active fields: rows 0 .. num_active - 1 of
 *   field_positions, or with field_ids the rows it names; entries < 0 or >= rows are skipped (padded lists pass as they are);
 * - the cell of a point v is floor((v + shift) / cell) per axis, IEEE division; `cell` is (float)(2 radius / sqrt 3) formed in
 *   double by the caller.  A cell is WANTED when an uncovered valid pixel falls into it, OCCUPIED when an active centre does
 *   (whether or not that field covers anything there, rm.py:303-311); the new cells are wanted and not occupied;
 * - new_positions rows 0 .. num_new - 1 = ((ijk - shift) + 0.5) cell (rm.py:325), the cells in ascending lexicographic
 *   (i, j, k) order, the order torch.unique(dim=0) gives the reference.
 * counts (4) int32 = {num_new, status, uncovered valid pixels, valid pixels}.  status 0: rows 0 .. num_new - 1 written, rows
 * past them untouched.  status 1: more than max_new new cells; num_new holds the number needed and NO row is written.
 * status 2: an uncovered valid pixel's cell index is outside (-2^20, 2^20) on some axis (or shift is not finite): num_new is 0
 * and no row is written.  The call returns NGM_OK in all three cases: the status lives on the device.
 * The set of cells is exact and the output bitwise identical from call to call: integer atomics only, nothing depends on the
 * order of arrival.  One memset and five launches on `stream`, no host synchronisation, capturable in a graph.
 * NGM_E_INVALID before anything is launched for a NULL argument or array (field_positions may be NULL iff num_active == 0),
 * height, width < 1 or height * width >= 2^31, pixel_stride < 1, rows or num_active < 0, num_active > rows without field_ids,
 * radius or cell not finite or <= 0, max_new < 1; NGM_E_UNSUPPORTED for max_new > NGM_COVER_MAX_NEW (every new field's rank is
 * found by counting the keys below its own: quadratic in num_new, 2^32 comparisons at the limit); NGM_E_WORKSPACE for a
 * workspace below ngm_cover_depth_workspace (bytes; the same refusals as negative codes); stale contents are never read. */
#define NGM_COVER_MAX_NEW 65536
typedef struct ngm_cover_depth_args {
  const float* depth;               /* (height, width) pixels, pixel_stride floats apart                           */
  const float* c2w;                 /* DEVICE (4, 4) row-major camera-to-world pose; the first three rows are read */
  const float* shift;               /* DEVICE (3): the grid's shift, drawn from [0, cell) by the caller            */
  const float* field_positions;     /* (rows, 3) field centres; NULL with num_active == 0                          */
  const int64_t* field_ids;         /* (num_active) rows of the active fields, or NULL: rows 0 .. num_active - 1   */
  float* new_positions;             /* (max_new, 3)                                                                */
  int32_t* counts;                  /* (4)                                                                         */
  int32_t pixel_stride;             /* 1: a depth image; 4: the depth channel of an (H, W, 4) RGB-D image          */
  int32_t rows, num_active;
  int32_t height, width;
  int32_t max_new;
  float fx, fy, cx, cy;
  float radius, cell;
} ngm_cover_depth_args;
int64_t ngm_cover_depth_workspace(int32_t height, int32_t width, int32_t num_active, int32_t max_new);
int ngm_cover_depth(const ngm_cover_depth_args* a, void* workspace, int64_t workspace_bytes, void* stream);
/* Measurement only: copies the five device counters of the LAST call on this workspace to out5 (host) after synchronising
 * `stream`: new cells before the max_new cut, range flag, uncovered valid pixels, valid pixels, insertions into the global set. */
int ngm_cover_depth_counters(int32_t height, int32_t width, int32_t num_active, int32_t max_new, void* workspace, int32_t* out5,
                             void* stream);

/* ---- measurement hooks (bench.py roofline leg) ------------------------------------------------
 * When enabled, every launch of the listed kernels is bracketed by hipEvents recorded on the launch
 * stream; ngm_profile_read() synchronises them and returns the accumulated device time. */
enum ngm_kernel_id {
  NGM_K_RENDER_FWD = 0, /* fused forward (sampler+encode+MLP+composite)                 */
  NGM_K_STASH_BWD = 1,  /* compositing + loss backward on the stash                      */
  NGM_K_FIELD_BWD = 2,  /* MFMA backward of encoding + MLP (dominant kernel)             */
  NGM_K_GRAD_REDUCE = 3,
  NGM_K_ADAM = 4,
  NGM_K_POINTS_FWD = 5,
  NGM_K_COMPOSITE_FWD = 6,
  NGM_K_COMPOSITE_BWD = 7,
  NGM_K_HASH_GRAD = 8,   /* hash-table gradient: simplex search + LDS fixed-point scatter (one level per workgroup) */
  NGM_K_HASH_REDUCE = 9, /* sum of the per-workgroup partial tables (+ fused sparse Adam on the tables)             */
  NGM_K_LOSS_REDUCE = 10,
  NGM_K_KNN_ASSIGN = 11, /* evaluation path: exact K nearest fields per point                                       */
  NGM_K_KNN_EVAL = 12,   /* evaluation path: per-field MLP tiles over the (point, neighbour) pairs (dominant there) */
  NGM_K_SAMPLER = 13,    /* standalone ray sampler (k_sample_rays / k_sample_rays_elem / k_sample_rays_weighted)            */
  NGM_K_COUNT = 14
};
int ngm_profile_enable(int32_t on);
int ngm_profile_reset(void);
int ngm_profile_read(int32_t kernel_id, double* total_ms, int64_t* launches);

/* Debug: with NGM_PHASE_TIMING set in the environment the backward kernel's first wave records its
 * s_memtime cycles per phase (prologue, inputs, encode, forward, output layer, staging, wgrad, dgrad,
 * encoding grads, relu mask, -, epilogue, total); this copies the 16 counters of the last launch. */
int ngm_debug_phase_cycles(unsigned long long* out528);   /* 16 slots (-DNGM_PHASE_TIMING) + 8 x 64 words the backward leaves zero */
/* Same for the fused forward (library built with -DNGM_PHASE_TIMING): slots = prologue, ray setup, sampler, step head,
 * encoding, hidden layers, activation stash stores, output layer, compositing, variance pass, ray outputs, block
 * reduction, -, -, total shader cycles, total 100 MHz ticks; then the event timeline of the 8 waves of that workgroup. */
int ngm_debug_fwd_phase_cycles(unsigned long long* out528);   /* 16 summary slots + 8 waves x 64 timeline entries ((slot << 48) | cycles) */

/* Debug: which MLP backward kernel the last ngm_render_bwd* / ngm_field_eval_bwd call launched:
 * 0 = k_field_bwd (32-sample tiles, forward recompute), 1 = k_field_bwd16 (16-sample tiles, recompute),
 * 2 = k_field_bwd16s (16-sample tiles, hidden activations read from the forward's stash), 3 = k_field_bwd_b3 (three-way
 * bf16 split, 32-sample tiles, stash), 5 = k_hash_mlp_bwd (hash
 * encoding + one hidden layer of <= 32 units, three-way bf16 split, encoding stash), -1 = none yet. */
int ngm_debug_last_bwd_variant(void);
/* Debug: the arithmetic the last launch of a forward-type kernel resolved ngm_field_cfg.matmul_mode to (AUTO is resolved
 * per kernel and batch shape): which = 0 fused render forward (ngm_render_fwd), 1 point evaluation (ngm_field_eval_fwd),
 * 2 kNN evaluation (ngm_field_eval_knn).  Returns NGM_MATMUL_F32 or NGM_MATMUL_BF16X3, -1 before the first launch. */
int ngm_debug_last_matmul(int which);
/* 1 when the last fused render forward ran the instance whose wave step evaluates ONE 32-sample tile (batches of at most 32
 * samples per wave: small per-rank batches), else 0 */
int ngm_debug_last_fwd_one_tile(void);
/* Debug: 1 when the last ngm_render_bwd / ngm_render_bwd_adam ran the compositing backward inside k_field_bwd_b3 (loss
 * seeds, pointwise geometry modes; no k_stash_bwd launch, the forward's colour / geometry stash stays intact), 0 when
 * k_stash_bwd ran.  ngm_debug_disable_fused_comp(1) forces the separate kernel. */
int ngm_debug_last_comp_fused(void);
int ngm_debug_disable_fused_comp(int on);   /* 1 = always launch k_stash_bwd; returns the previous setting */
/* DEVELOPER override of ngm_field_cfg.activation_stash for A/B timing of one library on one box (tools/): 0 / 1 force that
 * mode for every configuration of the process, -1 queries, -2 removes the override.  The product path never calls it: the
 * renderer sets ngm_field_cfg.activation_stash.
 * Returns the override in force before the call (-1: none). */
int ngm_debug_stash_mode(int mode);
int ngm_debug_last_stash_mode(void);   /* the stash the last MLP backward actually read: 0 / 1 as above, -1 none (recompute kernels) */
/* Debug: the MLP backward plan of a call with these arguments, without launching anything (no GPU needed).  rcfg != NULL: the
 * fused step on F fields x n rays (guided: the rays carry gt distances; seeds_written: the forward on the workspace ran with the
 * backward's targets, no per-workspace stash record); rcfg == NULL: the point evaluation on F x n points (stash_offered:
 * ngm_field_eval_bwd_stash rather than ngm_field_eval_bwd).  out5 = backward variant (ngm_debug_last_bwd_variant), compositing
 * fused, stash kind (0 none, 1 hidden activations, 2 hash encoding), stash layers, and the arithmetic the fused forward resolves
 * to (NGM_MATMUL_F32 / NGM_MATMUL_BF16X3; -1 in point mode).  Returns the plan's refusal (NGM_E_UNSUPPORTED / NGM_E_INVALID,
 * message in ngm_last_error) where the backward would refuse. */
int ngm_debug_plan_bwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t F, int64_t n, int32_t guided,
                       int32_t stash_offered, int32_t seeds_written, int32_t* out5);
/* Debug: the forward plan of a call with these arguments, without launching anything (no GPU needed; 256 compute units are
 * assumed without one).  surface 0: the fused render forward on F fields x n rays (rcfg required; guided: the rays carry gt
 * distances), 1: the point evaluation on F x n points, 2: the kNN evaluation (rcfg NULL for both).  out12 = compiled shape MI, MH, L,
 * arithmetic (NGM_MATMUL_F32 / NGM_MATMUL_BF16X3), one-tile wave step, waves per workgroup, dynamic LDS bytes, the neus instance,
 * threads per workgroup, rays per workgroup, samples buffered per wave, workgroups.  Returns the plan's refusal (NGM_E_UNSUPPORTED,
 * message in ngm_last_error) where the forward would refuse: no compiled instance, or an explicit NGM_MATMUL_BF16X3 outside the
 * split path's shape in the fused render forward. */
int ngm_debug_plan_fwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t surface, int32_t F, int64_t n, int32_t guided,
                       int32_t* out12);

/* ---- one-shot exchange of the loss sums between the ranks of one node ---------------
 * Replaces torch.distributed.all_reduce (RCCL) on the 16 floats between ngm_render_fwd and ngm_render_bwd* by ONE small
 * kernel that can be captured in the same hipGraph as the two: every rank writes its 16 values into every rank's
 * mailbox (peer memory mapped through hipIpc: xGMI stores), polls its own mailbox and sums in rank order -- bit-identical
 * sums on all ranks.  The reference has no counterpart (rm.py is single-process); the values are the sums / counts the
 * means of rm.py:1803-1871 are taken from.  Set-up (once per process group, host side, see distributed.PeerExchange):
 *   ngm_peer_alloc(ngm_peer_mailbox_bytes(), &mailbox)  ->  ngm_ipc_export(mailbox, handle)  ->  exchange the 64-byte
 *   handles by any means  ->  ngm_ipc_open(handle_of_rank_p, &px.mailbox[p]) for p != rank, px.mailbox[rank] = mailbox;
 *   px.seq / px.status: 8 + 4 bytes of zeroed device memory of this rank (ngm_peer_alloc works for them too).
 * Every rank must call ngm_loss_exchange the same number of times (idle ranks with zeros), like the collective it replaces.
 * A rank that waits longer than the time-out for a peer (default 30 s, ngm_peer_set_timeout; the all-reduce this replaces
 * would wait forever, a kernel must not: a dead peer would wedge the GPU) sets bit 0 of *status (sticky) and returns NaN in
 * all 16 sums: the losses and the update of THAT iteration are NaN on this rank, so the failure is visible at once and no
 * parameter is trained on partial normalisers.  A slot that already carries a later sequence number (ranks out of step
 * after such a time-out) is accepted and sets bit 1.  A non-zero status is fatal for the run. */
#define NGM_MAX_PEERS 8
typedef struct ngm_peer_exchange {
  int32_t world, rank;
  void* mailbox[NGM_MAX_PEERS];   /* [p] = rank p's mailbox as mapped into THIS process; [rank] = the own allocation   */
  unsigned long long* seq;        /* device counter of this rank, advanced by every exchange (starts at 0)             */
  int32_t* status;                /* device word of this rank: 0 = ok, bit 0 = time-out, bit 1 = out of step (sticky)   */
} ngm_peer_exchange;
int64_t ngm_peer_mailbox_bytes(void);
int ngm_peer_alloc(int64_t bytes, void** ptr);              /* zeroed fine-grained (uncached) device memory              */
int ngm_peer_free(void* ptr);
int ngm_ipc_export(void* ptr, unsigned char handle[64]);    /* hipIpcGetMemHandle                                        */
int ngm_ipc_open(const unsigned char handle[64], void** ptr);   /* hipIpcOpenMemHandle (lazy peer access)               */
int ngm_ipc_close(void* ptr);
int ngm_loss_exchange(const ngm_peer_exchange* px, float* loss_sums /* (16) device, summed in place */, void* stream);
/* How long an exchange waits for a peer before it gives up (process-wide, applies to launches and graph captures made
 * afterwards; <= 0 keeps the current value).  Returns the previous value in seconds.  Default 30 s, or NGM_PEER_TIMEOUT_S. */
double ngm_peer_set_timeout(double seconds);

#ifdef __cplusplus
}
#endif
#endif /* NGM_HIP_H */
