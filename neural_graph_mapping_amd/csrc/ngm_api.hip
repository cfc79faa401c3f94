// C ABI of the gfx950 hot path (declared in include/ngm_hip.h): argument validation, launch planning,
// workspace carving.  No allocation, no synchronisation; everything is enqueued on the caller's stream.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ngm_hip.h"
#include "ngm_launch.h"
#include "ngm_workspace.h"

int ngm_launch_sampler_weighted(const ngm_render_cfg* rc, const ngm_rays* rays, int S, int B, const float* boundaries,
                                const float* weights, float* points_cam, float* distances, float* dirs, hipStream_t st);
int ngm_launch_sampler(const ngm_render_cfg* rc, const ngm_rays* rays, int S, float* points_cam, float* distances,
                       float* dirs, float* points_world, hipStream_t st);
int ngm_launch_loss_values(const ngm_render_cfg* rc, const float* sums, float* out, hipStream_t st);
int ngm_launch_loss_reduce(const float* partials, int nblocks, float* sums, uint64_t* counter, hipStream_t st);
int ngm_launch_neus_sd_grad(const float* d_isd_rays, int F, int R, const float* neus_sd, int64_t sd_stride,
                            const int64_t* field_index, float* d_sd, hipStream_t st);
int ngm_launch_read_stash(const float4* sa, const float2* sb, int64_t n, float* geoms, float* dists, hipStream_t st);
int ngm_launch_adam(float* param, float* m, float* v, int64_t stride, const float* grad, int64_t gstride, int F, int64_t numel,
                    const AdamHyper& h, hipStream_t st);
int ngm_launch_adam_multi(const ngm_adam_tensor* tensors, int n, int F, const AdamHyper& h, int64_t* advance_step,
                          uint64_t* advance_offset, hipStream_t st, const int32_t* num_active = nullptr);
int ngm_launch_step_advance(int64_t* step_dev, uint64_t* off_dev, hipStream_t st);
int64_t ngm_mc_workspace_bytes(int nx, int ny, int nz);
int ngm_launch_mc_count(const float* vol, int nx, int ny, int nz, float iso, int64_t* counts, void* workspace,
                        int64_t workspace_bytes, hipStream_t st);
int ngm_launch_mc_emit(const float* vol, int nx, int ny, int nz, float iso, float* verts, int64_t max_verts,
                       int64_t* faces, int64_t max_faces, void* workspace, int64_t workspace_bytes, hipStream_t st);
int ngm_mc_copy_tables(int8_t* tri_table, int32_t* tri_count);
int64_t ngm_surface_sample_bytes(int64_t num_faces);
int ngm_launch_surface_sample(const float* verts, int64_t V, const int64_t* faces, int64_t F, int64_t N, uint64_t seed, float* points,
                              int64_t* face_ids, void* workspace, int64_t workspace_bytes, hipStream_t st);
int64_t ngm_nearest_point_bytes(int64_t M, int64_t N);
int ngm_launch_nearest_point(const float* refs, int64_t M, const float* queries, int64_t N, float* dist, int64_t* index, void* workspace,
                             int64_t workspace_bytes, hipStream_t st);
int64_t ngm_mesh_vertex_normals_bytes(int64_t V);
int ngm_launch_mesh_vertex_normals(const float* verts, int64_t V, const int64_t* faces, int64_t F, float* normals, void* workspace,
                                   int64_t workspace_bytes, hipStream_t st);
int64_t ngm_icp_point_to_plane_bytes(int64_t M, int64_t N);
int ngm_launch_icp_point_to_plane(const float* source, int64_t N, const float* target, const float* target_normals, int64_t M,
                                  double threshold, int max_iteration, double relative_fitness, double relative_rmse, const double* init,
                                  double* state, void* workspace, int64_t workspace_bytes, hipStream_t st);
int64_t ngm_image_metrics_bytes(int B, int H, int W, int crop);
int ngm_launch_image_metrics(const float* pred, const float* target, int B, int H, int W, int crop, double* out, void* workspace,
                             int64_t workspace_bytes, hipStream_t st);
int64_t ngm_cover_bytes(int H, int W, int num_active, int max_new);
const int32_t* ngm_cover_counters(int H, int W, int num_active, int max_new, void* workspace);
int ngm_launch_cover(const ngm_cover_depth_args& a, void* workspace, int64_t workspace_bytes, hipStream_t st);
int64_t ngm_mesh_subdivide_bytes(int64_t F);
int ngm_launch_mesh_subdivide_count(const float* verts, int64_t V, const int64_t* faces, int64_t F, double max_edge, int max_iter,
                                    void* workspace, int64_t workspace_bytes, int64_t* totals, hipStream_t st);
int ngm_launch_mesh_subdivide_emit(const float* verts, int64_t V, const int64_t* faces, int64_t F, const float* attrs, int C,
                                   const void* workspace, int64_t new_vertices, int64_t out_faces, float* out_verts,
                                   int64_t* out_faces_idx, float* out_attrs, int64_t* out_parent, hipStream_t st);
int ngm_launch_mesh_depth(const float* verts, int64_t V, const int64_t* faces, int64_t F, const float* c2w, int64_t P, int W, int H,
                          float fx, float fy, float cx, float cy, float near, float far, float* depth, hipStream_t st);
int ngm_launch_mesh_visibility(const float* verts, int64_t V, const float* c2w, int64_t P, int W, int H, float fx, float fy, float cx,
                               float cy, const float* depth, float eps, int64_t num_frustum_poses, int32_t* in_frustum,
                               int32_t* observed, hipStream_t st);
int ngm_launch_knn(const ngm_field_cfg* fc, const ngm_params* pr, int num_fields, int64_t P, const float* points,
                   const float* pos, const float* quat, int K, float distance_factor, float outside_value, float mask_radius,
                   float* out, void* workspace, int64_t workspace_bytes, const FwdPlan& plan, hipStream_t st);
int ngm_launch_grid_knn(const ngm_field_cfg* fc, const ngm_params* pr, int num_fields, const float* pos, const float* quat,
                        const float* xs, int nx, const float* ys, int ny, const float* zs, int nz, int K, float distance_factor,
                        float outside_value, float mask_radius, int channel, int negate, float* volume, void* workspace,
                        int64_t workspace_bytes, const FwdPlan& plan, hipStream_t st);
int64_t ngm_knn_workspace_bytes(int num_fields, int64_t P, int K);
int64_t ngm_knn_render_workspace_bytes(int num_fields, int ray_block, int S, int K);
int ngm_launch_render_eval_knn(const ngm_field_cfg* fc, const ngm_render_cfg* rc, const ngm_params* pr, int num_fields,
                               const float* pos, const float* quat, const ngm_rays* rays, int K, float distance_factor,
                               float outside_value, float mask_radius, int ray_block, const ngm_prediction* pred,
                               void* workspace, int64_t workspace_bytes, const FwdPlan& plan, hipStream_t st);

#include <mutex>
#include <unordered_map>
#include <vector>

static thread_local char g_err[512] = "";
static int check_enc_grads(const ngm_field_cfg* fc, const ngm_grads* grads, FieldBwdArgs& a);

// ---- profiling hooks ----------------------------------------------------------------------------
namespace {
struct EvPair { hipEvent_t a, b; };
std::mutex g_prof_mu;
bool g_prof_on = false;
std::vector<EvPair> g_prof_pending[NGM_K_COUNT];
std::vector<EvPair> g_prof_free;
double g_prof_ms[NGM_K_COUNT] = {0};
int64_t g_prof_n[NGM_K_COUNT] = {0};
thread_local EvPair g_cur;
}  // namespace

NgmProfScope::NgmProfScope(int kernel_id, hipStream_t stream) : id(kernel_id), st(stream), on(false) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_on) return;
  on = true;
  if (g_prof_free.empty()) {
    EvPair p;
    (void)hipEventCreate(&p.a);
    (void)hipEventCreate(&p.b);
    g_cur = p;
  } else {
    g_cur = g_prof_free.back();
    g_prof_free.pop_back();
  }
  (void)hipEventRecord(g_cur.a, st);
}
NgmProfScope::~NgmProfScope() {
  if (!on) return;
  (void)hipEventRecord(g_cur.b, st);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_pending[id].push_back(g_cur);
}
static void prof_drain() {
  for (int k = 0; k < NGM_K_COUNT; ++k) {
    for (auto& p : g_prof_pending[k]) {
      float ms = 0.f;
      (void)hipEventSynchronize(p.b);
      if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { g_prof_ms[k] += ms; g_prof_n[k] += 1; }
      g_prof_free.push_back(p);
    }
    g_prof_pending[k].clear();
  }
}

static int fail(int code, const char* msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
#define NGM_FWD_DEBUG_WORDS (16 + 8 * 64)   // 16 summary slots + 8 waves x 64 timeline entries
static unsigned long long* g_debug_cycles = nullptr;
static int g_no_fused_comp = 0;       // ngm_debug_disable_fused_comp
static int g_stash_override = -1;     // ngm_debug_stash_mode
// Which targets the LAST forward on a workspace wrote its per-ray loss seeds for (host-side bookkeeping by pointer identity:
// the fused compositing backward trusts off_rayseed only when the forward that filled this workspace ran with the same
// targets; a forward without targets, or with other targets, leaves the backward on k_stash_bwd, which derives the seeds
// from targets + prediction itself).
static std::mutex g_seed_mu;
static std::unordered_map<const void*, const void*> g_seed_targets;       // workspace -> targets.rgbds of the forward that wrote the seeds
static std::unordered_map<const void*, int> g_ws_act_layers;              // workspace -> hidden layers the last training forward stashed (0: all)
static void note_forward_stash(const void* ws, int act_layers) {
  std::lock_guard<std::mutex> lk(g_seed_mu);
  if (g_ws_act_layers.size() >= 4096) g_ws_act_layers.clear();
  g_ws_act_layers[ws] = act_layers;
}
// -1: no record (another process wrote the workspace, or the record was dropped): trust the backward's own predicate
static int forward_stash_layers(const void* ws) {
  std::lock_guard<std::mutex> lk(g_seed_mu);
  auto it = g_ws_act_layers.find(ws);
  return it == g_ws_act_layers.end() ? -1 : it->second;
}
static void note_forward_seeds(const void* ws, const void* rgbds) {
  std::lock_guard<std::mutex> lk(g_seed_mu);
  if (!rgbds) { g_seed_targets.erase(ws); return; }
  // bounded: a caller that allocates a fresh workspace per forward (the autograd ops do) would otherwise grow the map by one
  // entry per distinct address for the life of the process.  Dropping old entries is safe: a backward that finds none runs the
  // separate k_stash_bwd instead of the fused seeds (same results, one launch more).
  if (g_seed_targets.size() >= 4096) g_seed_targets.clear();
  g_seed_targets[ws] = rgbds;
}
static bool forward_wrote_seeds_for(const void* ws, const void* rgbds) {
  std::lock_guard<std::mutex> lk(g_seed_mu);
  auto it = g_seed_targets.find(ws);
  return it != g_seed_targets.end() && it->second == rgbds;
}

static int check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return NGM_E_HIP;
  }
  return NGM_OK;
}
static int num_cus() {
  static int cached = 0;
  if (cached) return cached;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
    cached = prop.multiProcessorCount;
  else
    cached = 256;  // MI355X
  (void)hipGetLastError();
  return cached;
}
// ---- the forward plan ----------------------------------------------------------------------------------------------------------
// Which forward instance a call runs -- shape, arithmetic, wave step -- and how it is launched: plan_fwd fills one FwdPlan
// (ngm_launch.h) from plain values, before anything is carved or launched; the launchers switch on it.
struct FwdAsk {
  int surface = NGM_FWD_RENDER;         // NGM_FWD_RENDER / NGM_FWD_POINTS / NGM_FWD_KNN
  const ngm_render_cfg* rc = nullptr;   // fused render: geometry mode
  int F = 1;
  int64_t n = 0;                        // fused render: rays per field; point evaluation: points per field
  int S = 0;                            // fused render: samples per ray
  bool counted = false;                 // fused render: the call carries a device count of active rows
};
static const char* const no_instance = "forward: the launcher does not take the planned instance (internal error)";
static FwdPlan g_last_fwd[3];           // per surface, the last plan that launched (ngm_debug_last_matmul / _fwd_one_tile)
// The only reader of NGM_NO_HALF_STEP (developer A/B switch: never the one-tile wave step).  A refused fused-render plan still
// carries the launch shape the workspace is sized by.
static FwdPlan plan_fwd(const ngm_field_cfg* fc, const FwdAsk& q) {
  static const bool no_half = getenv("NGM_NO_HALF_STEP") != nullptr;
  static thread_local char why[256];
  FwdPlan p;
  p.surface = q.surface;
  p.MI = (fc->dim_enc + 31) / 32; p.MH = (fc->dim_hidden + 31) / 32; p.L = fc->num_layers;
  p.need_cos = fc->encoding == NGM_ENC_NERF;
  p.hash = fc->encoding == NGM_ENC_PERMUTO ? 1 : fc->encoding == NGM_ENC_TRIPLANE ? 2 : 0;
  p.skip = fc->skip_mode;
  const int ncu = num_cus();
  const bool neus = q.rc && q.rc->geometry_mode == NGM_GEO_NEUS;
  p.counted = q.counted;
  p.neus = neus;
  const char* const no_kernel = "no forward kernel for this (D,H,L)";
  auto finish = [&](bool b3, const char* refusal) {
    p.matmul = b3 ? NGM_MATMUL_BF16X3 : NGM_MATMUL_F32;
    p.threads = 64 * p.waves;
    if (!refusal && p.lds_bytes > NGM_LDS_MAX) refusal = "the forward's weights and sample planes do not fit the LDS";
    if (refusal) { p.status = NGM_E_UNSUPPORTED; p.why = refusal; }
    return p;
  };
  if (q.surface != NGM_FWD_RENDER) {     // the evaluations: the mode is a preference (fp32 MFMA where the split is not compiled)
    const bool points = q.surface == NGM_FWD_POINTS;
    const bool b3 = fc->matmul_mode != NGM_MATMUL_F32 && (points ? ngm_points_fwd_takes(*fc, true) : ngm_knn_eval_takes(*fc, true));
    p.waves = b3 ? 8 : NGM_WAVES_PER_BLOCK;
    p.lds_bytes = ngm_fwd_lds_bytes(*fc, b3, 0, 0);
    if (points) {
      int64_t bpf = (ncu + q.F - 1) / q.F;                     // workgroups per field
      p.per_block = align_up((q.n + bpf - 1) / bpf, NGM_BLOCK);
      bpf = (q.n + p.per_block - 1) / p.per_block;
      p.blocks = (int)(bpf * q.F);
    } else {
      p.blocks = (b3 ? 1 : 4) * ncu;
    }
    return finish(b3, (points ? ngm_points_fwd_takes(*fc, false) : ngm_knn_eval_takes(*fc, false)) ? nullptr : no_kernel);
  }
  // fused render: one workgroup per CU-slot; 8 waves (2 per SIMD: latency hiding) unless the per-wave LDS sample planes would
  // not fit, then 4 waves
  const int F = q.F, R = (int)q.n;
  auto shape = [&](int waves, bool planes, int64_t maxs_cap = 1024) {
    int ch = (ncu + F - 1) / F;
    const int max_ch = (R + waves - 1) / waves;
    if (ch > max_ch) ch = max_ch;
    if (ch < 1) ch = 1;
    int rpb = (R + ch - 1) / ch;
    rpb = (int)align_up(rpb, waves);
    const int rpw = rpb / waves;
    int64_t maxs = align_up((int64_t)(rpw < 32 ? rpw : 32) * q.S, 64);
    if (maxs > maxs_cap) maxs = maxs_cap;                // samples a wave buffers per ray batch (whole rays)
    if (maxs < align_up(q.S, 64)) maxs = align_up(q.S, 64);
    p.rays_per_block = rpb; p.waves = waves; p.maxs = (int)maxs;
    p.blocks = F * ((R + rpb - 1) / rpb);
    p.lds_bytes = ngm_fwd_lds_bytes(*fc, planes, waves, p.maxs);
    return p.lds_bytes <= NGM_LDS_MAX;
  };
  if (!shape(8, false) || R < 8) shape(4, false);        // exact-fp32 plan first: 8 waves unless its LDS does not fit
  // a grid of 8-wave workgroups that leaves CUs idle (a rank with one or two active fields): 4 waves per
  // workgroup on twice as many CUs -- one wave per SIMD runs a step in about half the time (F = 1: 29 -> 25.5 us, split path)
  const bool few = R >= 8 && (int64_t)F * ((R + 7) / 8) < ncu;
  // The split path's weight planes (48 KB for two 64-wide layers) compete with the per-wave sample planes for LDS: a
  // batch of many samples per ray (8192 x 256: 1024 samples buffered per wave) leaves no room at 8 waves.  Smaller ray
  // batches per wave do (one 256-sample ray at a time: 8.7 KB per wave), at no measurable cost -- tried in that order.
  auto fit_b3 = [&]() {
    for (int64_t cap : {(int64_t)1024, (int64_t)512, (int64_t)256})
      if (shape(8, true, cap) && R >= 8) return true;
    return shape(4, true);
  };
  bool b3 = false;
  if (fc->matmul_mode == NGM_MATMUL_BF16X3) {           // explicit: whatever shape makes it fit, refused where it is not compiled
    b3 = !neus;
    (void)fit_b3();
    if (!ngm_render_fwd_takes(*fc, neus, true)) {
      snprintf(why, sizeof(why), "render_fwd: matmul_mode bf16x3 has no fused-forward instance for shape <%d,%d,%d> with this encoding, "
               "skip mode and geometry mode (neus runs fp32 MFMA): use NGM_MATMUL_AUTO or NGM_MATMUL_F32", p.MI, p.MH, p.L);
      return finish(b3, why);
    }
  } else if (fc->matmul_mode == NGM_MATMUL_AUTO && ngm_render_fwd_takes(*fc, neus, true)) {
    const FwdPlan keep = p;
    b3 = (few && shape(4, true)) || (fit_b3() && p.waves == 8);      // auto: the planes next to an 8-wave plan, else exact-fp32 MFMA
    if (!b3) p = keep;
  }
  // every wave's batches hold at most 32 samples (rays per wave x samples per ray): the one-tile instance of the split path and
  // of the hash encoding without skip connection
  p.one_tile = !neus && !no_half && (int64_t)(p.rays_per_block / p.waves) * q.S <= 32 && (b3 || (p.hash == 1 && p.skip == NGM_SKIP_NO));
  return finish(b3, ngm_render_fwd_takes(*fc, neus, b3) ? nullptr : no_kernel);
}

// ---- the MLP backward plan -----------------------------------------------------------------------------------------------------
// Which kernel a backward runs (variant: 0 k_field_bwd, 1 k_field_bwd16, 2 k_field_bwd16s, 3 k_field_bwd_b3, 5 k_hash_mlp_bwd),
// which stash the forward writes for it and whether the compositing backward rides inside it are ONE decision, taken by
// plan_mlp_bwd from plain values.  Forward and backward ask it before anything is carved or launched: a stash is written exactly
// when a kernel reads it, and a refusal leaves workspace, gradients, parameters and counters as they were.
struct BwdAsk {
  const ngm_render_cfg* rc = nullptr;   // ray mode; NULL: point mode
  int F = 1;
  int64_t P = 0;                        // samples per field
  bool seeded = false;                  // ray mode: explicit seeds (ngm_render_bwd_seeded*), not the loss
  bool stash_offered = false;           // point mode: the caller holds a stash for the forward to write / the backward to read
  int rec_layers = -1;                  // per-workspace record forward_stash_layers: 0 every hidden layer, 1 layer 0 only, -1 none
  bool seeds_written = false;           // per-workspace record forward_wrote_seeds_for these targets
};
struct BwdPlan {
  int status; const char* why;          // NGM_OK, or the refusal (NGM_E_UNSUPPORTED / NGM_E_INVALID) and its message
  int stash_kind;                       // 0: none; 1: post-ReLU hidden activations (64 floats per sample and layer); 2: the hash
                                        // encoding itself (32 features per sample: no simplex search, no table gathers)
  int stash_layers, half;               // layers in the stash: every hidden layer, or (half) layer 0 of two; kind 2: 1
  int variant, fused_comp;
  int64_t per_block; int blocks_per_field;
};
static BwdPlan g_last_bwd = {NGM_OK, nullptr, 0, 0, 0, -1, 0, 0, 0};   // the last plan that launched (ngm_debug_last_*)

// unit: samples a workgroup's range is a multiple of -- whole 32-sample tiles for each of its waves (4 waves: 128; the
// hash network's 8-wave backward: 256)
static void plan_bwd(int F, int64_t P, int64_t* per_block, int* bpf, int64_t unit = 32 * NGM_WAVES_PER_BLOCK) {
  const int ncu = num_cus();
  int64_t b = (ncu + F - 1) / F;
  int64_t per = align_up((P + b - 1) / b, unit);
  if (per < unit) per = unit;
  *per_block = per;
  *bpf = (int)((P + per - 1) / per);
}
// The only reader of the three process switches: NGM_NO_ACT_STASH=1 (recompute everywhere; saves the stash's workspace),
// ngm_debug_stash_mode (developer A/B override of ngm_field_cfg.activation_stash) and ngm_debug_disable_fused_comp.
static BwdPlan plan_mlp_bwd(const ngm_field_cfg* fc, const BwdAsk& q) {
  static const bool no_stash = getenv("NGM_NO_ACT_STASH") != nullptr;
  BwdPlan p;
  memset(&p, 0, sizeof(p));
  p.variant = -1;
  const bool ray = q.rc != nullptr;
  const int L = fc->num_layers, ti = (fc->dim_enc + 15) / 16, th = (fc->dim_hidden + 15) / 16;
  plan_bwd(q.F, q.P, &p.per_block, &p.blocks_per_field, ray && fc->encoding == NGM_ENC_PERMUTO ? 256 : 128);
  BwdProblem pr = {!ray, q.P, p.per_block, 0, false, false};
  // The stash.  Its consumers are skip-less (with a skip connection the stashed activation no longer tells the ReLU mask); the
  // triplane backward recomputes (it needs the taps anyway).  Point mode: only k_field_bwd_b3 reads one.
  if (!no_stash && fc->skip_mode == NGM_SKIP_NO && fc->encoding != NGM_ENC_TRIPLANE) {
    if (fc->encoding == NGM_ENC_PERMUTO) pr.stash_kind = (ti == 2 && fc->dim_hidden <= 32) ? 2 : 0;
    else pr.stash_kind = (ti == 4 && th == 4 && L <= 2) ? 1 : 0;
    if (!ray && !(pr.stash_kind == 1 && q.stash_offered && ngm_field_bwd_b3_takes(*fc, pr))) pr.stash_kind = 0;
  }
  // Half stash: with two hidden layers on the split path the forward stashes layer 0's output only and k_field_bwd_b3<.., HS>
  // recomputes the output layer's input from it: 256 instead of 512 bytes of stash per sample each way.  What the forward on
  // this workspace recorded wins over the configuration the backward was handed.
  if (pr.stash_kind && q.rec_layers >= 0) pr.half = q.rec_layers != 0;
  else if (ray && pr.stash_kind == 1 && L == 2 && (g_stash_override >= 0 ? g_stash_override : fc->activation_stash == NGM_STASH_HALF)) {
    pr.half = true;
    pr.half = ngm_field_bwd_b3_takes(*fc, pr);
  }
  p.stash_kind = pr.stash_kind; p.half = pr.half;
  p.stash_layers = pr.stash_kind == 1 ? (pr.half ? 1 : L) : pr.stash_kind == 2 ? 1 : 0;
  auto refuse = [&](int status, const char* why) { p.status = status; p.why = why; return p; };
  if (L > 2)
    return refuse(NGM_E_UNSUPPORTED, "num_layers = 3 is forward only (point evaluation, fused render forward, kNN evaluation): no backward kernel");
  // the table gradient follows the MLP backward in every backward: a table it does not take is refused here, not after that launch
  if (fc->encoding == NGM_ENC_PERMUTO && !ngm_hash_grad_takes(*fc))
    return refuse(NGM_E_UNSUPPORTED, "permutohedral backward: hash table too large for the LDS-staged scatter");
  // Compositing backward inside the MLP backward: the loss (not explicit seeds) in a pointwise geometry mode, per-ray seeds
  // the forward wrote for these targets, ray indices that fit 24 bits, and a stash kernel that takes the fused problem.  The
  // variance-weighted loss modes (gradients through the rendered variances) are k_stash_bwd's.
  const bool may_fuse = ray && !g_no_fused_comp && !q.seeded && q.seeds_written && q.P < (1 << 24) &&
                        q.rc->geometry_mode != NGM_GEO_NEUS && q.rc->geometry_mode != NGM_GEO_DENSITY &&             // pointwise
                        q.rc->photometric_mode != NGM_PHOTO_GAUSSIAN_NLL && q.rc->depth_mode == NGM_DEPTH_HUBER;      // no *_nll
  // In order of preference: bf16-split tiles on the activation stash -> hash encoding + 1x32 MLP on its encoding stash (both
  // fused if they may) -> 16-sample tiles on the stash -> 16-sample-tile recompute -> 32-sample-tile recompute.
  auto stash_kernel = [&](bool fused) {
    pr.fused_comp = fused;
    return ngm_field_bwd_b3_takes(*fc, pr) ? 3 : ngm_hash_mlp_bwd_takes(*fc, pr) ? 5 : -1;
  };
  if (pr.stash_kind) {
    if (may_fuse) p.variant = stash_kernel(true);
    p.fused_comp = p.variant >= 0;
    if (p.variant < 0) p.variant = stash_kernel(false);
    if (pr.half && p.variant != 3)                       // no other kernel reads a half stash
      return refuse(NGM_E_INVALID, "render_bwd: the forward stashed one hidden layer (split path) but k_field_bwd_b3 does not take this problem");
    if (p.variant < 0 && ngm_field_bwd16s_takes(*fc, pr)) p.variant = 2;
  }
  if (p.variant < 0 && ngm_field_bwd16_takes(*fc, pr)) p.variant = 1;
  if (p.variant < 0 && ngm_field_bwd_takes(*fc, pr)) p.variant = 0;
  if (p.variant < 0) return refuse(NGM_E_UNSUPPORTED, "no MLP backward kernel for this (D,H,L)");
  return p;
}
static int launch_mlp_bwd(const BwdPlan& p, FieldBwdArgs& a, hipStream_t st) {
  static const bool timing = getenv("NGM_PHASE_TIMING") != nullptr;
  a.debug_cycles = nullptr;
  if (timing) {
    if (!g_debug_cycles) { (void)hipMalloc(&g_debug_cycles, NGM_FWD_DEBUG_WORDS * 8); (void)hipMemset(g_debug_cycles, 0, NGM_FWD_DEBUG_WORDS * 8); }
    a.debug_cycles = g_debug_cycles;
  }
  g_last_bwd = p;
  const int blocks = a.blocks_per_field * a.F;
  int e = NGM_E_INVALID;
  switch (p.variant) {
    case 3: e = ngm_launch_field_bwd_b3(a, blocks, st); break;
    case 5: e = ngm_launch_hash_mlp_bwd(a, blocks, st); break;
    case 2: e = ngm_launch_field_bwd16s(a, blocks, st); break;
    case 1: e = ngm_launch_field_bwd16(a, blocks, st); break;
    case 0: e = ngm_launch_field_bwd(a, blocks, st); break;
  }
  return e ? fail(e, "MLP backward: the launcher does not take the planned problem (internal error)") : check_launch("ngm_field_bwd");
}

// mlp = false: the standalone encoding stages (ngm_encode_fwd / ngm_encode_bwd), which never run the hidden layers
static int check_field_cfg(const ngm_field_cfg* fc, bool mlp = true) {
  if (!fc) return fail(NGM_E_INVALID, "field cfg is NULL");
  if (fc->dim_out != 4) return fail(NGM_E_UNSUPPORTED, "dim_out must be 4 (r,g,b,geometry)");
  if (fc->num_layers < 1 || fc->num_layers > NGM_MAX_LAYERS) return fail(NGM_E_UNSUPPORTED, "num_layers out of range");
  // depths no launcher has a kernel for (include/ngm_hip.h, NGM_MAX_LAYERS): refused here, before any launch
  if (mlp && fc->num_layers > 3)
    return fail(NGM_E_UNSUPPORTED, "num_layers = 4: no entry point has a kernel for four hidden layers (1-2: everything; 3: forward only, 33..64-wide)");
  if (mlp && fc->num_layers == 3 && (fc->dim_enc <= 32 || fc->dim_hidden <= 32))
    return fail(NGM_E_UNSUPPORTED, "num_layers = 3 needs dim_enc and dim_hidden in 33..64: no entry point has a three-layer kernel for layers of 32 units or fewer");
  if (fc->encoding == NGM_ENC_PERMUTO) {
    if (fc->nr_feat_per_level != 2 || fc->nr_levels < 1 || fc->nr_levels > 16 || fc->dim_enc != 2 * fc->nr_levels)
      return fail(NGM_E_UNSUPPORTED, "permutohedral encoding: nr_feat_per_level must be 2, nr_levels <= 16, no concat_points");
    if (fc->log2_hashmap_size < 4 || fc->log2_hashmap_size > 24) return fail(NGM_E_UNSUPPORTED, "permutohedral: log2_hashmap_size out of range");
    if (!(fc->level_scale[0] > 0.f)) return fail(NGM_E_INVALID, "permutohedral: level_scale not filled (ngm_permuto_fill_scales)");
  }
  if (fc->encoding == NGM_ENC_NERF && fc->dim_enc != 6 * fc->num_octaves) return fail(NGM_E_INVALID, "nerf: dim_enc != 6*octaves");
  if (fc->encoding == NGM_ENC_TRIPLANE) {
    if (fc->tri_resolution < 2 || fc->tri_resolution > 4096 || fc->tri_mode < NGM_TRI_SUM || fc->tri_mode > NGM_TRI_CONCAT ||
        (fc->tri_mode == NGM_TRI_CONCAT && fc->dim_enc % 3))
      return fail(NGM_E_INVALID, "triplane: resolution / mode / dim_enc inconsistent");
  }
  if (fc->encoding == NGM_ENC_NONE && fc->dim_enc != 3) return fail(NGM_E_INVALID, "no encoding: dim_enc must be 3");
  if (fc->dim_enc < 1 || fc->dim_enc > 64 || fc->dim_hidden < 1 || fc->dim_hidden > 64)
    return fail(NGM_E_UNSUPPORTED, "dim_enc / dim_hidden must be <= 64");
  if (((fc->dim_enc + 31) / 32) != ((fc->dim_hidden + 31) / 32) && !(fc->dim_enc <= 32 && fc->dim_hidden <= 32))
    return fail(NGM_E_UNSUPPORTED, "dim_enc and dim_hidden must pad to the same multiple of 32");
  if (fc->skip_mode != NGM_SKIP_NO && fc->skip_mode != NGM_SKIP_ADD && fc->skip_mode != NGM_SKIP_CONCAT)
    return fail(NGM_E_UNSUPPORTED, "skip_mode: no / add / concat");
  // skip connections are encoding-agnostic like models.py:159-169 (every encoding x {no, add, concat}); "add" needs room for
  // the encoding in the hidden units (the reference adds out[..., :D] += encoding: D <= H)
  if (fc->skip_mode == NGM_SKIP_ADD && fc->dim_hidden < fc->dim_enc)
    return fail(NGM_E_UNSUPPORTED, "skip_mode add: needs dim_hidden >= dim_enc");
  if (fc->activation_stash != NGM_STASH_FULL && fc->activation_stash != NGM_STASH_HALF)
    return fail(NGM_E_INVALID, "activation_stash: NGM_STASH_FULL / NGM_STASH_HALF (ABI 10: is the struct the caller built 276 bytes?)");
  if (fc->hash_grad_atomics != NGM_HASH_ATOMICS_EXACT && fc->hash_grad_atomics != NGM_HASH_ATOMICS_FLOAT)
    return fail(NGM_E_INVALID, "hash_grad_atomics: NGM_HASH_ATOMICS_EXACT / NGM_HASH_ATOMICS_FLOAT");
  return NGM_OK;
}
static int check_params(const ngm_field_cfg* fc, const ngm_params* pr) {
  if (!pr) return fail(NGM_E_INVALID, "params is NULL");
  if (fc->encoding == NGM_ENC_FOURIER && !pr->enc_w) return fail(NGM_E_INVALID, "fourier encoding needs enc_w");
  if (fc->encoding == NGM_ENC_PERMUTO && (!pr->lattice || !pr->shift)) return fail(NGM_E_INVALID, "permutohedral encoding needs lattice + shift");
  if (fc->encoding == NGM_ENC_TRIPLANE && (!pr->planes || pr->dtype != NGM_DT_F32)) return fail(NGM_E_INVALID, "triplane encoding needs fp32 planes");
  for (int l = 0; l <= fc->num_layers; ++l)
    if (!pr->w[l] || !pr->b[l]) return fail(NGM_E_INVALID, "missing layer weight/bias pointer");
  if (pr->dtype != NGM_DT_F32 && pr->dtype != NGM_DT_BF16 && pr->dtype != NGM_DT_F16) return fail(NGM_E_INVALID, "params.dtype");
  return NGM_OK;
}

extern "C" {

int ngm_abi_version(void) { return NGM_ABI_VERSION; }

int ngm_permuto_fill_scales(ngm_field_cfg* cfg) {
  if (!cfg || cfg->nr_levels < 1 || cfg->nr_levels > 16 || !(cfg->coarsest_scale > 0) || !(cfg->finest_scale > 0))
    return fail(NGM_E_INVALID, "ngm_permuto_fill_scales: bad configuration");
  const int L = cfg->nr_levels;
  const double la = log10((double)cfg->coarsest_scale), lb = log10((double)cfg->finest_scale);
  for (int l = 0; l < L; ++l) {
    double sig = (L == 1) ? cfg->coarsest_scale : pow(10.0, la + (lb - la) * (double)l / (double)(L - 1));
    if (l == 0) sig = cfg->coarsest_scale;
    if (l == L - 1 && L > 1) sig = cfg->finest_scale;
    for (int i = 0; i < 3; ++i) cfg->level_scale[3 * l + i] = (float)((1.0 / sqrt((double)((i + 1) * (i + 2)))) / sig);
  }
  return NGM_OK;
}
const char* ngm_last_error(void) { return g_err; }

int ngm_profile_enable(int32_t on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = on != 0;
  return NGM_OK;
}
int ngm_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_drain();
  for (int k = 0; k < NGM_K_COUNT; ++k) { g_prof_ms[k] = 0; g_prof_n[k] = 0; }
  return NGM_OK;
}
int ngm_profile_read(int32_t kernel_id, double* total_ms, int64_t* launches) {
  if (kernel_id < 0 || kernel_id >= NGM_K_COUNT) return fail(NGM_E_INVALID, "bad kernel id");
  std::lock_guard<std::mutex> lk(g_prof_mu);
  prof_drain();
  if (total_ms) *total_ms = g_prof_ms[kernel_id];
  if (launches) *launches = g_prof_n[kernel_id];
  return NGM_OK;
}

// ------------------------------------------------------------------------------------------------
// training-target sampler
// ------------------------------------------------------------------------------------------------
static int check_keyframes(const ngm_keyframes* kf) {
  if (!kf || !kf->c2ws || !kf->rgbd || !kf->frame_to_store) return fail(NGM_E_INVALID, "target sampler: NULL keyframe argument");
  if (kf->num_frames < 1 || kf->height < 1 || kf->width < 1) return fail(NGM_E_INVALID, "target sampler: empty keyframe set");
  return NGM_OK;
}
int ngm_target_visibility(const ngm_keyframes* kf, int32_t F, const float* field_pos, int32_t num_offsets, const float* offsets,
                          float radius, uint8_t* kf_mask, float* bbox, void* stream) {
  int e = check_keyframes(kf);
  if (e) return e;
  if (F < 0 || num_offsets < 1 || !field_pos || !offsets || !kf_mask || !bbox) return fail(NGM_E_INVALID, "ngm_target_visibility: bad argument");
  if (F == 0) return NGM_OK;
  ngm_launch_target_visibility(*kf, F, field_pos, num_offsets, offsets, radius, kf_mask, bbox, (hipStream_t)stream);
  return check_launch("ngm_target_visibility");
}
int ngm_target_rays(const ngm_keyframes* kf, int32_t F, int32_t R, const float* field_pos, float radius, const float* bbox,
                    const int64_t* frame_cids, const float* u_xy, const ngm_target_out* out, void* stream) {
  int e = check_keyframes(kf);
  if (e) return e;
  if (F < 0 || R < 1 || !field_pos || !bbox || !frame_cids || !u_xy || !out || !out->ijs || !out->near || !out->far || !out->gt ||
      !out->rgbds || !out->rgb_mask || !out->depth_mask || !out->term_probs || !out->term_mask)
    return fail(NGM_E_INVALID, "ngm_target_rays: bad argument");
  if (F == 0) return NGM_OK;
  ngm_launch_target_rays(*kf, F, R, field_pos, radius, bbox, frame_cids, u_xy, *out, (hipStream_t)stream);
  return check_launch("ngm_target_rays");
}

// ngm_target_sample_mv and ngm_target_sample_mv_live (is_live; its sizes are maxima, include/ngm_hip.h): one list of checks in
// which five conditions differ, one launcher.  `fn` is the entry point that was called.
static int target_sample_mv(const char* fn, bool is_live, const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_live* live,
                            const ngm_target_out* out, void* workspace, int64_t workspace_bytes, void* stream,
                            const int32_t* num_fields_dev = nullptr) {
  char msg[256];
  auto refuse = [&](int code, const char* what) { return snprintf(msg, sizeof(msg), "%s: %s", fn, what), fail(code, msg); };
  int e = check_keyframes(kf);
  if (e) return e;
  if (!s || !out || (is_live && !live)) return refuse(NGM_E_INVALID, "NULL argument");
  if (s->num_current < (is_live ? 1 : 0) || s->num_fields < 0 || s->num_rays < 1 || s->world_size < 1 || s->rank < 0 ||
      s->rank >= s->world_size || (is_live && live->num_train_fields < 0))
    return refuse(NGM_E_INVALID, is_live ? "bad sizes (max_current >= 1, num_rays >= 1, 0 <= rank < world_size)"
                                         : "bad sizes (num_rays >= 1, 0 <= rank < world_size)");
  if (is_live && s->num_current > s->num_fields) return refuse(NGM_E_INVALID, "max_current > num_fields");
  const int32_t T = is_live ? live->num_train_fields : 0, max_obs = T / 2 < s->num_current ? T / 2 : s->num_current;
  const int64_t n_all = is_live ? (T < s->num_fields ? T : s->num_fields) : (int64_t)s->num_observed + s->num_random;
  if (is_live && (s->num_observed != max_obs || s->num_random != n_all))
    return refuse(NGM_E_INVALID, "num_observed / num_random must be their maxima min(T / 2, max_current) / min(T, num_fields)");
  if (!is_live && (s->num_observed < 0 || s->num_observed > s->num_current || s->num_random < 0 ||
                   s->num_random > s->num_fields - s->num_observed))
    return refuse(NGM_E_INVALID, "num_observed <= num_current and num_random <= num_fields - num_observed");
  if (n_all > NGM_TARGET_MAX_DRAW) return refuse(NGM_E_UNSUPPORTED, "more than NGM_TARGET_MAX_DRAW fields drawn");
  const int64_t owned = s->num_fields > s->rank ? ((int64_t)s->num_fields - s->rank + s->world_size - 1) / s->world_size : 0;
  if (s->capacity != (n_all < owned ? n_all : owned))
    return refuse(NGM_E_INVALID, is_live ? "capacity must be min(min(T, num_fields), fields of this rank)"
                                         : "capacity must be min(num_observed + num_random, fields of this rank)");
  if (is_live && (!live->num_current || !live->num_frames || !live->num_observed || !live->num_random))
    return refuse(NGM_E_INVALID, "NULL device count");
  if (((is_live || s->num_current > 0) && !s->current_field_ids) || (s->num_fields > 0 && !s->field_positions) || !s->count ||
      !s->field_ids || (s->num_observed > 0 && !s->subset_observed) || (s->num_random > 0 && !s->subset_random) || !s->offsets ||
      !s->frame_cids || !s->u_xy || (s->iteration < 0 && !s->iteration_dev))
    return refuse(NGM_E_INVALID, "NULL array (iteration < 0 needs iteration_dev)");
  if (!out->ijs || !out->near || !out->far || !out->gt || !out->rgbds || !out->rgb_mask || !out->depth_mask || !out->term_probs ||
      !out->term_mask)
    return refuse(NGM_E_INVALID, "NULL output array");
  if ((int64_t)s->capacity * s->num_rays > INT32_MAX) return refuse(NGM_E_UNSUPPORTED, "capacity x num_rays >= 2^31");
  if (ngm_launch_target_sample_mv(*kf, *s, is_live ? live : nullptr, *out, workspace, workspace_bytes, (hipStream_t)stream, num_fields_dev))
    return refuse(NGM_E_WORKSPACE, "workspace too small");
  return check_launch(fn);
}
int64_t ngm_target_sample_mv_workspace(int32_t num_frames, int32_t num_current, int32_t num_fields, int32_t capacity) {
  if (num_frames < 1 || num_current < 0 || num_fields < 0 || capacity < 0 || capacity > NGM_TARGET_MAX_DRAW) return -1;
  return ngm_target_sample_mv_bytes(num_frames, num_current, num_fields, capacity);
}
int64_t ngm_target_sample_mv_live_workspace(int32_t max_frames, int32_t max_current, int32_t num_fields, int32_t capacity) {
  return max_current < 1 ? -1 : ngm_target_sample_mv_workspace(max_frames, max_current, num_fields, capacity);   // a maximum: >= 1
}
int ngm_target_sample_mv(const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_out* out, void* workspace,
                         int64_t workspace_bytes, void* stream) {
  return target_sample_mv("ngm_target_sample_mv", false, kf, s, nullptr, out, workspace, workspace_bytes, stream);
}
int ngm_target_sample_mv_live(const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_live* live,
                              const ngm_target_out* out, void* workspace, int64_t workspace_bytes, void* stream) {
  return target_sample_mv("ngm_target_sample_mv_live", true, kf, s, live, out, workspace, workspace_bytes, stream);
}
// the grow variant: the live entry point's checks with s->num_fields = max_fields (every maximum follows from it), + the count
int64_t ngm_target_sample_mv_grow_workspace(int32_t max_frames, int32_t max_current, int32_t max_fields, int32_t capacity) {
  return max_fields < 1 ? -1 : ngm_target_sample_mv_live_workspace(max_frames, max_current, max_fields, capacity);
}
int ngm_target_sample_mv_grow(const ngm_keyframes* kf, const ngm_target_sample* s, const ngm_target_live* live,
                              const int32_t* num_fields_dev, const ngm_target_out* out, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  if (!num_fields_dev) return fail(NGM_E_INVALID, "ngm_target_sample_mv_grow: NULL num_fields_dev");
  return target_sample_mv("ngm_target_sample_mv_grow", true, kf, s, live, out, workspace, workspace_bytes, stream, num_fields_dev);
}

int64_t ngm_target_observed_fields_workspace(int32_t height, int32_t width) {
  if (height < 1 || width < 1 || (int64_t)height * width > INT32_MAX) return -1;
  return ngm_target_observed_fields_bytes(height, width);
}
static int observed_fields(const ngm_observed_fields* a, const int32_t* num_fields_dev, void* workspace, int64_t workspace_bytes,
                           void* stream);
int ngm_target_observed_fields(const ngm_observed_fields* a, void* workspace, int64_t workspace_bytes, void* stream) {
  return observed_fields(a, nullptr, workspace, workspace_bytes, stream);
}
int64_t ngm_target_observed_fields_grow_workspace(int32_t height, int32_t width) {
  return ngm_target_observed_fields_workspace(height, width);
}
int ngm_target_observed_fields_grow(const ngm_observed_fields* a, const int32_t* num_fields_dev, void* workspace,
                                    int64_t workspace_bytes, void* stream) {
  if (!num_fields_dev) return fail(NGM_E_INVALID, "ngm_target_observed_fields_grow: NULL num_fields_dev");
  return observed_fields(a, num_fields_dev, workspace, workspace_bytes, stream);
}
// both entry points (the messages keep the first one's name: the checks are its checks)
static int observed_fields(const ngm_observed_fields* a, const int32_t* num_fields_dev, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  if (!a) return fail(NGM_E_INVALID, "ngm_target_observed_fields: NULL argument");
  if (a->height < 1 || a->width < 1 || (int64_t)a->height * a->width > INT32_MAX || a->num_fields < 0 || !(a->radius >= 0.f))
    return fail(NGM_E_INVALID, "ngm_target_observed_fields: bad sizes (H, W >= 1, H x W < 2^31, num_fields >= 0, radius >= 0)");
  if (a->num_points < 1 || a->num_points > NGM_OBSERVED_MAX_POINTS)
    return fail(NGM_E_UNSUPPORTED, "ngm_target_observed_fields: 1 <= num_points <= NGM_OBSERVED_MAX_POINTS");
  if (!a->rgbd || !a->c2w || (a->num_fields > 0 && (!a->field_positions || !a->current_field_ids)) || !a->current_count || !a->pixels ||
      !a->num_used || (a->frame < 0 && !a->frame_dev))
    return fail(NGM_E_INVALID, "ngm_target_observed_fields: NULL array (frame < 0 needs frame_dev)");
  if (ngm_launch_target_observed_fields(*a, workspace, workspace_bytes, (hipStream_t)stream, num_fields_dev))
    return fail(NGM_E_WORKSPACE, "ngm_target_observed_fields: workspace too small");
  return check_launch("ngm_target_observed_fields");
}

int ngm_fields_append(const ngm_fields_append_args* a, void* stream) {
  if (!a) return fail(NGM_E_INVALID, "ngm_fields_append: NULL argument");
  if (a->num_tensors < 0 || a->num_tensors > NGM_APPEND_MAX_TENSORS || (a->num_tensors > 0 && !a->tensors))
    return fail(NGM_E_INVALID, "ngm_fields_append: 0 <= num_tensors <= NGM_APPEND_MAX_TENSORS");
  if (a->max_fields < 1 || a->first < 0 || a->num_new < 0 || (int64_t)a->first + a->num_new > a->max_fields)
    return fail(NGM_E_INVALID, "ngm_fields_append: rows [first, first + num_new) must lie inside [0, max_fields)");
  if (!a->positions || !a->orientations || !a->num_fields_dev || (a->num_new > 0 && (!a->new_positions || !a->new_orientations)))
    return fail(NGM_E_INVALID, "ngm_fields_append: NULL array");
  for (int i = 0; i < a->num_tensors; ++i) {
    const ngm_append_tensor& t = a->tensors[i];
    if (!t.param || !t.prototype || t.numel < 1 || t.stride < t.numel)
      return fail(NGM_E_INVALID, "ngm_fields_append: tensor without param / prototype, or stride < numel");
    if (t.param_lp && t.lp_dtype != NGM_DT_BF16 && t.lp_dtype != NGM_DT_F16)
      return fail(NGM_E_INVALID, "ngm_fields_append: a 16-bit copy is bfloat16 or float16");
  }
  if (a->num_new == 0) return NGM_OK;                    // nothing to add: the count already holds `first`
  ngm_launch_fields_append(*a, (hipStream_t)stream);
  return check_launch("ngm_fields_append");
}

int ngm_fields_repose(const ngm_fields_repose_args* a, void* stream) {
  if (!a) return fail(NGM_E_INVALID, "ngm_fields_repose: NULL argument");
  if (a->num_fields < 0 || a->num_poses < 0) return fail(NGM_E_INVALID, "ngm_fields_repose: num_fields and num_poses must be >= 0");
  if ((a->num_fields > 0 && (!a->positions || !a->orientations || !a->anchor_slot)) ||
      (a->num_poses > 0 && (!a->prev_poses || !a->new_poses)))
    return fail(NGM_E_INVALID, "ngm_fields_repose: NULL array");
  if (a->num_poses == 0) return NGM_OK;                  // no pose table: every anchor is out of range, nothing moves
  ngm_launch_fields_repose(*a, (hipStream_t)stream);
  return check_launch("ngm_fields_repose");
}

int ngm_field_counts_add(const int64_t* field_ids, const int32_t* count, int32_t rows, int64_t* training_iterations, int32_t num_fields,
                         void* stream) {
  if (rows < 0 || num_fields < 0 || (rows > 0 && (!field_ids || !training_iterations)))
    return fail(NGM_E_INVALID, "ngm_field_counts_add: bad argument");
  if (rows == 0 || num_fields == 0) return NGM_OK;
  ngm_launch_field_counts_add(field_ids, count, rows, num_fields, training_iterations, (hipStream_t)stream);
  return check_launch("ngm_field_counts_add");
}

int ngm_target_sv_intersect(int32_t F, int64_t N, const float* field_pos_cam, const float* points_cam, float radius, uint8_t* hit,
                            void* stream) {
  if (F < 0 || N < 0 || radius < 0.f || (F > 0 && N > 0 && (!field_pos_cam || !points_cam || !hit)))
    return fail(NGM_E_INVALID, "ngm_target_sv_intersect: bad argument");
  if (F == 0 || N == 0) return NGM_OK;
  if (F > 65535) return fail(NGM_E_UNSUPPORTED, "ngm_target_sv_intersect: more than 65535 candidate fields");
  ngm_launch_target_sv_intersect(F, N, field_pos_cam, points_cam, radius, hit, (hipStream_t)stream);
  return check_launch("ngm_target_sv_intersect");
}
int ngm_target_sv_rays(int32_t F, int32_t R, const float* field_pos_cam, float radius, const int64_t* pts_ijs, const int64_t* segments,
                       const float* image, int32_t height, int32_t width, float fx, float fy, float cx, float cy,
                       const ngm_target_out* out, void* stream) {
  if (F < 0 || R < 1 || height < 1 || width < 1 || !field_pos_cam || !pts_ijs || !segments || !image || !out || !out->ijs || !out->near ||
      !out->far || !out->gt || !out->rgbds || !out->rgb_mask || !out->depth_mask || !out->term_probs || !out->term_mask)
    return fail(NGM_E_INVALID, "ngm_target_sv_rays: bad argument");
  if (F == 0) return NGM_OK;
  ngm_launch_target_sv_rays(F, R, field_pos_cam, radius, pts_ijs, segments, image, height, width, fx, fy, cx, cy, *out, (hipStream_t)stream);
  return check_launch("ngm_target_sv_rays");
}

// rows a rank can need: min(T, num_active, its fields among num_fields)
static int64_t target_sample_sv_rows(const ngm_target_sample_sv_args* a) {
  const int64_t owned = a->num_fields > a->rank ? ((int64_t)a->num_fields - a->rank + a->world_size - 1) / a->world_size : 0;
  int64_t rows = a->num_train_fields < a->num_active ? a->num_train_fields : a->num_active;
  return rows < owned ? rows : owned;
}
int64_t ngm_target_sample_sv_workspace(int32_t height, int32_t width, int32_t num_active, int32_t num_points, int32_t capacity) {
  if (height < 1 || width < 1 || (int64_t)height * width > INT32_MAX || num_active < 0 || num_points < 1 ||
      num_points > NGM_SV_MAX_POINTS || capacity < 0 || capacity > NGM_TARGET_MAX_DRAW)
    return -1;
  return ngm_target_sample_sv_bytes(height, width, num_active, num_points, capacity);
}
int ngm_target_sample_sv(const ngm_target_sample_sv_args* a, const ngm_target_out* out, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  if (!a || !out) return fail(NGM_E_INVALID, "ngm_target_sample_sv: NULL argument");
  if (a->num_slots < 1 || a->height < 1 || a->width < 1 || (int64_t)a->height * a->width > INT32_MAX || a->num_active < 0 ||
      a->num_fields < 0 || a->num_train_fields < 0 || a->num_rays < 1 || a->capacity < 0 || a->world_size < 1 || a->rank < 0 ||
      a->rank >= a->world_size || a->num_points < 1 || !(a->radius >= 0.f))
    return fail(NGM_E_INVALID, "ngm_target_sample_sv: bad sizes (num_slots, H, W, num_points, num_rays >= 1, H x W < 2^31, "
                               "0 <= rank < world_size, radius >= 0, nothing negative)");
  if (a->num_points > NGM_SV_MAX_POINTS || a->num_train_fields > NGM_TARGET_MAX_DRAW || a->num_rays > NGM_TARGET_MAX_DRAW ||
      a->capacity > NGM_TARGET_MAX_DRAW)
    return fail(NGM_E_INVALID, "ngm_target_sample_sv: num_points <= NGM_SV_MAX_POINTS; num_train_fields, num_rays and capacity <= "
                               "NGM_TARGET_MAX_DRAW");
  if (a->capacity < target_sample_sv_rows(a))
    return fail(NGM_E_INVALID, "ngm_target_sample_sv: capacity must be >= min(num_train_fields, num_active, fields of this rank)");
  if ((a->segments_in && !a->pixels_in) || ((a->pixels_in || a->subset_fields_in || a->segments_in) && a->world_size != 1))
    return fail(NGM_E_INVALID, "ngm_target_sample_sv: segments_in needs pixels_in; recorded draws are for world_size 1");
  if (!a->rgbd || !a->c2w || (a->num_active > 0 && (!a->active_field_ids || !a->hits)) || (a->num_fields > 0 && !a->field_positions) ||
      !a->count || !a->pixels || !a->num_used || !a->num_candidates || (a->num_train_fields > 0 && !a->subset_fields) ||
      (a->capacity > 0 && (!a->field_ids || !a->segments)) || (a->iteration < 0 && !a->iteration_dev))
    return fail(NGM_E_INVALID, "ngm_target_sample_sv: NULL array (iteration < 0 needs iteration_dev)");
  if (a->capacity > 0 && (!out->ijs || !out->near || !out->far || !out->gt || !out->rgbds || !out->rgb_mask || !out->depth_mask ||
                          !out->term_probs || !out->term_mask))
    return fail(NGM_E_INVALID, "ngm_target_sample_sv: NULL output array");
  if (ngm_launch_target_sample_sv(*a, *out, workspace, workspace_bytes, (hipStream_t)stream))
    return fail(NGM_E_WORKSPACE, "ngm_target_sample_sv: workspace too small");
  return check_launch("ngm_target_sample_sv");
}

int ngm_debug_last_bwd_variant(void) { return g_last_bwd.variant; }
int ngm_debug_last_matmul(int which) { return (which >= 0 && which < 3) ? g_last_fwd[which].matmul : -1; }
int ngm_debug_last_fwd_one_tile(void) { return g_last_fwd[NGM_FWD_RENDER].one_tile; }
int ngm_debug_last_comp_fused(void) { return g_last_bwd.fused_comp; }
int ngm_debug_disable_fused_comp(int on) { const int old = g_no_fused_comp; g_no_fused_comp = on ? 1 : 0; return old; }

static unsigned long long* g_debug_cycles_fwd = nullptr;
int ngm_debug_fwd_phase_cycles(unsigned long long* out528) {
  if (!g_debug_cycles_fwd || !out528) return NGM_E_INVALID;
  (void)hipDeviceSynchronize();
  return hipMemcpy(out528, g_debug_cycles_fwd, NGM_FWD_DEBUG_WORDS * 8, hipMemcpyDeviceToHost) == hipSuccess ? NGM_OK : NGM_E_HIP;
}
int ngm_debug_phase_cycles(unsigned long long* out528) {
  if (!g_debug_cycles || !out528) return NGM_E_INVALID;
  (void)hipDeviceSynchronize();
  return hipMemcpy(out528, g_debug_cycles, NGM_FWD_DEBUG_WORDS * 8, hipMemcpyDeviceToHost) == hipSuccess ? NGM_OK : NGM_E_HIP;
}

int ngm_device_info(int* ncu, char* name, int name_len) {
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    (void)hipGetLastError();
    return fail(NGM_E_HIP, "no HIP device");
  }
  if (ncu) *ncu = prop.multiProcessorCount;
  if (name && name_len > 0) snprintf(name, name_len, "%s (%s)", prop.name, prop.gcnArchName);
  return NGM_OK;
}

// ------------------------------------------------------------------------------------------------
int ngm_sample_rays(const ngm_render_cfg* cfg, const ngm_rays* rays, float* points_cam, float* distances, float* dirs,
                    void* stream) {
  if (!cfg || !rays || !rays->ijs) return fail(NGM_E_INVALID, "ngm_sample_rays: NULL argument");
  const int S = cfg->num_samples_coarse + (rays->gt ? cfg->num_samples_guided : 0);
  if (S < 1) return fail(NGM_E_INVALID, "no samples");
  ngm_launch_sampler(cfg, rays, S, points_cam, distances, dirs, nullptr, (hipStream_t)stream);
  return check_launch("ngm_sample_rays");
}

int ngm_sample_rays_world(const ngm_render_cfg* cfg, const ngm_rays* rays, float* points_cam, float* points_world,
                          float* distances, float* dirs, void* stream) {
  if (!cfg || !rays || !rays->ijs) return fail(NGM_E_INVALID, "ngm_sample_rays_world: NULL argument");
  if (points_world && !rays->c2ws) return fail(NGM_E_INVALID, "ngm_sample_rays_world: c2ws required");
  const int S = cfg->num_samples_coarse + (rays->gt ? cfg->num_samples_guided : 0);
  if (S < 1) return fail(NGM_E_INVALID, "no samples");
  ngm_launch_sampler(cfg, rays, S, points_cam, distances, dirs, points_world, (hipStream_t)stream);
  return check_launch("ngm_sample_rays_world");
}

int ngm_sample_rays_weighted(const ngm_render_cfg* cfg, const ngm_rays* rays, int32_t num_bins, const float* boundaries,
                             const float* weights, float* points_cam, float* distances, float* dirs, void* stream) {
  if (!cfg || !rays || !rays->ijs || !boundaries || !weights) return fail(NGM_E_INVALID, "ngm_sample_rays_weighted: NULL argument");
  // camera.py:260-261: "Either both or none of weights and boundaries must be None" -- both are required here; one draw array
  // without the other would mix the reference's two torch.rand streams with the Philox stream
  if ((rays->u_coarse == nullptr) != (rays->u_guided == nullptr))
    return fail(NGM_E_INVALID, "ngm_sample_rays_weighted: u_coarse (bin draws) and u_guided (offset draws) must both be given or both be NULL");
  const int S = cfg->num_samples_coarse;
  if (S < 1 || num_bins < 1) return fail(NGM_E_INVALID, "ngm_sample_rays_weighted: no samples / no bins");
  ngm_launch_sampler_weighted(cfg, rays, S, num_bins, boundaries, weights, points_cam, distances, dirs, (hipStream_t)stream);
  return check_launch("ngm_sample_rays_weighted");
}

// ------------------------------------------------------------------------------------------------
int ngm_encode_fwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                   const float* field_pos, const float* field_quat, float* out, void* stream) {
  int rc = check_field_cfg(fcfg, false);
  if (rc) return rc;
  rc = check_params(fcfg, params);
  if (rc) return rc;
  if (!points || !out || F < 1 || P < 0) return fail(NGM_E_INVALID, "ngm_encode_fwd: bad argument");
  if ((field_pos == nullptr) != (field_quat == nullptr)) return fail(NGM_E_INVALID, "pos/quat must both be given");
  if (P == 0) return NGM_OK;
  rc = ngm_launch_encode_points(*fcfg, *params, F, P, points, field_pos, field_quat, out, (hipStream_t)stream);
  if (rc) return fail(rc, "ngm_encode_fwd: encoding not available as a standalone stage (triplane)");
  return check_launch("ngm_encode_fwd");
}

static int64_t tri_numel(const ngm_field_cfg* fc) {       // floats of one field's planes (3, C, res, res)
  const int64_t C = fc->tri_mode == NGM_TRI_CONCAT ? fc->dim_enc / 3 : fc->dim_enc;
  return 3 * C * fc->tri_resolution * fc->tri_resolution;
}
// The encoding's backward scratch, continuing its holder's arena (render, field-eval backward, encode backward): permutohedral
// dL/dE per sample and level, scaled local positions, per-workgroup table partials; triplane the Q23.40 accumulators
static void hash_scratch_layout(const ngm_field_cfg* fc, int F, int64_t P, FieldBwdArgs& a, WsArena& ws) {
  if (fc->encoding == NGM_ENC_TRIPLANE) { a.tri_numel = tri_numel(fc); a.tri_acc = ws.take<long long>((int64_t)F * a.tri_numel); return; }
  if (fc->encoding != NGM_ENC_PERMUTO) return;
  a.hash_dE = ws.take<float2>((int64_t)fc->nr_levels * F * P);
  a.hash_xyz = ws.take<float4>((int64_t)F * P);
  a.hash_part = ws.take<float>((int64_t)F * fc->nr_levels * 8 * 2 * ((int64_t)1 << fc->log2_hashmap_size));
}

// the standalone encoding backward: the Fourier kernel's per-workgroup partials, or the permutohedral scratch
static void encode_bwd_layout(const ngm_field_cfg* fc, int F, int64_t P, float** fourier_part, FieldBwdArgs& a, WsArena& ws) {
  if (fc->encoding == NGM_ENC_FOURIER) *fourier_part = ws.take<float>(ngm_encode_bwd_fourier_scratch(F, P) / 4);
  if (fc->encoding == NGM_ENC_PERMUTO) hash_scratch_layout(fc, F, P, a, ws);
}
int64_t ngm_encode_bwd_workspace(const ngm_field_cfg* fcfg, int32_t F, int64_t P) {
  if (!fcfg || F < 1 || P < 0) return NGM_E_INVALID;
  float* fourier_part;
  return ws_bytes(encode_bwd_layout, fcfg, F, P, &fourier_part, FieldBwdArgs());
}

int ngm_encode_bwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                   const float* field_pos, const float* field_quat, const float* d_enc, const ngm_grads* grads, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  int rc = check_field_cfg(fcfg, false);
  if (rc) return rc;
  rc = check_params(fcfg, params);
  if (rc) return rc;
  if (!points || !d_enc || !grads || F < 1 || P < 0) return fail(NGM_E_INVALID, "ngm_encode_bwd: bad argument");
  if ((field_pos == nullptr) != (field_quat == nullptr)) return fail(NGM_E_INVALID, "pos/quat must both be given");
  if (fcfg->encoding == NGM_ENC_TRIPLANE)
    return fail(NGM_E_UNSUPPORTED, "ngm_encode_bwd: the triplane encoding has no standalone backward stage (ngm_field_eval_bwd)");
  if (fcfg->encoding != NGM_ENC_PERMUTO && fcfg->encoding != NGM_ENC_FOURIER) return NGM_OK;     // no parameters
  FieldBwdArgs a;
  memset(&a, 0, sizeof(a));
  float* fourier_part = nullptr;
  WsArena ws(workspace);
  encode_bwd_layout(fcfg, F, P, &fourier_part, a, ws);
  if (!workspace || !ws.covers(workspace_bytes)) return fail(NGM_E_WORKSPACE, "ngm_encode_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  if (fcfg->encoding == NGM_ENC_FOURIER) {
    if (!grads->enc_w) return fail(NGM_E_INVALID, "ngm_encode_bwd: grads->enc_w is NULL");
    if (P == 0) {
      const int64_t n = (int64_t)(fcfg->dim_enc - (fcfg->raw_coords ? 3 : 0)) * 3;
      for (int f = 0; f < F; ++f) (void)hipMemsetAsync(grads->enc_w + f * grads->enc_w_stride, 0, 4 * (size_t)n, st);
      return check_launch("ngm_encode_bwd");
    }
    rc = ngm_launch_encode_bwd_fourier(*fcfg, *params, F, P, points, field_pos, field_quat, d_enc, grads->enc_w, grads->enc_w_stride,
                                       fourier_part, st);
    if (rc) return fail(rc, "ngm_encode_bwd: launch failed");
    return check_launch("ngm_encode_bwd");
  }
  if (!grads->lattice) return fail(NGM_E_INVALID, "ngm_encode_bwd: grads->lattice is NULL");
  // refused before the preparation kernel is launched, not after it
  if (!ngm_hash_grad_takes(*fcfg)) return fail(NGM_E_UNSUPPORTED, "ngm_encode_bwd: table size not supported by the table-gradient kernel");
  a.fc = *fcfg; a.pr = *params; a.F = F; a.P = P;
  a.lattice_grad = grads->lattice; a.lattice_grad_stride = grads->lattice_stride;
  if (P == 0) {
    const int64_t n = (int64_t)fcfg->nr_levels * ((int64_t)1 << fcfg->log2_hashmap_size) * 2;
    for (int f = 0; f < F; ++f) (void)hipMemsetAsync(grads->lattice + f * grads->lattice_stride, 0, 4 * (size_t)n, st);
    return check_launch("ngm_encode_bwd");
  }
  rc = ngm_launch_encode_bwd_prep_hash(*fcfg, *params, F, P, points, field_pos, field_quat, d_enc, a.hash_dE, a.hash_xyz, st);
  if (!rc) rc = ngm_launch_hash_grad(a, st);
  if (rc) return fail(rc, "ngm_encode_bwd: table size not supported by the table-gradient kernel");
  return check_launch("ngm_encode_bwd");
}

static int64_t param_pad(const ngm_field_cfg* fc) {
  int64_t e, w[NGM_MAX_LAYERS + 1], b[NGM_MAX_LAYERS + 1];
  return align_up(ngm_param_offsets(fc, &e, w, b), 64);
}

// point-mode backward (a.F, a.blocks_per_field, a.p_pad are set): per-workgroup gradient partials (+ 64 floats), the scratch
static void field_eval_bwd_layout(const ngm_field_cfg* fc, int64_t P, FieldBwdArgs& a, WsArena& ws) {
  a.partials = ws.take<float>((int64_t)a.F * a.blocks_per_field * a.p_pad + 64);
  hash_scratch_layout(fc, a.F, P, a, ws);
}
int64_t ngm_field_eval_bwd_workspace(const ngm_field_cfg* fcfg, int32_t F, int64_t P) {
  if (check_field_cfg(fcfg)) return NGM_E_INVALID;
  FieldBwdArgs a = FieldBwdArgs();
  int64_t per;
  a.F = F; a.p_pad = param_pad(fcfg);
  plan_bwd(F, P, &per, &a.blocks_per_field);
  return ws_bytes(field_eval_bwd_layout, fcfg, P, a);
}

// ---- point evaluation: forward, training forward and backward ------------------------------------------------------------------
// The reference's unchanged _optimization_iteration reaches NeuralFieldSet.forward(use_vmap=True) under autograd.  With a stash
// offered (ABI 11: ngm_field_eval_fwd_train / ngm_field_eval_bwd_stash) the forward writes what the fused step's forward writes
// (ActStash, 256 B per sample and hidden layer) and k_field_bwd_b3 reads it in point mode; without one the backward recomputes.
static BwdPlan plan_points(const ngm_field_cfg* fc, int32_t F, int64_t P, bool stash_offered) { return plan_mlp_bwd(fc, BwdAsk{nullptr, F, P, false, stash_offered}); }
// the point-mode stash: per layer whole 32-sample tiles (+1: a field may start mid-tile) of 64 activations, + 16 floats
static float* field_eval_stash_layout(const ngm_field_cfg* fc, int32_t F, int64_t P, int64_t* layer_stride, WsArena& ws) {
  *layer_stride = align_up((int64_t)F * P, 32) * 64 + 2048;
  return ws.take<float>(fc->num_layers * *layer_stride + 16);
}
int64_t ngm_field_eval_stash_bytes(const ngm_field_cfg* fcfg, int32_t F, int64_t P) {
  if (check_field_cfg(fcfg) || F < 1 || P < 0) return NGM_E_INVALID;
  if (P == 0 || !plan_points(fcfg, F, P, true).stash_kind) return 0;
  int64_t stride;
  return ws_bytes(field_eval_stash_layout, fcfg, F, P, &stride);
}
// stash_offered: ngm_field_eval_fwd_train, which writes the stash or refuses
static int field_eval_fwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                          const float* points, const float* field_pos, const float* field_quat, float* out, bool stash_offered,
                          void* stash, int64_t stash_bytes, void* stream) {
  int rc = check_field_cfg(fcfg);
  if (rc) return rc;
  rc = check_params(fcfg, params);
  if (rc) return rc;
  if (!points || !out || F < 1 || P < 0) return fail(NGM_E_INVALID, "ngm_field_eval_fwd: bad argument");
  if ((field_pos == nullptr) != (field_quat == nullptr)) return fail(NGM_E_INVALID, "pos/quat must both be given");
  if (P == 0) return NGM_OK;
  FwdAsk ask;
  ask.surface = NGM_FWD_POINTS; ask.F = F; ask.n = P;
  const FwdPlan plan = plan_fwd(fcfg, ask);
  if (plan.status) return fail(plan.status, plan.why);
  PointsFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.fc = *fcfg; a.pr = *params; a.F = F; a.P = P; a.points = points; a.pos = field_pos; a.quat = field_quat; a.out = out;
  if (stash_offered) {
    if (ngm_field_eval_stash_bytes(fcfg, F, P) <= 0) return fail(NGM_E_UNSUPPORTED, "ngm_field_eval_fwd_train: no stash-reading backward for this configuration (ngm_field_eval_stash_bytes == 0): use ngm_field_eval_fwd / ngm_field_eval_bwd");
    WsArena ss(stash);
    a.act = field_eval_stash_layout(fcfg, F, P, &a.act_layer_stride, ss);
    if (!stash || !ss.covers(stash_bytes)) return fail(NGM_E_WORKSPACE, "ngm_field_eval_fwd_train: stash too small (ngm_field_eval_stash_bytes)");
  }
  a.per_block = plan.per_block;
  rc = ngm_launch_points_fwd(a, plan, (hipStream_t)stream);
  if (rc) return fail(rc, no_instance);
  g_last_fwd[NGM_FWD_POINTS] = plan;
  return check_launch("ngm_field_eval_fwd");
}
int ngm_field_eval_fwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                       const float* field_pos, const float* field_quat, float* out, void* stream) {
  return field_eval_fwd(fcfg, params, F, P, points, field_pos, field_quat, out, false, nullptr, 0, stream);
}
int ngm_field_eval_fwd_train(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                             const float* field_pos, const float* field_quat, float* out, void* stash, int64_t stash_bytes,
                             void* stream) {
  return field_eval_fwd(fcfg, params, F, P, points, field_pos, field_quat, out, true, stash, stash_bytes, stream);
}

// stash_offered: ngm_field_eval_bwd_stash, which reads the stash or refuses
static int field_eval_bwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P,
                          const float* points, const float* field_pos, const float* field_quat, const float* d_out,
                          const ngm_grads* grads, bool stash_offered, const void* stash, int64_t stash_bytes, void* workspace,
                          int64_t workspace_bytes, void* stream) {
  int rc = check_field_cfg(fcfg);
  if (rc) return rc;
  rc = check_params(fcfg, params);
  if (rc) return rc;
  if (!points || !d_out || !grads || F < 1 || P < 1) return fail(NGM_E_INVALID, "ngm_field_eval_bwd: bad argument");
  if ((field_pos == nullptr) != (field_quat == nullptr)) return fail(NGM_E_INVALID, "pos/quat must both be given");
  const BwdPlan plan = plan_points(fcfg, F, P, stash_offered);
  if (plan.status) return fail(plan.status, plan.why);
  FieldBwdArgs a;
  memset(&a, 0, sizeof(a));
  if (stash_offered) {
    if (!plan.stash_kind) return fail(NGM_E_UNSUPPORTED, "ngm_field_eval_bwd_stash: no stash-reading backward for this configuration");
    WsArena ss(stash);
    a.act = field_eval_stash_layout(fcfg, F, P, &a.act_layer_stride, ss);
    if (!stash || !ss.covers(stash_bytes)) return fail(NGM_E_WORKSPACE, "ngm_field_eval_bwd_stash: stash too small");
  }
  a.F = F; a.blocks_per_field = plan.blocks_per_field; a.p_pad = param_pad(fcfg);
  WsArena ws(workspace);
  field_eval_bwd_layout(fcfg, P, a, ws);
  if (!ws.covers(workspace_bytes) || !workspace) return fail(NGM_E_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  a.fc = *fcfg; a.pr = *params; a.F = F; a.P = P; a.points = points; a.pos = field_pos; a.quat = field_quat;
  a.d_out = reinterpret_cast<const float4*>(d_out);
  a.per_block = plan.per_block;
  rc = check_enc_grads(fcfg, grads, a);
  if (rc) return rc;
  if (a.tri_acc) (void)hipMemsetAsync(a.tri_acc, 0, (size_t)F * a.tri_numel * 8, st);
  rc = launch_mlp_bwd(plan, a, st);
  if (rc) return rc;
  if (fcfg->encoding == NGM_ENC_TRIPLANE) { ngm_launch_tri_finish(a, st); rc = check_launch("ngm_tri_finish"); if (rc) return rc; }
  if (fcfg->encoding == NGM_ENC_PERMUTO) {
    rc = ngm_launch_hash_grad(a, st);
    if (rc) return fail(rc, "permutohedral backward: hash table too large for the LDS-staged scatter");
    rc = check_launch("ngm_hash_grad");
    if (rc) return rc;
  }
  GradReduceArgs g;
  memset(&g.adam, 0, sizeof(g.adam));
  g.fc = *fcfg; g.gr = *grads; g.F = F; g.blocks_per_field = a.blocks_per_field; g.partials = a.partials; g.p_pad = a.p_pad;
  ngm_launch_grad_reduce(g, st);
  return check_launch("ngm_grad_reduce");
}
int ngm_field_eval_bwd(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                       const float* field_pos, const float* field_quat, const float* d_out, const ngm_grads* grads,
                       void* workspace, int64_t workspace_bytes, void* stream) {
  return field_eval_bwd(fcfg, params, F, P, points, field_pos, field_quat, d_out, grads, false, nullptr, 0, workspace, workspace_bytes, stream);
}
int ngm_field_eval_bwd_stash(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t F, int64_t P, const float* points,
                             const float* field_pos, const float* field_quat, const float* d_out, const ngm_grads* grads,
                             const void* stash, int64_t stash_bytes, void* workspace, int64_t workspace_bytes, void* stream) {
  return field_eval_bwd(fcfg, params, F, P, points, field_pos, field_quat, d_out, grads, true, stash, stash_bytes, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------
int ngm_composite_fwd(const ngm_render_cfg* cfg, int64_t N, int32_t S, const float* colors, const float* geoms,
                      const float* dists, const float* depths, const float* neus_isds, float* C, float* D, float* Cvar,
                      float* Dvar, float* term, float* weights, void* stream) {
  if (!cfg || !colors || !geoms || !dists || !depths || N < 0) return fail(NGM_E_INVALID, "ngm_composite_fwd: bad argument");
  if (N == 0) return NGM_OK;
  CompositeArgs a;
  memset(&a, 0, sizeof(a));
  a.rc = *cfg; a.N = N; a.S = S; a.colors = colors; a.geoms = geoms; a.dists = dists; a.depths = depths; a.isds = neus_isds;
  a.C = C; a.D = D; a.Cv = Cvar; a.Dv = Dvar; a.term = term; a.weights = weights;
  const int rc = ngm_launch_composite_fwd(a, (hipStream_t)stream);
  if (rc) return fail(rc, "ngm_composite_fwd: unsupported S (max 1024)");
  return check_launch("ngm_composite_fwd");
}

int ngm_composite_fwd_packed(const ngm_render_cfg* cfg, int64_t N, int32_t S, const float* field_out4, const float* dists,
                             const float* points_cam, float* rgbd, float* Cvar, float* Dvar, float* term, void* stream) {
  if (!cfg || !field_out4 || !dists || !points_cam || N < 0) return fail(NGM_E_INVALID, "ngm_composite_fwd_packed: bad argument");
  if (N == 0) return NGM_OK;
  CompositeArgs a;
  memset(&a, 0, sizeof(a));
  a.rc = *cfg; a.N = N; a.S = S; a.out4 = reinterpret_cast<const float4*>(field_out4); a.pcam = points_cam; a.dists = dists;
  a.rgbd = rgbd; a.Cv = Cvar; a.Dv = Dvar; a.term = term;
  const int rc = ngm_launch_composite_fwd(a, (hipStream_t)stream);
  if (rc) return fail(rc, "ngm_composite_fwd_packed: unsupported S (max 1024)");
  return check_launch("ngm_composite_fwd_packed");
}

int ngm_composite_bwd(const ngm_render_cfg* cfg, int64_t N, int32_t S, const float* colors, const float* geoms,
                      const float* dists, const float* depths, const float* neus_isds, const float* dC, const float* dD,
                      const float* dterm, float* d_colors, float* d_geoms, float* d_neus_isds, void* stream) {
  if (!cfg || !colors || !geoms || !dists || !depths || N < 0) return fail(NGM_E_INVALID, "ngm_composite_bwd: bad argument");
  if (N == 0) return NGM_OK;
  CompositeArgs a;
  memset(&a, 0, sizeof(a));
  a.rc = *cfg; a.N = N; a.S = S; a.colors = colors; a.geoms = geoms; a.dists = dists; a.depths = depths; a.isds = neus_isds;
  a.dC = dC; a.dD = dD; a.dterm = dterm; a.d_colors = d_colors; a.d_geoms = d_geoms; a.d_isds = d_neus_isds;
  const int rc = ngm_launch_composite_bwd(a, (hipStream_t)stream);
  if (rc) return fail(rc, "ngm_composite_bwd: S > 1024");
  return check_launch("ngm_composite_bwd");
}

// ------------------------------------------------------------------------------------------------
// fused render / train step
// ------------------------------------------------------------------------------------------------
struct RenderPlan {
  int S;
  FwdPlan fwd;                     // the fused forward: instance, launch shape, LDS
  BwdPlan bwd;                     // train: the MLP backward this workspace is carved for, and the stash the forward writes for it
  int64_t p_pad;
  int64_t off_rayseed;             // (F*R, 8) per-ray loss derivatives without the normalisers (fused compositing backward)
  int64_t off_raytab, off_stashA, off_stashB, off_losspart, off_gradpart, off_hash, off_act, act_layer_stride, total;
  int64_t off_dout, off_disd;      // neus: separate per-sample gradient buffer, per-ray d loss / d isd
  char* base;                      // the workspace's aligned base the offsets count from (null when only sizing)
};
// ask: the backward's seed mode and the forward's per-workspace records (ngm_render_bwd*); the forward and the sizing leave it empty.
// workspace: the caller's, or null for the size query; enc: the backward's record, which receives the encoding's scratch
static RenderPlan plan_render(const ngm_field_cfg* fc, const ngm_render_cfg* rc, int F, int R, bool guided, bool train,
                              BwdAsk ask = BwdAsk(), bool counted = false, const void* workspace = nullptr,
                              FieldBwdArgs* enc = nullptr) {
  RenderPlan p = RenderPlan();
  p.S = rc->num_samples_coarse + (guided ? rc->num_samples_guided : 0);
  FwdAsk fq;
  fq.rc = rc; fq.F = F; fq.n = R; fq.S = p.S; fq.counted = counted;
  p.fwd = plan_fwd(fc, fq);
  p.p_pad = param_pad(fc);
  WsArena ws(workspace);
  p.base = ws.base();
  if (train) {
    const int64_t NR = (int64_t)F * R, NS = NR * p.S;
    p.off_raytab = ws.offset(); ws.take<float>(NR * 8);
    p.off_rayseed = ws.offset(); ws.take<float>(NR * 8);
    p.off_stashA = ws.offset(); ws.take<float4>(NS);
    p.off_stashB = ws.offset(); ws.take<float2>(NS);
    p.off_losspart = ws.offset(); ws.take<float>((int64_t)p.fwd.blocks * NGM_NUM_LOSS_SUMS);
    if (rc->geometry_mode == NGM_GEO_NEUS) {
      p.off_dout = ws.offset(); ws.take<float4>(NS);
      p.off_disd = ws.offset(); ws.take<float>(NR);
    }
    ask.rc = rc; ask.F = F; ask.P = (int64_t)R * p.S;
    p.bwd = plan_mlp_bwd(fc, ask);
    p.off_gradpart = ws.offset(); ws.take<float>((int64_t)F * p.bwd.blocks_per_field * p.p_pad);
    p.off_hash = ws.offset();
    FieldBwdArgs none;
    hash_scratch_layout(fc, F, (int64_t)R * p.S, enc ? *enc : none, ws);
    if (p.bwd.stash_kind) {     // floats per layer: whole 32-sample tiles (+1: a field may start mid-tile) of 64 activations / 32 features
      p.act_layer_stride = p.bwd.stash_kind == 1 ? align_up(NS, 32) * 64 + 2048 : align_up(NS, 32) * 32 + 1024;
      p.off_act = ws.offset(); ws.take<float>(p.bwd.stash_layers * p.act_layer_stride + 16);
    }
  }
  p.total = ws.bytes();
  return p;
}

int64_t ngm_render_workspace(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t F, int32_t R, int32_t train) {
  const int e = check_field_cfg(fcfg);                 // NGM_E_UNSUPPORTED for a configuration no kernel takes
  if (e) return e;
  if (!rcfg || F < 1 || R < 1) return NGM_E_INVALID;
  // sized for the guided case (S_c + S_g), the larger of the two
  return plan_render(fcfg, rcfg, F, R, true, train != 0).total;
}

// The encoding's gradient tensors, validated before anything launches.  permutohedral: the table is fully overwritten by
// k_hash_reduce (no zero-fill); triplane: the caller zeroes a.tri_acc on the stream before the MLP backward.
static int check_enc_grads(const ngm_field_cfg* fc, const ngm_grads* grads, FieldBwdArgs& a) {
  if (fc->encoding == NGM_ENC_TRIPLANE) {
    if (!grads->planes || grads->planes_stride < tri_numel(fc)) return fail(NGM_E_INVALID, "triplane: grads.planes missing / stride too small");
    if (!a.tri_acc) return fail(NGM_E_WORKSPACE, "triplane: no accumulator scratch");
    a.planes_grad = grads->planes; a.planes_grad_stride = grads->planes_stride;
    return NGM_OK;
  }
  if (fc->encoding != NGM_ENC_PERMUTO) return NGM_OK;
  if (!grads->lattice) return fail(NGM_E_INVALID, "permutohedral: grads.lattice is NULL");
  const int64_t per = (int64_t)fc->nr_levels * ((int64_t)1 << fc->log2_hashmap_size) * 2;
  if (grads->lattice_stride < per) return fail(NGM_E_INVALID, "permutohedral: grads.lattice_stride too small");
  a.lattice_grad = grads->lattice; a.lattice_grad_stride = grads->lattice_stride;
  return NGM_OK;
}

static int check_render(const ngm_field_cfg* fc, const ngm_render_cfg* rc, const ngm_params* pr, const ngm_rays* rays) {
  int e = check_field_cfg(fc);
  if (e) return e;
  e = check_params(fc, pr);
  if (e) return e;
  if (!rc || !rays || !rays->ijs || !rays->c2ws || !rays->field_pos || !rays->field_quat)
    return fail(NGM_E_INVALID, "render: NULL ray argument");
  if (rays->F < 1 || rays->R < 1) return fail(NGM_E_INVALID, "render: empty batch");
  if (rc->geometry_mode == NGM_GEO_NEUS && !pr->neus_sd)
    return fail(NGM_E_INVALID, "fused render: the neus geometry mode needs params.neus_sd (the per-field _neus_sd, rm.py:641-644)");
  const int S = rc->num_samples_coarse + (rays->gt ? rc->num_samples_guided : 0);
  if (S < 1 || S > 1024) return fail(NGM_E_UNSUPPORTED, "fused render: samples per ray must be in [1,1024]");
  return NGM_OK;
}

// The counted step (ngm_render_*_counted): launched at the capacity rays->F, every kernel learns the number of active rows
// from device memory.  Outside it: the configurations that run extra launches over all F rows (neus: neighbour stencil +
// ngm_launch_neus_sd_grad; triplane: accumulator memset + ngm_launch_tri_finish) and the variance-weighted loss modes.
// These two checks come first and read nothing but the two configurations.
static int check_counted(const char* who, const ngm_field_cfg* fc, const ngm_render_cfg* rc, const int32_t* num_active) {
  char msg[256];
  if (!num_active) {
    snprintf(msg, sizeof(msg), "%s: num_active is NULL (the un-suffixed entry point is the call for all F rows)", who);
    return fail(NGM_E_INVALID, msg);
  }
  const char* why = nullptr;
  if (rc && rc->geometry_mode == NGM_GEO_NEUS) why = "the neus geometry mode";
  else if (fc && fc->encoding == NGM_ENC_TRIPLANE) why = "the triplane encoding";
  else if (rc && (rc->photometric_mode == NGM_PHOTO_GAUSSIAN_NLL || rc->depth_mode != NGM_DEPTH_HUBER)) why = "the *_nll loss modes";
  if (why) {
    snprintf(msg, sizeof(msg), "%s: %s is outside the counted step (it launches over all F rows): slice the batch to its count and call the un-suffixed entry point", who, why);
    return fail(NGM_E_UNSUPPORTED, msg);
  }
  return NGM_OK;
}

static int render_fwd_impl(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                           const ngm_targets* targets, const ngm_prediction* pred, float* loss_sums, void* workspace,
                           int64_t workspace_bytes, void* stream, const int32_t* num_active) {
  int e = check_render(fcfg, rcfg, params, rays);
  if (e) return e;
  if (!pred) return fail(NGM_E_INVALID, "render_fwd: pred is NULL");
  const bool has_tg = targets != nullptr;
  const bool save = workspace != nullptr;   // keep the per-sample stash for a later backward
  if (has_tg && (!targets->rgbds || !targets->depth_mask)) return fail(NGM_E_INVALID, "render_fwd: incomplete targets");
  if (has_tg && targets->term_mask && !targets->term_probs) return fail(NGM_E_INVALID, "render_fwd: term_mask without term_probs");
  if (has_tg && !save) return fail(NGM_E_WORKSPACE, "render_fwd: targets need a workspace");
  if (save && (!pred->rgbds || !pred->term_probs)) return fail(NGM_E_INVALID, "render_fwd(save): pred.rgbds/term_probs required");
  const RenderPlan p = plan_render(fcfg, rcfg, rays->F, rays->R, rays->gt != nullptr, save, BwdAsk(), num_active != nullptr, workspace);
  if (p.fwd.status) return fail(p.fwd.status, p.fwd.why);
  if (save && workspace_bytes < p.total) return fail(NGM_E_WORKSPACE, "render_fwd: workspace too small");
  char* ws = p.base;
  RenderFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.fc = *fcfg; a.pr = *params; a.rc = *rcfg; a.rays = *rays; a.pred = *pred;
  a.fc.matmul_mode = p.fwd.matmul;                                    // AUTO resolved by the plan (LDS budget of this batch shape)
  if (p.fwd.neus) { a.neus_sd = params->neus_sd; a.neus_sd_stride = params->neus_sd_stride; }
  a.has_targets = has_tg ? 1 : 0;
  a.num_active = num_active;
  if (has_tg) a.tg = *targets;
  a.S = p.S; a.rays_per_block = p.fwd.rays_per_block; a.waves_per_block = p.fwd.waves; a.maxs = p.fwd.maxs;
  if (save) {
    a.raytab = reinterpret_cast<float*>(ws + p.off_raytab);
    if (has_tg) a.rayseed = reinterpret_cast<float*>(ws + p.off_rayseed);
    a.stashA = reinterpret_cast<float4*>(ws + p.off_stashA);
    a.stashB = reinterpret_cast<float2*>(ws + p.off_stashB);
    a.loss_partials = reinterpret_cast<float*>(ws + p.off_losspart);
    if (p.act_layer_stride) { a.act = reinterpret_cast<float*>(ws + p.off_act); a.act_layer_stride = p.act_layer_stride; }
    a.act_layers = p.bwd.half;
    static const bool timing = getenv("NGM_PHASE_TIMING") != nullptr;
    if (timing) {
      if (!g_debug_cycles_fwd) { (void)hipMalloc(&g_debug_cycles_fwd, NGM_FWD_DEBUG_WORDS * 8); (void)hipMemset(g_debug_cycles_fwd, 0, NGM_FWD_DEBUG_WORDS * 8); }
      a.debug_cycles = g_debug_cycles_fwd;
    }
  }
  e = ngm_launch_render_fwd(a, p.fwd, (hipStream_t)stream);
  if (e) return fail(e, no_instance);
  g_last_fwd[NGM_FWD_RENDER] = p.fwd;
  if (save) {
    note_forward_stash(workspace, p.bwd.half);
    note_forward_seeds(workspace, a.rayseed ? targets->rgbds : nullptr);
  }
  e = check_launch("ngm_render_fwd");
  if (e) return e;
  if (has_tg && loss_sums) {      // loss_sums == NULL: deferred -- ngm_render_bwd* (loss_sums == NULL) reduces the partials itself
    ngm_launch_loss_reduce(a.loss_partials, p.fwd.blocks, loss_sums,
                           (rays->philox_offset_autoinc && rays->philox_offset_dev) ? const_cast<uint64_t*>(rays->philox_offset_dev) : nullptr,
                           (hipStream_t)stream);
    e = check_launch("ngm_loss_reduce");
  }
  return e;
}
int ngm_render_fwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                   const ngm_targets* targets, const ngm_prediction* pred, float* loss_sums, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  return render_fwd_impl(fcfg, rcfg, params, rays, targets, pred, loss_sums, workspace, workspace_bytes, stream, nullptr);
}
int ngm_render_fwd_counted(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                           const ngm_targets* targets, const ngm_prediction* pred, float* loss_sums, void* workspace,
                           int64_t workspace_bytes, void* stream, const int32_t* num_active) {
  const int e = check_counted("ngm_render_fwd_counted", fcfg, rcfg, num_active);
  if (e) return e;
  return render_fwd_impl(fcfg, rcfg, params, rays, targets, pred, loss_sums, workspace, workspace_bytes, stream, num_active);
}

static int render_bwd_common(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params,
                             const ngm_rays* rays, StashBwdArgs& sb, const ngm_grads* grads, void* workspace,
                             int64_t workspace_bytes, hipStream_t st, const GradAdam* adam = nullptr,
                             const GradAdam* lattice_adam = nullptr, bool* lattice_adam_applied = nullptr,
                             const int32_t* num_active = nullptr) {
  // the plan and every argument check first: a refusal launches nothing
  BwdAsk ask;      // with what the forward on THIS workspace wrote
  ask.seeded = sb.seed_mode != 0; ask.rec_layers = forward_stash_layers(workspace); ask.seeds_written = forward_wrote_seeds_for(workspace, sb.tg.rgbds);
  FieldBwdArgs a;
  memset(&a, 0, sizeof(a));
  const RenderPlan p = plan_render(fcfg, rcfg, rays->F, rays->R, rays->gt != nullptr, true, ask, false, workspace, &a);
  if (p.bwd.status) return fail(p.bwd.status, p.bwd.why);
  if (!workspace || workspace_bytes < p.total) return fail(NGM_E_WORKSPACE, "render_bwd: workspace too small");
  const bool nll_loss = rcfg->photometric_mode == NGM_PHOTO_GAUSSIAN_NLL || rcfg->depth_mode != NGM_DEPTH_HUBER;
  if (nll_loss && sb.seed_mode == 0 && (!sb.pred.color_vars || !sb.pred.depth_vars))
    return fail(NGM_E_INVALID, "render_bwd: the *_nll loss modes need pred.color_vars and pred.depth_vars");
  char* ws = p.base;
  a.fc = *fcfg; a.pr = *params; a.F = rays->F; a.P = (int64_t)rays->R * p.S; a.S = p.S;
  a.num_active = num_active;
  int e = check_enc_grads(fcfg, grads, a);
  if (e) return e;
  sb.rc = *rcfg; sb.F = rays->F; sb.R = rays->R; sb.S = p.S;
  sb.num_active = num_active;
  if (!rays->gt) sb.rc.w_freespace = sb.rc.w_tsdf = 0.f;       // no gt: the reference forms no free-space / TSDF terms (rm.py:624, 632)
  sb.stashA = reinterpret_cast<float4*>(ws + p.off_stashA);
  sb.stashB = reinterpret_cast<const float2*>(ws + p.off_stashB);
  sb.raytab = reinterpret_cast<const float*>(ws + p.off_raytab);
  const bool neus = rcfg->geometry_mode == NGM_GEO_NEUS;
  if (neus) {
    sb.neus_sd = params->neus_sd; sb.neus_sd_stride = params->neus_sd_stride; sb.field_index = params->field_index;
    sb.d_out = reinterpret_cast<float4*>(ws + p.off_dout);
    sb.d_isd_rays = reinterpret_cast<float*>(ws + p.off_disd);
  }
  if (sb.seed_mode == 0 && !sb.loss_sums) {      // deferred loss reduction: the forward left its partials in the workspace
    sb.loss_partials = reinterpret_cast<const float*>(ws + p.off_losspart);
    sb.n_partials = p.fwd.blocks;
    sb.counter = (rays->philox_offset_autoinc && rays->philox_offset_dev)
                     ? reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(rays->philox_offset_dev)) : nullptr;
  }
  a.per_block = p.bwd.per_block; a.blocks_per_field = p.bwd.blocks_per_field;
  a.raytab = sb.raytab; a.stashB = sb.stashB; a.d_out = neus ? sb.d_out : sb.stashA;
  a.partials = reinterpret_cast<float*>(ws + p.off_gradpart); a.p_pad = p.p_pad;
  if (p.bwd.stash_kind) { a.act = reinterpret_cast<const float*>(ws + p.off_act); a.act_layer_stride = p.act_layer_stride; a.act_half = p.bwd.half; }
  if (p.bwd.fused_comp) {
    // d_out holds the forward's stash untouched (hash encoding: k_hash_mlp_bwd writes the positions k_hash_grad needs itself)
    a.fused_comp = 1; a.rc = sb.rc;
    a.rayseed = reinterpret_cast<const float*>(ws + p.off_rayseed);
    a.loss_sums = sb.loss_sums; a.loss_partials = sb.loss_partials; a.n_partials = sb.n_partials;
    a.sums_out = sb.sums_out; a.loss_out = sb.loss_out; a.counter = sb.counter;
  } else {
    // k_stash_bwd runs first and leaves dL/d(raw outputs) in place of the forward's stash
    sb.xyz_out = a.hash_xyz;                 // positions for the table-gradient kernel (hash encoding)
    a.hash_xyz_ready = a.hash_xyz != nullptr;
    e = ngm_launch_stash_bwd(sb, st);
    if (e) return fail(e, "render_bwd: unsupported geometry mode");
    e = check_launch("ngm_stash_bwd");
    if (e) return e;
  }
  if (neus && grads->neus_sd)
    ngm_launch_neus_sd_grad(sb.d_isd_rays, rays->F, rays->R, params->neus_sd, params->neus_sd_stride, params->field_index,
                            grads->neus_sd, st);
  if (a.tri_acc) (void)hipMemsetAsync(a.tri_acc, 0, (size_t)a.F * a.tri_numel * 8, st);
  e = launch_mlp_bwd(p.bwd, a, st);
  if (e) return e;
  if (fcfg->encoding == NGM_ENC_TRIPLANE) { ngm_launch_tri_finish(a, st); e = check_launch("ngm_tri_finish"); if (e) return e; }
  GradReduceArgs g;
  memset(&g.adam, 0, sizeof(g.adam));
  if (adam) g.adam = *adam;
  g.num_active = num_active;
  g.fc = *fcfg; g.gr = *grads; g.F = rays->F; g.blocks_per_field = a.blocks_per_field; g.partials = a.partials; g.p_pad = a.p_pad;
  bool mlp_reduced = false;
  if (fcfg->encoding == NGM_ENC_PERMUTO) {
    if (lattice_adam) a.lattice_adam = *lattice_adam;
    // the MLP's reduction + Adam rides along in the table-gradient launch (both depend on the MLP backward only)
    e = ngm_launch_hash_grad(a, st, lattice_adam_applied, &g, &mlp_reduced);
    if (e == NGM_E_INVALID) return fail(e, "render_bwd_adam: adam tensors do not match the parameter segments");
    if (e) return fail(e, "permutohedral backward: hash table too large for the LDS-staged scatter");
    e = check_launch("ngm_hash_grad");
    if (e) return e;
  }
  if (mlp_reduced) return NGM_OK;
  if (ngm_launch_grad_reduce(g, st)) return fail(NGM_E_INVALID, "render_bwd_adam: adam tensors do not match the parameter segments");
  return check_launch("ngm_grad_reduce");
}

static int render_bwd_impl(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                           const ngm_targets* targets, const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                           float* loss_out, void* workspace, int64_t workspace_bytes, void* stream, const int32_t* num_active) {
  int e = check_render(fcfg, rcfg, params, rays);
  if (e) return e;
  if (!targets || !targets->rgbds || !targets->depth_mask || !pred || !pred->rgbds || !pred->term_probs || !grads)
    return fail(NGM_E_INVALID, "render_bwd: NULL argument");
  StashBwdArgs sb;
  memset(&sb, 0, sizeof(sb));
  sb.seed_mode = 0; sb.tg = *targets; sb.pred = *pred; sb.loss_sums = loss_sums;
  sb.loss_out = loss_out;      // written by the compositing-backward kernel (no separate launch)
  return render_bwd_common(fcfg, rcfg, params, rays, sb, grads, workspace, workspace_bytes, (hipStream_t)stream, nullptr, nullptr,
                           nullptr, num_active);
}
int ngm_render_bwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                   const ngm_targets* targets, const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                   float* loss_out, void* workspace, int64_t workspace_bytes, void* stream) {
  return render_bwd_impl(fcfg, rcfg, params, rays, targets, pred, loss_sums, grads, loss_out, workspace, workspace_bytes, stream,
                         nullptr);
}
int ngm_render_bwd_counted(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                           const ngm_targets* targets, const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                           float* loss_out, void* workspace, int64_t workspace_bytes, void* stream, const int32_t* num_active) {
  const int e = check_counted("ngm_render_bwd_counted", fcfg, rcfg, num_active);
  if (e) return e;
  return render_bwd_impl(fcfg, rcfg, params, rays, targets, pred, loss_sums, grads, loss_out, workspace, workspace_bytes, stream,
                         num_active);
}

static int render_bwd_adam_impl(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                                const ngm_targets* targets, const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                                const ngm_adam_tensor* mlp_tensors, int32_t num_mlp_tensors, const ngm_adam_tensor* lattice_tensor,
                                const int64_t* field_index, int64_t step, int64_t* step_dev, float lr, float beta1, float beta2,
                                float eps, float weight_decay, float* loss_out, void* workspace, int64_t workspace_bytes,
                                void* stream, const int32_t* num_active) {
  int e = check_render(fcfg, rcfg, params, rays);
  if (e) return e;
  if (!targets || !targets->rgbds || !targets->depth_mask || !pred || !pred->rgbds || !pred->term_probs || !grads ||
      !mlp_tensors || num_mlp_tensors < 1 || (step < 1 && !step_dev))
    return fail(NGM_E_INVALID, "render_bwd_adam: bad argument");
  if ((fcfg->encoding == NGM_ENC_PERMUTO) != (lattice_tensor != nullptr))
    return fail(NGM_E_INVALID, "render_bwd_adam: lattice_tensor goes with the permutohedral encoding");
  StashBwdArgs sb;
  memset(&sb, 0, sizeof(sb));
  sb.seed_mode = 0; sb.tg = *targets; sb.pred = *pred; sb.loss_sums = loss_sums;
  sb.loss_out = loss_out;
  GradAdam ad;
  ad.tensors = mlp_tensors; ad.num = num_mlp_tensors;
  ad.hyper = AdamHyper{field_index, step_dev, step, lr, beta1, beta2, eps, weight_decay};
  if (lattice_tensor && (!lattice_tensor->param || !lattice_tensor->exp_avg || !lattice_tensor->exp_avg_sq || !lattice_tensor->grad))
    return fail(NGM_E_INVALID, "render_bwd_adam: NULL lattice tensor");
  GradAdam lad = ad;
  lad.tensors = lattice_tensor; lad.num = lattice_tensor ? 1 : 0;
  bool lattice_done = false;
  e = render_bwd_common(fcfg, rcfg, params, rays, sb, grads, workspace, workspace_bytes, (hipStream_t)stream, &ad,
                        lattice_tensor ? &lad : nullptr, &lattice_done, num_active);
  if (e) return e;
  if (lattice_tensor && !lattice_done) {   // unaligned tables: k_hash_reduce left the update to a plain Adam launch
    ngm_launch_adam_multi(lattice_tensor, 1, rays->F, ad.hyper, nullptr, nullptr, (hipStream_t)stream, num_active);
    e = check_launch("ngm_adam_sparse_multi");
  }
  return e;
}
int ngm_render_bwd_adam(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                        const ngm_targets* targets, const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                        const ngm_adam_tensor* mlp_tensors, int32_t num_mlp_tensors, const ngm_adam_tensor* lattice_tensor,
                        const int64_t* field_index, int64_t step, int64_t* step_dev, float lr, float beta1, float beta2,
                        float eps, float weight_decay, float* loss_out, void* workspace, int64_t workspace_bytes, void* stream) {
  return render_bwd_adam_impl(fcfg, rcfg, params, rays, targets, pred, loss_sums, grads, mlp_tensors, num_mlp_tensors, lattice_tensor,
                              field_index, step, step_dev, lr, beta1, beta2, eps, weight_decay, loss_out, workspace, workspace_bytes,
                              stream, nullptr);
}
int ngm_render_bwd_adam_counted(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, const ngm_rays* rays,
                                const ngm_targets* targets, const ngm_prediction* pred, const float* loss_sums, const ngm_grads* grads,
                                const ngm_adam_tensor* mlp_tensors, int32_t num_mlp_tensors, const ngm_adam_tensor* lattice_tensor,
                                const int64_t* field_index, int64_t step, int64_t* step_dev, float lr, float beta1, float beta2,
                                float eps, float weight_decay, float* loss_out, void* workspace, int64_t workspace_bytes,
                                void* stream, const int32_t* num_active) {
  const int e = check_counted("ngm_render_bwd_adam_counted", fcfg, rcfg, num_active);
  if (e) return e;
  return render_bwd_adam_impl(fcfg, rcfg, params, rays, targets, pred, loss_sums, grads, mlp_tensors, num_mlp_tensors, lattice_tensor,
                              field_index, step, step_dev, lr, beta1, beta2, eps, weight_decay, loss_out, workspace, workspace_bytes,
                              stream, num_active);
}

int ngm_render_bwd_seeded_vars(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params,
                               const ngm_rays* rays, const ngm_prediction* pred, const float* d_rgbds, const float* d_color_vars,
                               const float* d_depth_vars, const float* d_term, const float* d_geom_samples,
                               const ngm_grads* grads, void* workspace, int64_t workspace_bytes, void* stream) {
  int e = check_render(fcfg, rcfg, params, rays);
  if (e) return e;
  if (!d_rgbds || !grads) return fail(NGM_E_INVALID, "render_bwd_seeded: NULL argument");
  if ((d_color_vars || d_depth_vars) && (!pred || !pred->rgbds || !pred->term_probs))
    return fail(NGM_E_INVALID, "render_bwd_seeded_vars: seeds on the variances need the forward's pred.rgbds and pred.term_probs");
  StashBwdArgs sb;
  memset(&sb, 0, sizeof(sb));
  sb.seed_mode = 1; sb.d_rgbds = d_rgbds; sb.d_term = d_term; sb.d_geom_samples = d_geom_samples;
  sb.d_cvars = d_color_vars; sb.d_dvars = d_depth_vars;
  if (pred) sb.pred = *pred;
  return render_bwd_common(fcfg, rcfg, params, rays, sb, grads, workspace, workspace_bytes, (hipStream_t)stream);
}

int ngm_render_bwd_seeded(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params,
                          const ngm_rays* rays, const float* d_rgbds, const float* d_term, const float* d_geom_samples,
                          const ngm_grads* grads, void* workspace, int64_t workspace_bytes, void* stream) {
  return ngm_render_bwd_seeded_vars(fcfg, rcfg, params, rays, nullptr, d_rgbds, nullptr, nullptr, d_term, d_geom_samples, grads,
                                    workspace, workspace_bytes, stream);
}

int ngm_render_read_samples(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t F, int32_t R, int32_t S,
                            const void* workspace, float* geoms, float* dists, void* stream) {
  if (check_field_cfg(fcfg) || !rcfg || !workspace) return fail(NGM_E_INVALID, "render_read_samples: bad argument");
  // S tells which plan the forward ran with (it plans from rays->gt): the stash offsets and the copy size depend on it
  const bool guided = S != rcfg->num_samples_coarse;
  if (S != rcfg->num_samples_coarse + (guided ? rcfg->num_samples_guided : 0))
    return fail(NGM_E_INVALID, "render_read_samples: S is neither S_c nor S_c + S_g of this render cfg");
  const RenderPlan p = plan_render(fcfg, rcfg, F, R, guided, true, BwdAsk(), false, workspace);
  const char* ws = p.base;
  ngm_launch_read_stash(reinterpret_cast<const float4*>(ws + p.off_stashA), reinterpret_cast<const float2*>(ws + p.off_stashB),
                        (int64_t)F * R * p.S, geoms, dists, (hipStream_t)stream);
  return check_launch("ngm_render_read_samples");
}

// ------------------------------------------------------------------------------------------------
int ngm_adam_sparse(float* param, float* exp_avg, float* exp_avg_sq, int64_t stride, const float* grad,
                    int64_t grad_stride, const int64_t* field_index, int32_t F, int64_t numel_per_field, int64_t step,
                    float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
  if (!param || !exp_avg || !exp_avg_sq || !grad || F < 1 || numel_per_field < 1 || step < 1)
    return fail(NGM_E_INVALID, "ngm_adam_sparse: bad argument");
  ngm_launch_adam(param, exp_avg, exp_avg_sq, stride, grad, grad_stride, F, numel_per_field,
                  AdamHyper{field_index, nullptr, step, lr, beta1, beta2, eps, weight_decay}, (hipStream_t)stream);
  return check_launch("ngm_adam_sparse");
}

int ngm_adam_sparse_multi(const ngm_adam_tensor* tensors, int32_t num_tensors, const int64_t* field_index, int32_t F,
                          int64_t step, int64_t* step_dev, float lr, float beta1, float beta2, float eps,
                          float weight_decay, int32_t advance_step_dev, uint64_t* advance_philox_offset_dev, void* stream) {
  if (!tensors || num_tensors < 1 || num_tensors > 2 * (NGM_MAX_LAYERS + 1) + 2 || F < 1 || (step < 1 && !step_dev))
    return fail(NGM_E_INVALID, "ngm_adam_sparse_multi: bad argument");
  for (int i = 0; i < num_tensors; ++i)
    if (!tensors[i].param || !tensors[i].exp_avg || !tensors[i].exp_avg_sq || !tensors[i].grad || tensors[i].numel < 1)
      return fail(NGM_E_INVALID, "ngm_adam_sparse_multi: NULL tensor");
  ngm_launch_adam_multi(tensors, num_tensors, F, AdamHyper{field_index, step_dev, step, lr, beta1, beta2, eps, weight_decay},
                        (advance_step_dev && step_dev) ? step_dev : nullptr, advance_philox_offset_dev, (hipStream_t)stream);
  return check_launch("ngm_adam_sparse_multi");
}

int ngm_step_advance(int64_t* step_dev, uint64_t* philox_offset_dev, void* stream) {
  ngm_launch_step_advance(step_dev, philox_offset_dev, (hipStream_t)stream);
  return check_launch("ngm_step_advance");
}

static FwdPlan plan_knn(const ngm_field_cfg* fc) {
  FwdAsk ask;
  ask.surface = NGM_FWD_KNN;
  return plan_fwd(fc, ask);
}
int64_t ngm_field_eval_knn_workspace(int32_t num_fields, int64_t P, int32_t num_knn) {
  const int K = num_knn < num_fields ? num_knn : num_fields;
  if (num_fields < 1 || P < 0 || K < 1) return NGM_E_INVALID;
  return ngm_knn_workspace_bytes(num_fields, P, K);
}

int ngm_field_eval_knn(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t num_fields, int64_t P,
                       const float* points, const float* field_pos, const float* field_quat, int32_t num_knn,
                       float distance_factor, float outside_value, float mask_radius, float* out, void* workspace,
                       int64_t workspace_bytes, void* stream) {
  int e = check_field_cfg(fcfg);
  if (e) return e;
  e = check_params(fcfg, params);
  if (e) return e;
  if (!points || !field_pos || !field_quat || !out || num_fields < 1 || P < 0) return fail(NGM_E_INVALID, "ngm_field_eval_knn: bad argument");
  if (P == 0) return NGM_OK;
  const int K = num_knn < num_fields ? num_knn : num_fields;
  if (K < 1 || K > 16) return fail(NGM_E_UNSUPPORTED, "ngm_field_eval_knn: K must be in [1,16]");
  const FwdPlan plan = plan_knn(fcfg);         // the evaluation is planned before the grid build and the assignment launch
  if (plan.status) return fail(plan.status, plan.why);
  e = ngm_launch_knn(fcfg, params, num_fields, P, points, field_pos, field_quat, K, distance_factor, outside_value,
                     mask_radius > 0.f ? mask_radius : fcfg->field_radius, out, workspace, workspace_bytes, plan, (hipStream_t)stream);
  if (e == NGM_E_WORKSPACE) return fail(e, "ngm_field_eval_knn: workspace too small");
  if (e) return fail(e, "ngm_field_eval_knn: not available for this configuration");
  g_last_fwd[NGM_FWD_KNN] = plan;
  return check_launch("ngm_field_eval_knn");
}

// the lattice entry's argument checks, shared by the workspace query and the call: 0, or the status; *K, *P on success
static int grid_knn_shape(int32_t num_fields, int32_t nx, int32_t ny, int32_t nz, int32_t num_knn, int* K, int64_t* P) {
  if (nx < 1 || ny < 1 || nz < 1) return fail(NGM_E_INVALID, "ngm_grid_eval_knn: every side of the lattice must be >= 1");
  if (num_fields < 1) return fail(NGM_E_UNSUPPORTED, "ngm_grid_eval_knn: no field");
  *K = num_knn < num_fields ? num_knn : num_fields;
  if (*K < 1 || *K > 16) return fail(NGM_E_UNSUPPORTED, "ngm_grid_eval_knn: K must be in [1,16]");
  const int64_t nxy = (int64_t)nx * ny;             // (two int32 factors at a time fit an int64, three at once need not)
  *P = nxy > 0x7fffffff ? nxy : nxy * nz;
  if (*P > 0x7fffffff / *K)
    return fail(NGM_E_UNSUPPORTED, "ngm_grid_eval_knn: nx * ny * nz * K must stay below 2^31 (evaluate the block in parts, or with ngm_field_eval_knn)");
  return NGM_OK;
}
int64_t ngm_grid_eval_knn_workspace(int32_t num_fields, int32_t nx, int32_t ny, int32_t nz, int32_t num_knn) {
  int K = 0;
  int64_t P = 0;
  const int e = grid_knn_shape(num_fields, nx, ny, nz, num_knn, &K, &P);
  return e ? e : ngm_knn_workspace_bytes(num_fields, P, K);
}

int ngm_grid_eval_knn(const ngm_field_cfg* fcfg, const ngm_params* params, int32_t num_fields, const float* field_pos,
                      const float* field_quat, const float* xs, int32_t nx, const float* ys, int32_t ny, const float* zs,
                      int32_t nz, int32_t num_knn, float distance_factor, float outside_value, float mask_radius,
                      int32_t channel, int32_t negate, float* volume, void* workspace, int64_t workspace_bytes, void* stream) {
  int e = check_field_cfg(fcfg);
  if (e) return e;
  e = check_params(fcfg, params);
  if (e) return e;
  if (!xs || !ys || !zs || !volume || !field_pos || !field_quat) return fail(NGM_E_INVALID, "ngm_grid_eval_knn: NULL axis, volume or pose");
  if (channel < 0 || channel > 3) return fail(NGM_E_INVALID, "ngm_grid_eval_knn: channel must be 0..3");
  int K = 0;
  int64_t P = 0;
  e = grid_knn_shape(num_fields, nx, ny, nz, num_knn, &K, &P);
  if (e) return e;
  const FwdPlan plan = plan_knn(fcfg);         // the evaluation is planned before the grid build and the assignment launch
  e = ngm_launch_grid_knn(fcfg, params, num_fields, field_pos, field_quat, xs, nx, ys, ny, zs, nz, K, distance_factor, outside_value,
                          mask_radius > 0.f ? mask_radius : fcfg->field_radius, channel, negate ? 1 : 0, volume, workspace,
                          workspace_bytes, plan, (hipStream_t)stream);
  if (e == NGM_E_WORKSPACE) return fail(e, "ngm_grid_eval_knn: workspace too small");
  if (plan.status) return fail(plan.status, plan.why);
  if (e) return fail(e, "ngm_grid_eval_knn: not available for this configuration");
  g_last_fwd[NGM_FWD_KNN] = plan;
  return check_launch("ngm_grid_eval_knn");
}

int64_t ngm_render_eval_knn_workspace(const ngm_render_cfg* rcfg, int32_t num_fields, int32_t ray_block, int32_t num_knn) {
  const int K = num_knn < num_fields ? num_knn : num_fields;
  if (!rcfg || num_fields < 1 || ray_block < 1 || K < 1 || rcfg->num_samples_coarse < 1) return NGM_E_INVALID;
  return ngm_knn_render_workspace_bytes(num_fields, ray_block, rcfg->num_samples_coarse, K);
}

int ngm_render_eval_knn(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, const ngm_params* params, int32_t num_fields,
                        const float* field_pos, const float* field_quat, const ngm_rays* rays, int32_t num_knn,
                        float distance_factor, float outside_value, float mask_radius, int32_t ray_block,
                        const ngm_prediction* pred, void* workspace, int64_t workspace_bytes, void* stream) {
  int e = check_field_cfg(fcfg);
  if (e) return e;
  e = check_params(fcfg, params);
  if (e) return e;
  if (!rcfg || !rays || !pred || !field_pos || !field_quat || num_fields < 1 || ray_block < 1 || !rays->ijs || !rays->c2ws ||
      rays->F < 0 || rays->R < 0)
    return fail(NGM_E_INVALID, "ngm_render_eval_knn: bad argument");
  if ((int64_t)rays->F * rays->R == 0) return NGM_OK;
  const int K = num_knn < num_fields ? num_knn : num_fields;
  if (K < 1 || K > 8) return fail(NGM_E_UNSUPPORTED, "ngm_render_eval_knn: K must be in [1,8] (the blend inside the quadrature is compiled for up to 8 neighbours; K = 9..16: the staged entry points, ngm_sample_rays_world -> ngm_field_eval_knn -> ngm_composite_fwd_packed)");
  const FwdPlan plan = plan_knn(fcfg);
  if (plan.status) return fail(plan.status, plan.why);
  e = ngm_launch_render_eval_knn(fcfg, rcfg, params, num_fields, field_pos, field_quat, rays, K, distance_factor, outside_value,
                                 mask_radius > 0.f ? mask_radius : fcfg->field_radius, ray_block, pred, workspace,
                                 workspace_bytes, plan, (hipStream_t)stream);
  if (e == NGM_E_WORKSPACE) return fail(e, "ngm_render_eval_knn: workspace too small");
  if (e) return fail(e, "ngm_render_eval_knn: not available for this configuration (samples per ray <= 1024, ray_block * samples * K < 2^31)");
  g_last_fwd[NGM_FWD_KNN] = plan;
  return check_launch("ngm_render_eval_knn");
}

// ------------------------------------------------------------------------------------------------
// mesh extraction
// ------------------------------------------------------------------------------------------------
int64_t ngm_marching_cubes_workspace(int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 2 || ny < 2 || nz < 2 || 3 * (int64_t)nx * ny * nz + 1 > 0x7fffffff) return NGM_E_INVALID;
  return ngm_mc_workspace_bytes(nx, ny, nz);
}
static int mc_fail(int e, const char* what) {
  if (e == NGM_E_WORKSPACE) return fail(e, "marching cubes: workspace too small");
  if (e == NGM_E_UNSUPPORTED) return fail(e, "marching cubes: grid too large (3 * nx * ny * nz must fit 31 bits)");
  if (e == NGM_E_HIP) return fail(e, "marching cubes: HIP error");
  if (e) return fail(e, what);
  return check_launch(what);
}
int ngm_marching_cubes_count(const float* volume, int32_t nx, int32_t ny, int32_t nz, float isolevel, int64_t* counts,
                             void* workspace, int64_t workspace_bytes, void* stream) {
  return mc_fail(ngm_launch_mc_count(volume, nx, ny, nz, isolevel, counts, workspace, workspace_bytes, (hipStream_t)stream),
                 "ngm_marching_cubes_count: bad argument");
}
int ngm_marching_cubes_emit(const float* volume, int32_t nx, int32_t ny, int32_t nz, float isolevel, float* verts,
                            int64_t max_verts, int64_t* faces, int64_t max_faces, void* workspace, int64_t workspace_bytes,
                            void* stream) {
  return mc_fail(ngm_launch_mc_emit(volume, nx, ny, nz, isolevel, verts, max_verts, faces, max_faces, workspace,
                                    workspace_bytes, (hipStream_t)stream), "ngm_marching_cubes_emit: bad argument");
}
int ngm_marching_cubes_tables(int8_t* tri_table, int32_t* tri_count) {
  const int e = ngm_mc_copy_tables(tri_table, tri_count);
  return e ? fail(e, "marching cubes: table derivation failed") : NGM_OK;
}

// ------------------------------------------------------------------------------------------------
// scoring a mesh: surface samples and exact nearest points (evaluation.py:75-130, 190-191; ngm_mesh_eval.hip)
// ------------------------------------------------------------------------------------------------
int64_t ngm_surface_sample_workspace(int64_t num_faces) {
  if (num_faces < 1 || num_faces > 0x7fffffff) return NGM_E_INVALID;
  return ngm_surface_sample_bytes(num_faces);
}
int ngm_surface_sample(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, int64_t num_samples,
                       uint64_t seed, float* points, int64_t* face_ids, void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_verts < 0 || num_faces < 0 || num_samples < 0) return fail(NGM_E_INVALID, "ngm_surface_sample: counts must be >= 0");
  if (num_faces == 0) return fail(NGM_E_INVALID, "ngm_surface_sample: a mesh without faces has no surface to sample");
  if (num_verts > 0x7fffffff || num_faces > 0x7fffffff || num_samples > 0x7fffffff)
    return fail(NGM_E_INVALID, "ngm_surface_sample: counts must be below 2^31");
  if (!faces || (num_verts > 0 && !verts) || !workspace || (num_samples > 0 && (!points || !face_ids)))
    return fail(NGM_E_INVALID, "ngm_surface_sample: NULL array");
  if (ngm_launch_surface_sample(verts, num_verts, faces, num_faces, num_samples, seed, points, face_ids, workspace, workspace_bytes,
                                (hipStream_t)stream))
    return fail(NGM_E_INVALID, "ngm_surface_sample: workspace too small (ngm_surface_sample_workspace)");
  if (num_samples == 0) return NGM_OK;
  return check_launch("ngm_surface_sample");
}
int64_t ngm_nearest_point_workspace(int64_t num_refs, int64_t num_queries) {
  if (num_refs < 1 || num_queries < 0 || num_refs > 0x7fffffff || num_queries > 0x7fffffff) return NGM_E_INVALID;
  return ngm_nearest_point_bytes(num_refs, num_queries);
}
int ngm_nearest_point(const float* refs, int64_t num_refs, const float* queries, int64_t num_queries, float* dist, int64_t* index,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_refs < 0 || num_queries < 0) return fail(NGM_E_INVALID, "ngm_nearest_point: counts must be >= 0");
  if (num_refs == 0) return fail(NGM_E_INVALID, "ngm_nearest_point: no reference points");
  if (num_refs > 0x7fffffff || num_queries > 0x7fffffff) return fail(NGM_E_INVALID, "ngm_nearest_point: counts must be below 2^31");
  if (!refs || !workspace || (num_queries > 0 && (!queries || !dist || !index))) return fail(NGM_E_INVALID, "ngm_nearest_point: NULL array");
  if (ngm_launch_nearest_point(refs, num_refs, queries, num_queries, dist, index, workspace, workspace_bytes, (hipStream_t)stream))
    return fail(NGM_E_INVALID, "ngm_nearest_point: workspace too small (ngm_nearest_point_workspace)");
  if (num_queries == 0) return NGM_OK;
  return check_launch("ngm_nearest_point");
}

// ------------------------------------------------------------------------------------------------
// culling a mesh: depth rasteriser and per-vertex visibility (mesh_culling.py:41-225; ngm_mesh_cull.hip)
// ------------------------------------------------------------------------------------------------
int ngm_mesh_depth(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, const float* c2w, int64_t num_poses,
                   int32_t width, int32_t height, float fx, float fy, float cx, float cy, float near, float far, float* depth,
                   void* stream) {
  if (num_verts < 0 || num_faces < 0 || num_poses < 0) return fail(NGM_E_INVALID, "ngm_mesh_depth: counts must be >= 0");
  if (num_verts > 0x7fffffff || num_faces > 0x7fffffff || num_poses > 0x7fffffff)
    return fail(NGM_E_INVALID, "ngm_mesh_depth: counts must be below 2^31");
  if (width < 1 || height < 1) return fail(NGM_E_INVALID, "ngm_mesh_depth: width and height must be >= 1");
  if (!(near > 0.f) || !(far > near)) return fail(NGM_E_INVALID, "ngm_mesh_depth: 0 < near < far");
  if ((num_verts > 0 && !verts) || (num_faces > 0 && !faces) || (num_poses > 0 && (!c2w || !depth)))
    return fail(NGM_E_INVALID, "ngm_mesh_depth: NULL array");
  if (num_poses == 0 || num_verts == 0) return NGM_OK;
  ngm_launch_mesh_depth(verts, num_verts, faces, num_faces, c2w, num_poses, width, height, fx, fy, cx, cy, near, far, depth,
                        (hipStream_t)stream);
  return check_launch("ngm_mesh_depth");
}
int ngm_mesh_visibility(const float* verts, int64_t num_verts, const float* c2w, int64_t num_poses, int32_t width, int32_t height,
                        float fx, float fy, float cx, float cy, const float* depth, float eps, int64_t num_frustum_poses,
                        int32_t* in_frustum, int32_t* observed, void* stream) {
  if (num_verts < 0 || num_poses < 0 || num_frustum_poses < 0) return fail(NGM_E_INVALID, "ngm_mesh_visibility: counts must be >= 0");
  if (num_verts > 0x7fffffff || num_poses > 0x7fffffff || num_frustum_poses > 0x7fffffff)
    return fail(NGM_E_INVALID, "ngm_mesh_visibility: counts must be below 2^31");
  if (width < 1 || height < 1) return fail(NGM_E_INVALID, "ngm_mesh_visibility: width and height must be >= 1");
  if ((num_verts > 0 && (!verts || !in_frustum || !observed)) || (num_poses > 0 && !c2w))
    return fail(NGM_E_INVALID, "ngm_mesh_visibility: NULL array");
  if (num_poses == 0 || num_verts == 0) return NGM_OK;
  ngm_launch_mesh_visibility(verts, num_verts, c2w, num_poses, width, height, fx, fy, cx, cy, depth, eps, num_frustum_poses, in_frustum,
                             observed, (hipStream_t)stream);
  return check_launch("ngm_mesh_visibility");
}

// ------------------------------------------------------------------------------------------------
// subdividing a mesh to a maximum edge length before it is culled (mesh_culling.py:260-261; ngm_mesh_eval.hip)
// ------------------------------------------------------------------------------------------------
int64_t ngm_mesh_subdivide_workspace(int64_t num_faces) {
  if (num_faces < 0 || num_faces > 0x7fffffff) return NGM_E_INVALID;
  return ngm_mesh_subdivide_bytes(num_faces);
}
int ngm_mesh_subdivide_count(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, double max_edge,
                             int32_t max_iter, void* workspace, int64_t workspace_bytes, int64_t* totals_dev, void* stream) {
  if (num_verts < 0 || num_faces < 0) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_count: counts must be >= 0");
  if (num_verts > 0x7fffffff || num_faces > 0x7fffffff) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_count: counts must be below 2^31");
  if (!(max_edge > 0.0) || !(max_edge < (double)INFINITY)) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_count: max_edge must be finite and > 0");
  if (max_iter < 0 || max_iter > 10) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_count: 0 <= max_iter <= 10");
  if ((num_verts > 0 && !verts) || (num_faces > 0 && (!faces || !workspace)) || !totals_dev)
    return fail(NGM_E_INVALID, "ngm_mesh_subdivide_count: NULL array");
  const int e = ngm_launch_mesh_subdivide_count(verts, num_verts, faces, num_faces, max_edge, max_iter, workspace, workspace_bytes,
                                                totals_dev, (hipStream_t)stream);
  if (e == NGM_E_WORKSPACE) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_count: workspace too small (ngm_mesh_subdivide_workspace)");
  if (e) return fail(e, "ngm_mesh_subdivide_count: HIP error");
  return check_launch("ngm_mesh_subdivide_count");
}
int ngm_mesh_subdivide_emit(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, const float* attrs,
                            int32_t num_channels, const void* workspace, int64_t new_vertices, int64_t out_faces, float* out_verts,
                            int64_t* out_faces_idx, float* out_attrs, int64_t* out_parent, void* stream) {
  if (num_verts < 0 || num_faces < 0 || new_vertices < 0 || out_faces < 0 || num_channels < 0)
    return fail(NGM_E_INVALID, "ngm_mesh_subdivide_emit: counts must be >= 0");
  if (num_verts > 0x7fffffff || num_faces > 0x7fffffff) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_emit: counts must be below 2^31");
  if (num_verts + new_vertices > 0x7fffffff || out_faces > 0x7fffffff)
    return fail(NGM_E_UNSUPPORTED, "ngm_mesh_subdivide_emit: the output must stay below 2^31 vertices and 2^31 faces");
  if (attrs && (int64_t)num_channels * (num_verts + new_vertices) > 0x7fffffff)
    return fail(NGM_E_UNSUPPORTED, "ngm_mesh_subdivide_emit: the output attributes must stay below 2^31 values");
  const int64_t nv = num_verts + new_vertices;
  if ((num_verts > 0 && !verts) || (num_faces > 0 && (!faces || !workspace)) || (nv > 0 && !out_verts) ||
      (out_faces > 0 && (!out_faces_idx || !out_parent)) || (attrs && num_channels > 0 && nv > 0 && !out_attrs))
    return fail(NGM_E_INVALID, "ngm_mesh_subdivide_emit: NULL array");
  if (num_faces == 0 && (new_vertices > 0 || out_faces > 0)) return fail(NGM_E_INVALID, "ngm_mesh_subdivide_emit: a mesh without faces has no output faces");
  ngm_launch_mesh_subdivide_emit(verts, num_verts, faces, num_faces, attrs, num_channels, workspace, new_vertices, out_faces, out_verts,
                                 out_faces_idx, out_attrs, out_parent, (hipStream_t)stream);
  return check_launch("ngm_mesh_subdivide_emit");
}

// ------------------------------------------------------------------------------------------------
// aligning a mesh to the ground truth: vertex normals and point-to-plane ICP (evaluation.py:133-160; ngm_mesh_eval.hip)
// ------------------------------------------------------------------------------------------------
int64_t ngm_mesh_vertex_normals_workspace(int64_t num_verts) {
  if (num_verts < 0 || num_verts > 0x7fffffff) return NGM_E_INVALID;
  return ngm_mesh_vertex_normals_bytes(num_verts);
}
int ngm_mesh_vertex_normals(const float* verts, int64_t num_verts, const int64_t* faces, int64_t num_faces, float* normals,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_verts < 0 || num_faces < 0) return fail(NGM_E_INVALID, "ngm_mesh_vertex_normals: counts must be >= 0");
  if (num_verts > 0x7fffffff || num_faces > 0x7fffffff) return fail(NGM_E_INVALID, "ngm_mesh_vertex_normals: counts must be below 2^31");
  if ((num_verts > 0 && (!verts || !normals || !workspace)) || (num_faces > 0 && !faces))
    return fail(NGM_E_INVALID, "ngm_mesh_vertex_normals: NULL array");
  if (ngm_launch_mesh_vertex_normals(verts, num_verts, faces, num_faces, normals, workspace, workspace_bytes, (hipStream_t)stream))
    return fail(NGM_E_INVALID, "ngm_mesh_vertex_normals: workspace too small (ngm_mesh_vertex_normals_workspace)");
  if (num_verts == 0) return NGM_OK;
  return check_launch("ngm_mesh_vertex_normals");
}
int64_t ngm_icp_point_to_plane_workspace(int64_t num_target, int64_t num_source) {
  if (num_target < 1 || num_source < 0 || num_target > 0x7fffffff || num_source > 0x7fffffff) return NGM_E_INVALID;
  return ngm_icp_point_to_plane_bytes(num_target, num_source);
}
int ngm_icp_point_to_plane(const float* source, int64_t num_source, const float* target, const float* target_normals, int64_t num_target,
                           double threshold, int32_t max_iteration, double relative_fitness, double relative_rmse, const double* init,
                           double* state, void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_source < 0 || num_target < 0) return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: counts must be >= 0");
  if (num_target == 0) return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: no target points");
  if (num_source > 0x7fffffff || num_target > 0x7fffffff) return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: counts must be below 2^31");
  if (!(threshold > 0.0) || !(threshold < (double)INFINITY)) return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: threshold must be finite and > 0");
  if (max_iteration < 0 || max_iteration > 1000) return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: 0 <= max_iteration <= 1000");
  if (!target || !target_normals || !state || !workspace || (num_source > 0 && !source))
    return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: NULL array");
  if (ngm_launch_icp_point_to_plane(source, num_source, target, target_normals, num_target, threshold, max_iteration, relative_fitness,
                                    relative_rmse, init, state, workspace, workspace_bytes, (hipStream_t)stream))
    return fail(NGM_E_INVALID, "ngm_icp_point_to_plane: workspace too small (ngm_icp_point_to_plane_workspace)");
  return check_launch("ngm_icp_point_to_plane");
}

// ------------------------------------------------------------------------------------------------
// scoring rendered frames: PSNR, SSIM and depth L1 in fp64 (evaluation.py:20-30, 46-62; ngm_image_metrics.hip)
// ------------------------------------------------------------------------------------------------
static bool image_metrics_shape_ok(int32_t batch, int32_t height, int32_t width, int32_t crop) {
  return batch >= 0 && height >= 0 && width >= 0 && crop >= 0 && (int64_t)batch * height * width < ((int64_t)1 << 31);
}
int64_t ngm_image_metrics_workspace(int32_t batch, int32_t height, int32_t width, int32_t crop) {
  if (!image_metrics_shape_ok(batch, height, width, crop)) return NGM_E_INVALID;
  return ngm_image_metrics_bytes(batch, height, width, crop);
}
int ngm_image_metrics(const float* pred, const float* target, int32_t batch, int32_t height, int32_t width, int32_t crop, double* out,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  if (batch < 0 || height < 0 || width < 0) return fail(NGM_E_INVALID, "ngm_image_metrics: batch, height and width must be >= 0");
  if (crop < 0) return fail(NGM_E_INVALID, "ngm_image_metrics: crop must be >= 0");
  if (!image_metrics_shape_ok(batch, height, width, crop)) return fail(NGM_E_INVALID, "ngm_image_metrics: batch * height * width must be below 2^31");
  if (!pred || !target || !out || !workspace) return fail(NGM_E_INVALID, "ngm_image_metrics: NULL array");
  if (((uintptr_t)pred | (uintptr_t)target) & 15) return fail(NGM_E_INVALID, "ngm_image_metrics: pred and target must be 16-byte aligned");
  if (ngm_launch_image_metrics(pred, target, batch, height, width, crop, out, workspace, workspace_bytes, (hipStream_t)stream))
    return fail(NGM_E_INVALID, "ngm_image_metrics: workspace too small (ngm_image_metrics_workspace)");
  if (batch == 0) return NGM_OK;
  return check_launch("ngm_image_metrics");
}

// covering a keyframe's depth with new fields (run_mapping.py:265-345; ngm_cover.hip)
static int cover_shape(int32_t height, int32_t width, int32_t num_active, int32_t max_new) {
  if (height < 1 || width < 1 || (int64_t)height * width >= ((int64_t)1 << 31))
    return fail(NGM_E_INVALID, "ngm_cover_depth: height and width must be >= 1 and height * width below 2^31");
  if (num_active < 0) return fail(NGM_E_INVALID, "ngm_cover_depth: num_active must be >= 0");
  if (max_new < 1) return fail(NGM_E_INVALID, "ngm_cover_depth: max_new must be >= 1");
  if (max_new > NGM_COVER_MAX_NEW) return fail(NGM_E_UNSUPPORTED, "ngm_cover_depth: max_new above NGM_COVER_MAX_NEW");
  return NGM_OK;
}
int64_t ngm_cover_depth_workspace(int32_t height, int32_t width, int32_t num_active, int32_t max_new) {
  const int rc = cover_shape(height, width, num_active, max_new);
  if (rc != NGM_OK) return rc;
  return ngm_cover_bytes(height, width, num_active, max_new);
}
int ngm_cover_depth(const ngm_cover_depth_args* a, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!a) return fail(NGM_E_INVALID, "ngm_cover_depth: NULL argument");
  if (!a->depth || !a->c2w || !a->shift || !a->new_positions || !a->counts || !workspace)
    return fail(NGM_E_INVALID, "ngm_cover_depth: NULL array");
  const int rc = cover_shape(a->height, a->width, a->num_active, a->max_new);
  if (rc == NGM_E_INVALID) return rc;
  if (a->pixel_stride < 1 || a->rows < 0) return fail(NGM_E_INVALID, "ngm_cover_depth: pixel_stride must be >= 1 and rows >= 0");
  if (a->num_active > 0 && !a->field_positions) return fail(NGM_E_INVALID, "ngm_cover_depth: active fields without field_positions");
  if (!a->field_ids && a->num_active > a->rows) return fail(NGM_E_INVALID, "ngm_cover_depth: num_active above rows");
  if (!(a->radius > 0.f) || !(a->cell > 0.f) || !(a->radius < INFINITY) || !(a->cell < INFINITY))
    return fail(NGM_E_INVALID, "ngm_cover_depth: radius and cell must be finite and > 0");
  if (rc != NGM_OK) return rc;                                               // NGM_E_UNSUPPORTED: after every NGM_E_INVALID
  if (ngm_launch_cover(*a, workspace, workspace_bytes, (hipStream_t)stream))
    return fail(NGM_E_WORKSPACE, "ngm_cover_depth: workspace too small (ngm_cover_depth_workspace)");
  return check_launch("ngm_cover_depth");
}
int ngm_cover_depth_counters(int32_t height, int32_t width, int32_t num_active, int32_t max_new, void* workspace, int32_t* out5,
                             void* stream) {
  if (!workspace || !out5) return fail(NGM_E_INVALID, "ngm_cover_depth_counters: NULL argument");
  const int rc = cover_shape(height, width, num_active, max_new);
  if (rc != NGM_OK) return rc;
  const int32_t* ctr = ngm_cover_counters(height, width, num_active, max_new, workspace);
  if (hipMemcpyAsync(out5, ctr, 5 * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return check_launch("ngm_cover_depth_counters") == NGM_OK ? fail(NGM_E_HIP, "ngm_cover_depth_counters: copy failed") : NGM_E_HIP;
  return NGM_OK;
}

// ------------------------------------------------------------------------------------------------
// one-shot loss exchange between the ranks of a node (ngm_peer.hip)
// ------------------------------------------------------------------------------------------------
static int hip_fail(hipError_t e, const char* what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  (void)hipGetLastError();
  return NGM_E_HIP;
}
int64_t ngm_peer_mailbox_bytes(void) { return 2 * NGM_MAX_PEERS * 16 * 8; }
int ngm_peer_alloc(int64_t bytes, void** ptr) {
  if (!ptr || bytes <= 0) return fail(NGM_E_INVALID, "ngm_peer_alloc: bad argument");
  const int e = ngm_peer_alloc_impl(bytes, ptr);
  return e ? hip_fail((hipError_t)e, "ngm_peer_alloc") : NGM_OK;
}
int ngm_peer_free(void* ptr) {
  const hipError_t e = hipFree(ptr);
  return e == hipSuccess ? NGM_OK : hip_fail(e, "ngm_peer_free");
}
int ngm_ipc_export(void* ptr, unsigned char handle[64]) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
  if (!ptr || !handle) return fail(NGM_E_INVALID, "ngm_ipc_export: NULL");
  hipIpcMemHandle_t h;
  const hipError_t e = hipIpcGetMemHandle(&h, ptr);
  if (e != hipSuccess) return hip_fail(e, "hipIpcGetMemHandle");
  memcpy(handle, &h, 64);
  return NGM_OK;
}
int ngm_ipc_open(const unsigned char handle[64], void** ptr) {
  if (!ptr || !handle) return fail(NGM_E_INVALID, "ngm_ipc_open: NULL");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, 64);
  const hipError_t e = hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess);
  return e == hipSuccess ? NGM_OK : hip_fail(e, "hipIpcOpenMemHandle");
}
int ngm_ipc_close(void* ptr) {
  const hipError_t e = hipIpcCloseMemHandle(ptr);
  return e == hipSuccess ? NGM_OK : hip_fail(e, "hipIpcCloseMemHandle");
}
int ngm_debug_last_stash_mode(void) { return g_last_bwd.stash_kind ? g_last_bwd.half : -1; }
int ngm_debug_stash_mode(int mode) {
  const int prev = g_stash_override;
  if (mode >= 0 && mode <= 1) g_stash_override = mode;
  else if (mode == -2) g_stash_override = -1;
  return prev;
}

int ngm_debug_plan_bwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t F, int64_t n, int32_t guided,
                       int32_t stash_offered, int32_t seeds_written, int32_t* out5) {
  const int e = check_field_cfg(fcfg);
  if (e) return e;
  if (!out5 || F < 1 || n < 1 || (rcfg && n > INT32_MAX)) return fail(NGM_E_INVALID, "ngm_debug_plan_bwd: bad argument");
  BwdPlan bp;
  int fwd_matmul = -1;
  if (rcfg) {
    BwdAsk ask;
    ask.seeds_written = seeds_written != 0;
    const RenderPlan p = plan_render(fcfg, rcfg, F, (int)n, guided != 0, true, ask);
    bp = p.bwd;
    fwd_matmul = p.fwd.matmul;
  } else {
    bp = plan_points(fcfg, F, n, stash_offered != 0);
  }
  out5[0] = bp.variant; out5[1] = bp.fused_comp; out5[2] = bp.stash_kind; out5[3] = bp.stash_layers; out5[4] = fwd_matmul;
  return bp.status ? fail(bp.status, bp.why) : NGM_OK;
}

int ngm_debug_plan_fwd(const ngm_field_cfg* fcfg, const ngm_render_cfg* rcfg, int32_t surface, int32_t F, int64_t n, int32_t guided,
                       int32_t* out12) {
  const int e = check_field_cfg(fcfg);
  if (e) return e;
  if (!out12 || surface < NGM_FWD_RENDER || surface > NGM_FWD_KNN || (surface == NGM_FWD_RENDER) != (rcfg != nullptr) || F < 1 || n < 1 ||
      (rcfg && n > INT32_MAX))
    return fail(NGM_E_INVALID, "ngm_debug_plan_fwd: bad argument");
  FwdAsk ask;
  ask.surface = surface; ask.F = F; ask.n = n;
  const FwdPlan p = rcfg ? plan_render(fcfg, rcfg, F, (int)n, guided != 0, false).fwd : plan_fwd(fcfg, ask);
  const int32_t out[12] = {p.MI, p.MH, p.L, p.matmul, p.one_tile, p.waves, (int32_t)p.lds_bytes, p.neus, p.threads, p.rays_per_block, p.maxs, p.blocks};
  memcpy(out12, out, sizeof(out));
  return p.status ? fail(p.status, p.why) : NGM_OK;
}

double ngm_peer_set_timeout(double seconds) { return ngm_peer_set_timeout_impl(seconds); }

int ngm_loss_exchange(const ngm_peer_exchange* px, float* loss_sums, void* stream) {
  if (!px || !loss_sums || !px->seq || !px->status) return fail(NGM_E_INVALID, "ngm_loss_exchange: NULL");
  if (px->world < 1 || px->world > NGM_MAX_PEERS || px->rank < 0 || px->rank >= px->world)
    return fail(NGM_E_INVALID, "ngm_loss_exchange: 1 <= world <= 8, 0 <= rank < world");
  for (int p = 0; p < px->world; ++p)
    if (!px->mailbox[p]) return fail(NGM_E_INVALID, "ngm_loss_exchange: mailbox of a rank not mapped");
  ngm_launch_loss_exchange(*px, loss_sums, (hipStream_t)stream);
  return check_launch("ngm_loss_exchange");
}

}  // extern "C"
