// The sparse per-field Adam update (torch.optim.Adam, L2-coupled weight decay, shared step; rm.py:357-362): the one
// hyper-parameter record, bias-correction pair and element update behind every kernel that applies it.
#pragma once
#include <hip/hip_runtime.h>

struct AdamHyper {
  const int64_t* field_index;      // row of field f in the parameter / moment tensors (NULL: f)
  const int64_t* step_dev;         // non-NULL: the step is read on the device instead of ...
  int64_t step;                    // ... this one (1-based)
  float lr, beta1, beta2, eps, wd;
};
struct AdamCoef { float lr_bc1, inv_sqrt_bc2; };      // lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step)

// The functions take the hyper-parameters as values that the call site reads from its own argument record (a.hyper.beta1):
// that keeps every kernel's machine code what it was with the update written out (profiles/r09_adam_unify.md).

// Double precision.  Host and device pow need not agree in the last bit: a site keeps the side it computes them on.  `step` is
// (double)(step_dev ? *step_dev : step), which each device site reads in place (profiles/r09_adam_unify.md).
__host__ __device__ __forceinline__ AdamCoef adam_coef(float lr, float beta1, float beta2, double step) {
  AdamCoef c;
  c.lr_bc1 = (float)((double)lr / (1.0 - pow((double)beta1, step)));
  c.inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, step)));
  return c;
}
// one element: m and v are updated in place, the new parameter is returned
__device__ __forceinline__ float adam_update(float p, float& m, float& v, float grad, const AdamCoef& c, float beta1, float beta2,
                                             float eps, float wd) {
  const float g = grad + wd * p;
  const float mn = beta1 * m + (1.0f - beta1) * g;
  const float vn = beta2 * v + (1.0f - beta2) * g * g;
  m = mn; v = vn;
  return p - c.lr_bc1 * (mn / (sqrtf(vn) * c.inv_sqrt_bc2 + eps));
}
__device__ __forceinline__ void adam_update4(float4& p, float4& m, float4& v, const float4& grad, const AdamCoef& c, float beta1,
                                             float beta2, float eps, float wd) {
  float* pp = &p.x; float* pm = &m.x; float* pv = &v.x; const float* pg = &grad.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) pp[k] = adam_update(pp[k], pm[k], pv[k], pg[k], c, beta1, beta2, eps, wd);
}
