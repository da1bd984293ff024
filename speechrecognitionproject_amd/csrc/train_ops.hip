// K7/K8: the small training-step kernels around the acoustic models.
//  * cross-entropy (mean over the batch) forward + backward  — nn.CrossEntropyLoss, training.py:73,87
//    and the same on the soft target of a mixed / label-smoothed batch (srk_cross_entropy_mix)
//  * Adam (beta1, beta2, eps; no weight decay, no amsgrad)     — torch.optim.Adam, training.py:74,91
//    over one flat fp32 parameter buffer (one launch for the whole model)
//  * inverted dropout with an explicit mask                     — nn.Dropout(), model_fbanks_cnn.py:79,98
#include <cfloat>
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

// One wave per row; C <= 64 * 4.  loss_rows[b] = logsumexp(x_b) - x_b[label_b];
// dx = (softmax(x_b) - onehot(label_b)) * scale.
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                      int B, int C, float scale, float* __restrict__ loss_rows,
                                                      float* __restrict__ dx, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* row = x + (size_t)b * C;
  const int64_t lab = labels[b];
  if (lab < 0 || lab >= C) {   // out-of-range label: the loss becomes NaN (loud), flag set
    if (lane == 0) {
      atomicExch(bad, 1);
      loss_rows[b] = NAN;
    }
    return;
  }
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float lse = m + logf(s);
  if (lane == 0) loss_rows[b] = lse - row[lab];
  if (dx)
    for (int c = lane; c < C; c += 64) dx[(size_t)b * C + c] = (expf(row[c] - lse) - (c == lab ? 1.f : 0.f)) * scale;
}

// ce_rows_kernel on a soft target (include/srk.h srk_cross_entropy_mix): with q = labels[partner_b], w = 1 - lam_b,
//   t_c = (1 - eps) (lam_b [c == y] + w [c == q]) + eps / C,   loss_rows[b] = lse - sum_c t_c x_c,
//   dx = (softmax(x_b) - t) * scale.
// partner == lam == nullptr: q = y, lam_b = 1.  A weight of exactly 0 drops its term and eps == 0 drops the
// smoothing sum, so without a mix and with eps == 0 every value is ce_rows_kernel's, bit for bit.  A row is
// validated before anything is read through its partner or labels.
__global__ __launch_bounds__(256) void ce_mix_rows_kernel(const float* __restrict__ x,
                                                          const int64_t* __restrict__ labels,
                                                          const int32_t* __restrict__ partner,
                                                          const float* __restrict__ lam, int B, int C, float eps,
                                                          float scale, float* __restrict__ loss_rows,
                                                          float* __restrict__ dx, int* __restrict__ bad) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* row = x + (size_t)b * C;
  const int64_t lab = labels[b];
  int64_t q = lab;
  float l = 1.f;
  bool ok = lab >= 0 && lab < C;
  if (partner) {
    const int p = partner[b];
    l = lam[b];
    ok = ok && p >= 0 && p < B && l >= 0.f && l <= 1.f;   // NaN fails both comparisons
    if (ok) {
      q = labels[p];
      ok = q >= 0 && q < C;
    }
  }
  if (!ok) {   // the loss becomes NaN (loud), flag set
    if (lane == 0) {
      atomicExch(bad, 1);
      loss_rows[b] = NAN;
    }
    return;
  }
  const float w = 1.f - l;
  float m = -INFINITY;
  for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += expf(row[c] - m);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float lse = m + logf(s);
  float tz = (l != 0.f ? l * row[lab] : 0.f) + (w != 0.f ? w * row[q] : 0.f);
  if (eps != 0.f) {
    float sz = 0.f;
    for (int c = lane; c < C; c += 64) sz += row[c];
    for (int o = 32; o > 0; o >>= 1) sz += __shfl_xor(sz, o, 64);
    tz = (1.f - eps) * tz + (eps / (float)C) * sz;
  }
  if (lane == 0) loss_rows[b] = lse - tz;
  if (dx) {
    const float keep = 1.f - eps, floor_t = eps / (float)C;
    for (int c = lane; c < C; c += 64) {
      const float t = keep * ((c == lab ? l : 0.f) + (c == q ? w : 0.f)) + floor_t;
      dx[(size_t)b * C + c] = (expf(row[c] - lse) - t) * scale;
    }
  }
}

// Deterministic mean of the per-row losses (one workgroup).
__global__ __launch_bounds__(256) void mean_kernel(const float* __restrict__ v, int n, float* __restrict__ out) {
  __shared__ float part[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) s += v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = part[0] / (float)n;
}

// torch.optim.Adam single-tensor update, in torch's operation order:
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
//   denom = sqrt(v) / sqrt(1 - b2^t) + eps ; p -= (lr / (1 - b1^t)) * m / denom
// grad_scale multiplies g first (1/world for a summed all-reduce, or 1).
__device__ __forceinline__ void adam_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                          float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                          float bc1, float bc2_sqrt, float grad_scale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      float4 pv = *reinterpret_cast<float4*>(p + i);
      float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x; float* pp = &pv.x;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = gp[k] * grad_scale;
        mp[k] = mp[k] * b1 + (1.f - b1) * gg;
        vp[k] = vp[k] * b2 + (1.f - b2) * gg * gg;
        const float denom = sqrtf(vp[k]) / bc2_sqrt + eps;
        pp[k] = pp[k] - (lr / bc1) * (mp[k] / denom);
      }
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
      *reinterpret_cast<float4*>(p + i) = pv;
    } else {
      for (int64_t k = i; k < n; ++k) {
        const float gg = g[k] * grad_scale;
        m[k] = m[k] * b1 + (1.f - b1) * gg;
        v[k] = v[k] * b2 + (1.f - b2) * gg * gg;
        const float denom = sqrtf(v[k]) / bc2_sqrt + eps;
        p[k] = p[k] - (lr / bc1) * (m[k] / denom);
      }
    }
  }
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                            float bc1, float bc2_sqrt, float grad_scale) {
  adam_body(p, g, m, v, n, lr, b1, b2, eps, bc1, bc2_sqrt, grad_scale);
}

// Counter-based Bernoulli mask (splitmix64 of seed ^ index): keep with probability 1 - p.
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t i) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);   // 24 random bits -> [0, 1)
}

__global__ void dropout_fwd_kernel(const float* __restrict__ x, int64_t n, float p, float scale, uint64_t seed,
                                   float* __restrict__ y, uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool k = uniform01(seed, (uint64_t)i) >= p;
  keep[i] = k;
  y[i] = k ? x[i] * scale : 0.f;
}

// Loss-scaler state (include/srk.h srk_grad_scaler_init): 8 words on the device.
struct ScalerState {
  float scale, inv_scale, growth, backoff;
  int found_inf, good_steps, interval, overflows;
};

__global__ void scaler_init_kernel(ScalerState* __restrict__ s, float scale, float growth, float backoff,
                                   int interval) {
  s->scale = scale;
  s->inv_scale = 1.0f / scale;
  s->growth = growth;
  s->backoff = backoff;
  s->found_inf = 0;
  s->good_steps = 0;
  s->interval = interval;
  s->overflows = 0;
}

// found_inf |= any non-finite gradient element (16-B loads; one atomic per wave that saw one).
__global__ __launch_bounds__(256) void finite_check_kernel(const float* __restrict__ g, int64_t n,
                                                           ScalerState* __restrict__ s) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  bool bad = false;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(g + i);
      // |x| <= FLT_MAX is false exactly for +-inf and NaN
      bad |= !(fabsf(v.x) <= FLT_MAX) || !(fabsf(v.y) <= FLT_MAX) || !(fabsf(v.z) <= FLT_MAX) ||
             !(fabsf(v.w) <= FLT_MAX);
    } else {
      for (int64_t k = i; k < n; ++k) bad |= !(fabsf(g[k]) <= FLT_MAX);
    }
  }
  if (__ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(&s->found_inf, 1);
}

// After the (possibly skipped) update: count / back off on an overflow, grow the scale after
// `interval` clean steps (interval 0 = static scale), clear the flag for the next step.
__global__ void scaler_update_kernel(ScalerState* __restrict__ s) {
  if (s->found_inf) {
    s->overflows += 1;
    s->good_steps = 0;
    if (s->interval > 0) {
      s->scale *= s->backoff;
      s->inv_scale = 1.0f / s->scale;
    }
  } else if (s->interval > 0 && ++s->good_steps >= s->interval) {
    s->scale *= s->growth;
    s->inv_scale = 1.0f / s->scale;
    s->good_steps = 0;
  }
  s->found_inf = 0;
}

// Device-resident optimizer step (graph-replayable): one lane advances the step count and stores the
// bias corrections the host path would compute (double precision, rounded to float) beside it.  A
// step the loss scaler skips (non-finite gradients) does not count, as with torch's GradScaler.
__global__ void adam_prep_kernel(int64_t* __restrict__ state, float beta1, float beta2,
                                 const ScalerState* __restrict__ sc) {
  if (sc && sc->found_inf) return;
  const int64_t step = state[0] + 1;
  state[0] = step;
  float* bc = reinterpret_cast<float*>(state + 1);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  bc[0] = (float)bc1;
  bc[1] = (float)sqrt(bc2);
}

__global__ __launch_bounds__(256) void adam_state_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                         float b1, float b2, float eps,
                                                         const int64_t* __restrict__ state, float grad_scale,
                                                         const ScalerState* __restrict__ sc) {
  if (sc) {
    if (sc->found_inf) return;     // skipped step: parameters and moments stay as they are
    grad_scale *= sc->inv_scale;
  }
  const float* f = reinterpret_cast<const float*>(state + 1);   // bc1, sqrt(bc2), lr
  adam_body(p, g, m, v, n, f[2], b1, b2, eps, f[0], f[1], grad_scale);
}

// ---- AdamW decay, global-norm clipping and a weight EMA around the same update (include/srk.h srk_adamw_step) ----
// Clip state on the device: what the norm pass measured and what the update multiplies the gradient by.
struct ClipState {
  float total_norm, coef;
  int32_t clipped_steps, pad;
};

constexpr int kNormThreads = 256;
constexpr int kNormMaxBlocks = 1024;
// The norm pass's grid, a function of n alone (the summation order, and so the bits, follow from it).
inline int64_t norm_blocks(int64_t n) {
  return std::max<int64_t>(1, std::min<int64_t>((n + kNormThreads * 4 - 1) / (kNormThreads * 4), kNormMaxBlocks));
}

// One read of the gradient: part[block] = sum over the block's elements of (g[i] * s)^2 and, with a scaler,
// found_inf |= any non-finite element (finite_check_kernel's test and atomic).  s = grad_scale [* inv_scale], applied
// before squaring so loss-scaled gradients cannot overflow the sum.  Fixed order, no floating-point atomics: a lane
// adds its elements in index order (grid stride 4 * blocks * 256), the 64 lanes fold by xor 32, 16, ... 1 (both
// partners of a pair compute the same commutative sum), wave 0's lane 0 adds the four wave sums in wave order.
// NORM = false: the finite check alone (a scaler without clipping), part is not touched.
template <bool NORM>
__global__ __launch_bounds__(kNormThreads) void grad_norm_kernel(const float* __restrict__ g, int64_t n,
                                                                 float grad_scale, ScalerState* __restrict__ sc,
                                                                 float* __restrict__ part) {
  __shared__ float wave_sum[kNormThreads / 64];
  const float s = sc ? grad_scale * sc->inv_scale : grad_scale;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  float acc = 0.f;
  bool bad = false;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 v = *reinterpret_cast<const float4*>(g + i);
      // |x| <= FLT_MAX is false exactly for +-inf and NaN
      bad |= !(fabsf(v.x) <= FLT_MAX) || !(fabsf(v.y) <= FLT_MAX) || !(fabsf(v.z) <= FLT_MAX) ||
             !(fabsf(v.w) <= FLT_MAX);
      if (NORM) {
        const float a = v.x * s, b = v.y * s, c = v.z * s, d = v.w * s;
        acc += a * a;
        acc += b * b;
        acc += c * c;
        acc += d * d;
      }
    } else {
      for (int64_t k = i; k < n; ++k) {
        bad |= !(fabsf(g[k]) <= FLT_MAX);
        if (NORM) {
          const float a = g[k] * s;
          acc += a * a;
        }
      }
    }
  }
  if (sc && __ballot(bad) != 0 && (threadIdx.x & 63) == 0) atomicOr(&sc->found_inf, 1);
  if (NORM) {
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
  }
}

// adam_prep_kernel plus the clip coefficient, one workgroup: the partials are summed in double in a fixed order
// (thread t takes t, t + 256, ...; then a halving tree), total_norm = sqrt(sum), coef = min(1, max_norm /
// (total_norm + 1e-6)) in float as torch.nn.utils.clip_grad_norm_ (a NaN norm gives a NaN coef, as torch's clamp).
// clip == nullptr: no clipping, the step count alone.
__global__ __launch_bounds__(256) void adam_prep_clip_kernel(int64_t* __restrict__ state, float beta1, float beta2,
                                                             const ScalerState* __restrict__ sc,
                                                             const float* __restrict__ part, int nparts,
                                                             float max_norm, ClipState* __restrict__ clip) {
  __shared__ double tree[256];
  const bool skipped = sc && sc->found_inf;
  if (clip) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += (double)part[i];
    tree[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      const float total = (float)sqrt(tree[0]);
      const float c = max_norm / (total + 1e-6f);
      const float coef = c > 1.f ? 1.f : c;
      clip->total_norm = total;
      clip->coef = coef;
      if (!skipped && coef < 1.f) clip->clipped_steps += 1;
      clip->pad = 0;
    }
  }
  if (threadIdx.x != 0 || skipped) return;
  // adam_prep_kernel's lines
  const int64_t step = state[0] + 1;
  state[0] = step;
  float* bc = reinterpret_cast<float*>(state + 1);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  bc[0] = (float)bc1;
  bc[1] = (float)sqrt(bc2);
}

// One element of the extended update.  Every rounding is spelled out (no contraction, explicit fmaf), because with
// coef == 1, no decay and no EMA the result has to be adam_body's bits, and adam_body as compiled for gfx950 rounds by
// code path: the float4 body fuses m = fma(1 - b1, gg, b1 m) and v = fma(gg, (1 - b2) gg, b2 v), the scalar tail's
// pair loop (the tail vectorised by two) fuses m = fma(b1, m, (1 - b1) gg) instead, and the tail's last single
// element fuses neither sum; all three end in p = fma(-(lr / bc1), m / denom, p).  tests/test_optim_ext_gpu.py holds
// the two kernels to each other at every tail length.
enum AdamRounding { kRoundVec4, kRoundPair, kRoundSingle };

template <AdamRounding R>
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float* __restrict__ ema, float gs,
                                              float kp, float b1, float b2, float c1, float c2, float eps,
                                              float bc2_sqrt, float step_size, float d) {
#pragma clang fp contract(off)
  const float gg = g * gs;
  const float pd = p * kp;                 // keep == 1.0f gives p back exactly
  if (R == kRoundVec4) {
    m = __builtin_fmaf(c1, gg, b1 * m);
  } else if (R == kRoundPair) {
    m = __builtin_fmaf(b1, m, c1 * gg);
  } else {
    m = b1 * m + c1 * gg;
  }
  if (R == kRoundSingle) {
    v = gg * (c2 * gg) + b2 * v;
  } else {
    v = __builtin_fmaf(gg, c2 * gg, b2 * v);
  }
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = __builtin_fmaf(-step_size, m / denom, pd);
  if (ema) *ema = d * *ema + (1.f - d) * p;
}

// adam_state_kernel with three more operands.  Per element, in this order: a skipped step writes nothing;
// gg = g * (s * coef) (coef == 1.0f: the float adam_body computes); a chunk marked for decay (one mask byte per 64
// floats, nullptr = every chunk) has p *= 1 - lr * weight_decay first (torch.optim.AdamW's decoupled form, the factor
// formed in double as torch forms it on the host); then adam_body's arithmetic; then ema = d * ema + (1 - d) * p_new
// where an EMA buffer is given.  A float4 never straddles a chunk (i % 4 == 0).
__global__ __launch_bounds__(256) void adamw_state_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                          float b1, float b2, float eps,
                                                          const int64_t* __restrict__ state, float grad_scale,
                                                          const ScalerState* __restrict__ sc, float weight_decay,
                                                          const uint8_t* __restrict__ mask,
                                                          const ClipState* __restrict__ clip, float* __restrict__ ema,
                                                          float ema_decay) {
#pragma clang fp contract(off)
  if (sc) {
    if (sc->found_inf) return;
    grad_scale *= sc->inv_scale;
  }
  const float* f = reinterpret_cast<const float*>(state + 1);   // bc1, sqrt(bc2), lr
  const float bc1 = f[0], bc2_sqrt = f[1], lr = f[2];
  // one gradient factor, s * coef: with coef == 1.0f it is s itself
  const float gs = grad_scale * (clip ? clip->coef : 1.f);
  const float keep = (float)(1.0 - (double)lr * (double)weight_decay);
  const bool decay = weight_decay != 0.f;
  const float c1 = 1.f - b1, c2 = 1.f - b2, step_size = lr / bc1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float kp = (decay && (!mask || mask[i >> 6])) ? keep : 1.f;
      float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      float4 pv = *reinterpret_cast<float4*>(p + i);
      float4 ev = ema ? *reinterpret_cast<float4*>(ema + i) : float4{0.f, 0.f, 0.f, 0.f};
      float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x; float* pp = &pv.x; float* ep = &ev.x;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        adamw_element<kRoundVec4>(pp[k], gp[k], mp[k], vp[k], ema ? ep + k : nullptr, gs, kp, b1, b2, c1, c2, eps,
                                  bc2_sqrt, step_size, ema_decay);
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
      *reinterpret_cast<float4*>(p + i) = pv;
      if (ema) *reinterpret_cast<float4*>(ema + i) = ev;
    } else {
      // adam_body's tail as compiled: pairs first, then a last single element
      const int64_t pairs_end = i + ((n - i) & ~(int64_t)1);
      for (int64_t k = i; k < n; ++k) {
        const float kp = (decay && (!mask || mask[k >> 6])) ? keep : 1.f;
        if (k < pairs_end)
          adamw_element<kRoundPair>(p[k], g[k], m[k], v[k], ema ? ema + k : nullptr, gs, kp, b1, b2, c1, c2, eps,
                                    bc2_sqrt, step_size, ema_decay);
        else
          adamw_element<kRoundSingle>(p[k], g[k], m[k], v[k], ema ? ema + k : nullptr, gs, kp, b1, b2, c1, c2, eps,
                                      bc2_sqrt, step_size, ema_decay);
      }
    }
  }
}

// Dropout whose seed lives on the device ([base, counter]): the mask of call k hashes base + k, and
// the counter advances behind the mask kernel — so a captured graph draws a fresh mask per replay.
__global__ void dropout_state_kernel(const float* __restrict__ x, int64_t n, float p, float scale,
                                     const uint64_t* __restrict__ state, float* __restrict__ y,
                                     uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t seed = state[0] + 0xD1B54A32D192ED03ull * state[1];
  const bool k = uniform01(seed, (uint64_t)i) >= p;
  keep[i] = k;
  y[i] = k ? x[i] * scale : 0.f;
}

// U[lo, hi) in float64 from the same device state and hash as the dropout mask (53 random bits per
// draw; lo + (hi - lo) * u in two roundings, as numpy's uniform); the counter advances behind it.
__global__ void uniform_f64_state_kernel(const uint64_t* __restrict__ state, double lo, double hi, int64_t n,
                                         double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t seed = state[0] + 0xD1B54A32D192ED03ull * state[1];
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0);
  const double w = (hi - lo) * u;
  out[i] = lo + w;
}

__global__ void counter_inc_kernel(uint64_t* __restrict__ c) { c[0] += 1; }

__global__ void dropout_kernel(const float* __restrict__ x, const uint8_t* __restrict__ keep, int64_t n, float scale,
                               float* __restrict__ y) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = keep[i] ? x[i] * scale : 0.f;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_cross_entropy(const float* logits, const int64_t* labels, int64_t B, int64_t C, float* loss,
                      float* dlogits, float* ws, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(B > 0 && C > 0 && C <= 4096, SRK_ERR_INVALID, "cross_entropy: bad shape");
  SRK_REQUIRE(logits && labels && loss && ws, SRK_ERR_INVALID, "cross_entropy: null pointer");
  hipStream_t s = srk::as_stream(stream);
  // ws: B floats of per-row loss, then one int error flag
  int* bad = reinterpret_cast<int*>(ws + B);
  SRK_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(srk::ce_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, labels, (int)B,
                     (int)C, 1.0f / (float)B, ws, dlogits, bad);
  hipLaunchKernelGGL(srk::mean_kernel, dim3(1), dim3(256), 0, s, ws, (int)B, loss);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_cross_entropy_mix(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam,
                          int64_t B, int64_t C, float smoothing, float* loss, float* dlogits, float* ws,
                          void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(B > 0 && B < (int64_t(1) << 31) && C > 0 && C <= 4096, SRK_ERR_INVALID, "cross_entropy_mix: bad shape");
  SRK_REQUIRE(smoothing >= 0.f && smoothing < 1.f, SRK_ERR_INVALID,
              "cross_entropy_mix: smoothing must be in [0, 1), got %g", (double)smoothing);
  SRK_REQUIRE((partner == nullptr) == (lam == nullptr), SRK_ERR_INVALID,
              "cross_entropy_mix: partner and lam are both given or both NULL");
  SRK_REQUIRE(logits && labels && loss && ws, SRK_ERR_INVALID, "cross_entropy_mix: null pointer");
  hipStream_t s = srk::as_stream(stream);
  // ws: B floats of per-row loss, then one int error flag (as srk_cross_entropy)
  int* bad = reinterpret_cast<int*>(ws + B);
  SRK_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(srk::ce_mix_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, labels, partner,
                     lam, (int)B, (int)C, smoothing, 1.0f / (float)B, ws, dlogits, bad);
  hipLaunchKernelGGL(srk::mean_kernel, dim3(1), dim3(256), 0, s, ws, (int)B, loss);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, int64_t step, float grad_scale, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && step >= 1, SRK_ERR_INVALID, "adam: bad n/step");
  if (n == 0) return SRK_OK;
  SRK_REQUIRE(param && grad && exp_avg && exp_avg_sq, SRK_ERR_INVALID, "adam: null pointer");
  SRK_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0,
              SRK_ERR_INVALID, "adam: buffers must be 16-byte aligned");
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  const int nt = 256;
  const int64_t blocks = std::min<int64_t>((n + nt * 4 - 1) / (nt * 4), 256 * 8);
  srk::ProfScope prof("adam", srk::as_stream(stream), 28.0 * (double)n);   // p,g,m,v read + p,m,v written
  hipLaunchKernelGGL(srk::adam_kernel, dim3((unsigned)blocks), dim3(nt), 0, srk::as_stream(stream), param, grad,
                     exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, (float)bc1, (float)std::sqrt(bc2), grad_scale);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_adam_step_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                        float beta2, float eps, int64_t* state, float grad_scale, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && state, SRK_ERR_INVALID, "adam_state: bad n / null state");
  if (n == 0) return SRK_OK;
  SRK_REQUIRE(param && grad && exp_avg && exp_avg_sq, SRK_ERR_INVALID, "adam_state: null pointer");
  SRK_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0 &&
              (uintptr_t)state % 8 == 0, SRK_ERR_INVALID, "adam_state: buffers must be 16-byte aligned");
  hipStream_t s = srk::as_stream(stream);
  hipLaunchKernelGGL(srk::adam_prep_kernel, dim3(1), dim3(1), 0, s, state, beta1, beta2,
                     (const srk::ScalerState*)nullptr);
  const int nt = 256;
  const int64_t blocks = std::min<int64_t>((n + nt * 4 - 1) / (nt * 4), 256 * 8);
  srk::ProfScope prof("adam", s, 28.0 * (double)n);   // p,g,m,v read + p,m,v written
  hipLaunchKernelGGL(srk::adam_state_kernel, dim3((unsigned)blocks), dim3(nt), 0, s, param, grad, exp_avg, exp_avg_sq,
                     n, beta1, beta2, eps, state, grad_scale, (const srk::ScalerState*)nullptr);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_grad_scaler_init(int32_t* scaler, float init_scale, float growth_factor, float backoff_factor,
                         int growth_interval, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(scaler && (uintptr_t)scaler % 4 == 0, SRK_ERR_INVALID, "grad_scaler_init: null / misaligned state");
  SRK_REQUIRE(init_scale > 0.f && std::isfinite(init_scale) && growth_factor >= 1.f && backoff_factor > 0.f &&
                  backoff_factor <= 1.f && growth_interval >= 0,
              SRK_ERR_INVALID, "grad_scaler_init: bad scale / growth / backoff / interval");
  hipLaunchKernelGGL(srk::scaler_init_kernel, dim3(1), dim3(1), 0, srk::as_stream(stream),
                     reinterpret_cast<srk::ScalerState*>(scaler), init_scale, growth_factor, backoff_factor,
                     growth_interval);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_adam_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                         float beta2, float eps, int64_t* state, float grad_scale, int32_t* scaler, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && state && scaler, SRK_ERR_INVALID, "adam_scaled: bad n / null state");
  SRK_REQUIRE(n == 0 || (param && grad && exp_avg && exp_avg_sq), SRK_ERR_INVALID, "adam_scaled: null pointer");
  SRK_REQUIRE(((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) % 16 == 0 &&
                  (uintptr_t)state % 8 == 0 && (uintptr_t)scaler % 4 == 0,
              SRK_ERR_INVALID, "adam_scaled: buffers must be 16-byte aligned");
  hipStream_t s = srk::as_stream(stream);
  auto* sc = reinterpret_cast<srk::ScalerState*>(scaler);
  const int nt = 256;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n + nt * 4 - 1) / (nt * 4), 256 * 8));
  if (n > 0) {
    srk::ProfScope prof("grad_check", s, 4.0 * (double)n);
    hipLaunchKernelGGL(srk::finite_check_kernel, dim3((unsigned)blocks), dim3(nt), 0, s, grad, n, sc);
  }
  hipLaunchKernelGGL(srk::adam_prep_kernel, dim3(1), dim3(1), 0, s, state, beta1, beta2, (const srk::ScalerState*)sc);
  if (n > 0) {
    srk::ProfScope prof("adam", s, 28.0 * (double)n);
    hipLaunchKernelGGL(srk::adam_state_kernel, dim3((unsigned)blocks), dim3(nt), 0, s, param, grad, exp_avg,
                       exp_avg_sq, n, beta1, beta2, eps, state, grad_scale, (const srk::ScalerState*)sc);
  }
  hipLaunchKernelGGL(srk::scaler_update_kernel, dim3(1), dim3(1), 0, s, sc);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int64_t srk_adamw_workspace_floats(int64_t n) { return n < 0 ? 0 : srk::norm_blocks(n); }

int srk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                   float beta2, float eps, int64_t* state, float grad_scale, int32_t* scaler, float weight_decay,
                   const uint8_t* decay_mask, float max_norm, int32_t* clip_state, float* ema, float ema_decay,
                   float* ws, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0, SRK_ERR_INVALID, "adamw: n must be >= 0, got %lld", (long long)n);
  SRK_REQUIRE(state, SRK_ERR_INVALID, "adamw: state is null");
  SRK_REQUIRE(n == 0 || (param && grad && exp_avg && exp_avg_sq), SRK_ERR_INVALID,
              "adamw: param, grad, exp_avg and exp_avg_sq must not be null");
  const struct { const char* name; const void* p; unsigned align; } ptrs[] = {
      {"param", param, 16}, {"grad", grad, 16}, {"exp_avg", exp_avg, 16}, {"exp_avg_sq", exp_avg_sq, 16},
      {"ema", ema, 16}, {"state", state, 8}, {"scaler", scaler, 4}, {"clip_state", clip_state, 4}, {"ws", ws, 4}};
  for (const auto& a : ptrs)
    SRK_REQUIRE((uintptr_t)a.p % a.align == 0, SRK_ERR_INVALID, "adamw: %s must be %u-byte aligned", a.name, a.align);
  SRK_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), SRK_ERR_INVALID,
              "adamw: weight_decay must be finite and >= 0, got %g", (double)weight_decay);
  SRK_REQUIRE(!std::isnan(max_norm), SRK_ERR_INVALID, "adamw: max_norm is NaN");
  const bool clip_on = max_norm > 0.f && std::isfinite(max_norm);   // <= 0 or +inf: clipping is off
  SRK_REQUIRE(!clip_on || clip_state, SRK_ERR_INVALID, "adamw: clip_state is null while clipping is on (max_norm %g)",
              (double)max_norm);
  SRK_REQUIRE(!clip_on || ws, SRK_ERR_INVALID,
              "adamw: ws is null while clipping is on (max_norm %g): srk_adamw_workspace_floats(n) floats",
              (double)max_norm);
  SRK_REQUIRE(ema == nullptr || (ema_decay >= 0.f && ema_decay < 1.f), SRK_ERR_INVALID,
              "adamw: ema_decay must be in [0, 1) with an ema buffer, got %g", (double)ema_decay);
  SRK_REQUIRE(ema == nullptr || (ema != param && ema != exp_avg && ema != exp_avg_sq && ema != grad), SRK_ERR_INVALID,
              "adamw: ema must be a buffer of its own");
  if (n == 0 && !scaler) return SRK_OK;   // as srk_adam_step_state
  hipStream_t s = srk::as_stream(stream);
  auto* sc = reinterpret_cast<srk::ScalerState*>(scaler);
  auto* clip = clip_on ? reinterpret_cast<srk::ClipState*>(clip_state) : nullptr;
  const int64_t nparts = clip_on && n > 0 ? srk::norm_blocks(n) : 0;
  if (n > 0 && clip_on) {
    srk::ProfScope prof("grad_norm", s, 4.0 * (double)n);
    hipLaunchKernelGGL(srk::grad_norm_kernel<true>, dim3((unsigned)nparts), dim3(srk::kNormThreads), 0, s, grad, n,
                       grad_scale, sc, ws);
  } else if (n > 0 && sc) {
    srk::ProfScope prof("grad_check", s, 4.0 * (double)n);
    hipLaunchKernelGGL(srk::grad_norm_kernel<false>, dim3((unsigned)srk::norm_blocks(n)), dim3(srk::kNormThreads), 0,
                       s, grad, n, grad_scale, sc, (float*)nullptr);
  }
  hipLaunchKernelGGL(srk::adam_prep_clip_kernel, dim3(1), dim3(256), 0, s, state, beta1, beta2,
                     (const srk::ScalerState*)sc, (const float*)ws, (int)nparts, max_norm, clip);
  if (n > 0) {
    const int nt = 256;
    const int64_t blocks = std::min<int64_t>((n + nt * 4 - 1) / (nt * 4), 256 * 8);   // adam_state_kernel's grid
    // p, g, m, v read + p, m, v written; ema read + written; one mask byte per 64 floats
    srk::ProfScope prof("adamw", s, (28.0 + (ema ? 8.0 : 0.0) + (decay_mask ? 1.0 / 64.0 : 0.0)) * (double)n);
    hipLaunchKernelGGL(srk::adamw_state_kernel, dim3((unsigned)blocks), dim3(nt), 0, s, param, grad, exp_avg,
                       exp_avg_sq, n, beta1, beta2, eps, state, grad_scale, (const srk::ScalerState*)sc, weight_decay,
                       decay_mask, (const srk::ClipState*)clip, ema, ema_decay);
  }
  if (sc) hipLaunchKernelGGL(srk::scaler_update_kernel, dim3(1), dim3(1), 0, s, sc);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_dropout_fwd_state(const float* x, int64_t n, float p, uint64_t* state, float* y, uint8_t* keep,
                          void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && p >= 0.f && p < 1.f && state && (n == 0 || (x && y && keep)), SRK_ERR_INVALID,
              "dropout_fwd_state: bad args");
  if (n == 0) return SRK_OK;
  hipStream_t s = srk::as_stream(stream);
  hipLaunchKernelGGL(srk::dropout_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, p,
                     1.0f / (1.0f - p), state, y, keep);
  hipLaunchKernelGGL(srk::counter_inc_kernel, dim3(1), dim3(1), 0, s, state + 1);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_uniform_f64_state(uint64_t* state, double lo, double hi, int64_t n, double* out, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && state && (n == 0 || out) && lo <= hi && (hi - lo) < INFINITY, SRK_ERR_INVALID,
              "uniform_f64_state: bad args");
  if (n == 0) return SRK_OK;
  hipStream_t s = srk::as_stream(stream);
  hipLaunchKernelGGL(srk::uniform_f64_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, state, lo, hi,
                     n, out);
  hipLaunchKernelGGL(srk::counter_inc_kernel, dim3(1), dim3(1), 0, s, state + 1);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_dropout_fwd(const float* x, int64_t n, float p, uint64_t seed, float* y, uint8_t* keep, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && p >= 0.f && p < 1.f && (n == 0 || (x && y && keep)), SRK_ERR_INVALID, "dropout_fwd: bad args");
  if (n == 0) return SRK_OK;
  hipLaunchKernelGGL(srk::dropout_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, srk::as_stream(stream), x,
                     n, p, 1.0f / (1.0f - p), seed, y, keep);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_dropout_apply(const float* x, const uint8_t* keep, int64_t n, float scale, float* y, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && (n == 0 || (x && keep && y)), SRK_ERR_INVALID, "dropout: bad args");
  if (n == 0) return SRK_OK;
  hipLaunchKernelGGL(srk::dropout_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, srk::as_stream(stream), x,
                     keep, n, scale, y);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
