// K7/K8: the small training-step kernels around the acoustic models.
//  * cross-entropy (mean over the batch) forward + backward  — nn.CrossEntropyLoss, training.py:73,87:
//    one row kernel on a soft target (mixed / label-smoothed batch); the hard target is its special case
//  * Adam over one flat fp32 parameter buffer (one launch for the whole model) — torch.optim.Adam, training.py:74,91:
//    one element update with every rounding spelled out, one grid-stride loop, one host launcher behind
//    srk_adam_step_state / _scaled / srk_adamw_step (loss scaling, AdamW decay, global-norm clipping, weight EMA
//    are operands that may be absent); srk_adam_step runs the same loop with lr and step from the host
//  * inverted dropout with an explicit mask                     — nn.Dropout(), model_fbanks_cnn.py:79,98
#include <cfloat>
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

// One wave per row, on a soft target (include/srk.h srk_cross_entropy_mix): with q = labels[partner_b], w = 1 - lam_b,
//   t_c = (1 - eps) (lam_b [c == y] + w [c == q]) + eps / C,   loss_rows[b] = lse - sum_c t_c x_c,
//   dx = (softmax(x_b) - t) * scale.
// partner == lam == nullptr: q = y, lam_b = 1.  A weight of exactly 0 drops its term and eps == 0 drops the
// smoothing sum, so without a mix and with eps == 0 (srk_cross_entropy) loss_rows[b] = lse - x_b[label_b] and
// dx = (softmax(x_b) - onehot(label_b)) * scale with no rounding added.  A row is validated before anything is read
// through its partner or labels.
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
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

// Counter-based Bernoulli mask (splitmix64 of seed ^ index): keep with probability 1 - p.
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t i) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);   // 24 random bits -> [0, 1)
}

// One element of the mask and of the masked output; the caller says where the seed comes from.
__device__ __forceinline__ void dropout_mask_body(const float* __restrict__ x, int64_t n, float p, float scale,
                                                  uint64_t seed, float* __restrict__ y, uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool k = uniform01(seed, (uint64_t)i) >= p;
  keep[i] = k;
  y[i] = k ? x[i] * scale : 0.f;
}

__global__ void dropout_fwd_kernel(const float* __restrict__ x, int64_t n, float p, float scale, uint64_t seed,
                                   float* __restrict__ y, uint8_t* __restrict__ keep) {
  dropout_mask_body(x, n, p, scale, seed, y, keep);
}

// The seed lives on the device ([base, counter]): the mask of call k hashes base + k, and the counter advances
// behind the mask kernel — so a captured graph draws a fresh mask per replay.
__global__ void dropout_state_kernel(const float* __restrict__ x, int64_t n, float p, float scale,
                                     const uint64_t* __restrict__ state, float* __restrict__ y,
                                     uint8_t* __restrict__ keep) {
  dropout_mask_body(x, n, p, scale, state[0] + 0xD1B54A32D192ED03ull * state[1], y, keep);
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

// ---- Adam: torch.optim.Adam's single-tensor update, with AdamW decay, global-norm clipping and a weight EMA as
// optional operands (include/srk.h srk_adamw_step) ----
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
// found_inf |= any non-finite element (16-B loads; one atomic per wave that saw one).  s = grad_scale [* inv_scale],
// applied before squaring so loss-scaled gradients cannot overflow the sum.  Fixed order, no floating-point atomics: a
// lane adds its elements in index order (grid stride 4 * blocks * 256), the 64 lanes fold by xor 32, 16, ... 1 (both
// partners of a pair compute the same commutative sum), wave 0's lane 0 adds the four wave sums in wave order.
// NORM = false: the finite check alone (a scaler without clipping), part is not touched; found_inf is an integer OR,
// so that instantiation may take any grid (update_blocks below), while NORM = true keeps norm_blocks(n).
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

// Device-resident optimizer step (graph-replayable), one workgroup.  Lane 0 advances the step count and stores the
// bias corrections the host path would compute (double precision, rounded to float) beside it; a step the loss
// scaler skips (non-finite gradients) does not count, as with torch's GradScaler.  With clipping, the clip
// coefficient first: the partials are summed in double in a fixed order (thread t takes t, t + 256, ...; then a
// halving tree), total_norm = sqrt(sum), coef = min(1, max_norm / (total_norm + 1e-6)) in float as
// torch.nn.utils.clip_grad_norm_ (a NaN norm gives a NaN coef, as torch's clamp).
// clip == nullptr: no clipping, the step count alone (one lane is enough).
__global__ __launch_bounds__(256) void adam_prep_kernel(int64_t* __restrict__ state, float beta1, float beta2,
                                                        const ScalerState* __restrict__ sc,
                                                        const float* __restrict__ part, int nparts, float max_norm,
                                                        ClipState* __restrict__ clip) {
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
  const int64_t step = state[0] + 1;
  state[0] = step;
  float* bc = reinterpret_cast<float*>(state + 1);
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  bc[0] = (float)bc1;
  bc[1] = (float)sqrt(bc2);
}

// One element of the update, in torch's operation order:
//   m = b1 m + (1 - b1) gg ; v = b2 v + (1 - b2) gg gg ; denom = sqrt(v) / sqrt(1 - b2^t) + eps ;
//   p = p kp - (lr / (1 - b1^t)) m / denom ; ema = d ema + (1 - d) p
// Every rounding is spelled out (no contraction, explicit fmaf), and it differs by code path: the float4 body fuses
// m = fma(1 - b1, gg, b1 m) and v = fma(gg, (1 - b2) gg, b2 v), a pair of tail elements fuses
// m = fma(b1, m, (1 - b1) gg) instead, and a last single tail element fuses neither sum; all three end in
// p = fma(-(lr / bc1), m / denom, p kp).  These are the roundings an earlier kernel written with plain * and + got
// from the compiler's contraction for gfx950; every checkpoint and golden was made with them, so they stay, and
// tests/golden/train_ops_bits.json (tests/test_train_ops_bits_gpu.py) pins them at every tail length.
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

// The scalars of one launch: gs multiplies the gradient (grad_scale [* inv_scale] [* clip coef]), keep is the decay
// factor 1 - lr * weight_decay (exactly 1.0f: no decay, and p * 1.0f is p).
struct AdamScalars {
  float lr, bc1, bc2_sqrt, gs, keep, ema_decay;
};

// The update of the whole buffer: a grid-stride loop over float4s with a scalar tail (pairs first, then a last single
// element: AdamRounding).  A chunk marked for decay (one mask byte per 64 floats, nullptr = every chunk) has p *= keep
// first (torch.optim.AdamW's decoupled form); a float4 never straddles a chunk (i % 4 == 0).  ema == nullptr: no EMA.
// EXT = false compiles decay, mask and EMA out (the caller has no decay and no ema): the same adamw_element, so the
// same bits (adam_plain_kernel says why it exists).
template <bool EXT>
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, int64_t n, float b1, float b2, float eps,
                                            const uint8_t* __restrict__ mask_or_null,
                                            float* __restrict__ ema_or_null, const AdamScalars s) {
#pragma clang fp contract(off)
  const uint8_t* __restrict__ mask = EXT ? mask_or_null : nullptr;
  float* __restrict__ ema = EXT ? ema_or_null : nullptr;
  const float gs = s.gs, keep = s.keep, bc2_sqrt = s.bc2_sqrt, ema_decay = s.ema_decay;
  const bool decay = EXT && keep != 1.f;
  const float c1 = 1.f - b1, c2 = 1.f - b2, step_size = s.lr / s.bc1;
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
      // one to three elements, all in one chunk: a pair first (if there are two), then a last single one
      const float kp = (decay && (!mask || mask[i >> 6])) ? keep : 1.f;
      int64_t k = i;
      if (n - i >= 2)
        for (const int64_t end = i + 2; k < end; ++k)
          adamw_element<kRoundPair>(p[k], g[k], m[k], v[k], ema ? ema + k : nullptr, gs, kp, b1, b2, c1, c2, eps,
                                    bc2_sqrt, step_size, ema_decay);
      if (k < n)
        adamw_element<kRoundSingle>(p[k], g[k], m[k], v[k], ema ? ema + k : nullptr, gs, kp, b1, b2, c1, c2, eps,
                                    bc2_sqrt, step_size, ema_decay);
    }
  }
}

// srk_adam_step: lr and the bias corrections come from the host, nothing else is on.
__global__ __launch_bounds__(256) void adam_host_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                        float b1, float b2, float eps, float lr, float bc1,
                                                        float bc2_sqrt, float grad_scale) {
  adam_update<false>(p, g, m, v, n, b1, b2, eps, nullptr, nullptr,
                     AdamScalars{lr, bc1, bc2_sqrt, grad_scale, 1.f, 0.f});
}

// The device-state step with decay, clipping and the EMA all off (a scaler or none): lr and the bias corrections from
// the device state adam_prep_kernel wrote, the unscaling and the skip from the scaler.  A skipped step writes nothing.
// It is adam_state_kernel below without the operands that are off; as one kernel the features-off launch measured
// 2 - 3 % slower at 6.4 M parameters than the plain update it replaces, this way about 1 % ("Measured
// against the parent").
__global__ __launch_bounds__(256) void adam_plain_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                         float b1, float b2, float eps,
                                                         const int64_t* __restrict__ state, float grad_scale,
                                                         const ScalerState* __restrict__ sc) {
  if (sc) {
    if (sc->found_inf) return;
    grad_scale *= sc->inv_scale;
  }
  const float* f = reinterpret_cast<const float*>(state + 1);   // bc1, sqrt(bc2), lr
  adam_update<false>(p, g, m, v, n, b1, b2, eps, nullptr, nullptr, AdamScalars{f[2], f[0], f[1], grad_scale, 1.f, 0.f});
}

// The same with any of decay, clipping and the EMA on: the clip coefficient from the clip state, the decay factor
// formed in double, as torch forms it on the host.
__global__ __launch_bounds__(256) void adam_state_kernel(float* __restrict__ p, const float* __restrict__ g,
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
  const float lr = f[2];
  // one gradient factor, s * coef: with coef == 1.0f it is s itself
  const float gs = grad_scale * (clip ? clip->coef : 1.f);
  // weight_decay == 0 is no decay whatever lr holds (1 - inf * 0 would be NaN)
  const float keep = weight_decay != 0.f ? (float)(1.0 - (double)lr * (double)weight_decay) : 1.f;
  adam_update<true>(p, g, m, v, n, b1, b2, eps, mask, ema, AdamScalars{lr, f[0], f[1], gs, keep, ema_decay});
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

// ---- host side ----
// Both cross-entropy entries after their own shape checks.  ws: B floats of per-row loss, then one int error flag.
int ce_launch(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam, int64_t B,
              int64_t C, float smoothing, float* loss, float* dlogits, float* ws, void* stream) {
  hipStream_t s = as_stream(stream);
  int* bad = reinterpret_cast<int*>(ws + B);
  SRK_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), s));
  hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, s, logits, labels, partner, lam,
                     (int)B, (int)C, smoothing, 1.0f / (float)B, ws, dlogits, bad);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, ws, (int)B, loss);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
}

// The grid of the update and of the finite check alone: one float4 per lane and trip, at most 2048 workgroups.
constexpr int kAdamThreads = 256;
inline int64_t update_blocks(int64_t n) {
  return std::max<int64_t>(1, std::min<int64_t>((n + kAdamThreads * 4 - 1) / (kAdamThreads * 4), 256 * 8));
}

// The one-line texts of the entries older than srk_adamw_step for the four buffers (adam_launch names the offender).
int adam_buffers_terse(const char* who, const float* p, const float* g, const float* m, const float* v, int64_t n,
                       bool rest_aligned) {
  SRK_REQUIRE(n == 0 || (p && g && m && v), SRK_ERR_INVALID, "%s: null pointer", who);
  SRK_REQUIRE(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16 == 0 && rest_aligned, SRK_ERR_INVALID,
              "%s: buffers must be 16-byte aligned", who);
  return SRK_OK;
}

// What a device-state Adam step takes (srk_adamw_step's operands); what an entry does not have stays null / zero.
struct AdamArgs {
  float* param;
  const float* grad;
  float *exp_avg, *exp_avg_sq;
  int64_t n;
  float beta1, beta2, eps;
  int64_t* state;
  float grad_scale;
  int32_t* scaler = nullptr;
  float weight_decay = 0.f;
  const uint8_t* decay_mask = nullptr;
  float max_norm = 0.f;
  int32_t* clip_state = nullptr;
  float* ema = nullptr;
  float ema_decay = 0.f;
  float* ws = nullptr;
};

// The one launcher behind srk_adam_step_state / _scaled / srk_adamw_step: checks, then
// [norm | finite check] -> prep -> update -> [scaler update].  `who` prefixes the error texts.
int adam_launch(const char* who, const AdamArgs& a, void* stream) {
  const int64_t n = a.n;
  SRK_REQUIRE(n >= 0, SRK_ERR_INVALID, "%s: n must be >= 0, got %lld", who, (long long)n);
  SRK_REQUIRE(a.state, SRK_ERR_INVALID, "%s: state is null", who);
  SRK_REQUIRE(n == 0 || (a.param && a.grad && a.exp_avg && a.exp_avg_sq), SRK_ERR_INVALID,
              "%s: param, grad, exp_avg and exp_avg_sq must not be null", who);
  const struct { const char* name; const void* p; unsigned align; } ptrs[] = {
      {"param", a.param, 16}, {"grad", a.grad, 16}, {"exp_avg", a.exp_avg, 16}, {"exp_avg_sq", a.exp_avg_sq, 16},
      {"ema", a.ema, 16}, {"state", a.state, 8}, {"scaler", a.scaler, 4}, {"clip_state", a.clip_state, 4},
      {"ws", a.ws, 4}};
  for (const auto& q : ptrs)
    SRK_REQUIRE((uintptr_t)q.p % q.align == 0, SRK_ERR_INVALID, "%s: %s must be %u-byte aligned", who, q.name, q.align);
  SRK_REQUIRE(a.weight_decay >= 0.f && std::isfinite(a.weight_decay), SRK_ERR_INVALID,
              "%s: weight_decay must be finite and >= 0, got %g", who, (double)a.weight_decay);
  SRK_REQUIRE(!std::isnan(a.max_norm), SRK_ERR_INVALID, "%s: max_norm is NaN", who);
  const bool clip_on = a.max_norm > 0.f && std::isfinite(a.max_norm);   // <= 0 or +inf: clipping is off
  SRK_REQUIRE(!clip_on || a.clip_state, SRK_ERR_INVALID,
              "%s: clip_state is null while clipping is on (max_norm %g)", who, (double)a.max_norm);
  SRK_REQUIRE(!clip_on || a.ws, SRK_ERR_INVALID,
              "%s: ws is null while clipping is on (max_norm %g): srk_adamw_workspace_floats(n) floats", who,
              (double)a.max_norm);
  SRK_REQUIRE(a.ema == nullptr || (a.ema_decay >= 0.f && a.ema_decay < 1.f), SRK_ERR_INVALID,
              "%s: ema_decay must be in [0, 1) with an ema buffer, got %g", who, (double)a.ema_decay);
  SRK_REQUIRE(a.ema == nullptr || (a.ema != a.param && a.ema != a.exp_avg && a.ema != a.exp_avg_sq && a.ema != a.grad),
              SRK_ERR_INVALID, "%s: ema must be a buffer of its own", who);
  if (n == 0 && !a.scaler) return SRK_OK;   // nothing to update and no scaler to advance
  hipStream_t s = as_stream(stream);
  auto* sc = reinterpret_cast<ScalerState*>(a.scaler);
  auto* clip = clip_on ? reinterpret_cast<ClipState*>(a.clip_state) : nullptr;
  const int64_t nparts = clip_on && n > 0 ? norm_blocks(n) : 0;
  if (n > 0 && clip_on) {
    ProfScope prof("grad_norm", s, 4.0 * (double)n);
    hipLaunchKernelGGL(grad_norm_kernel<true>, dim3((unsigned)nparts), dim3(kNormThreads), 0, s, a.grad, n,
                       a.grad_scale, sc, a.ws);
  } else if (n > 0 && sc) {
    ProfScope prof("grad_check", s, 4.0 * (double)n);
    hipLaunchKernelGGL(grad_norm_kernel<false>, dim3((unsigned)update_blocks(n)), dim3(kNormThreads), 0, s, a.grad, n,
                       a.grad_scale, sc, (float*)nullptr);
  }
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(clip ? 256 : 1), 0, s, a.state, a.beta1, a.beta2,
                     (const ScalerState*)sc, (const float*)a.ws, (int)nparts, a.max_norm, clip);
  if (n > 0) {
    // "adam": the plain update (no scaler, decay, clipping or EMA), "adamw": anything more (srk_adamw_step with a
    // scaler alone has always been recorded so, and tests/test_optim_ext_gpu.py reads it there).  p, g, m, v read +
    // p, m, v written; ema read + written; one mask byte per 64 floats
    const bool plain = !sc && a.weight_decay == 0.f && !clip_on && !a.ema;
    ProfScope prof(plain ? "adam" : "adamw", s,
                   (28.0 + (a.ema ? 8.0 : 0.0) + (a.decay_mask ? 1.0 / 64.0 : 0.0)) * (double)n);
    const dim3 grid((unsigned)update_blocks(n)), block(kAdamThreads);
    if (a.weight_decay == 0.f && !clip && !a.ema)
      hipLaunchKernelGGL(adam_plain_kernel, grid, block, 0, s, a.param, a.grad, a.exp_avg, a.exp_avg_sq, n, a.beta1,
                         a.beta2, a.eps, (const int64_t*)a.state, a.grad_scale, (const ScalerState*)sc);
    else
      hipLaunchKernelGGL(adam_state_kernel, grid, block, 0, s, a.param, a.grad, a.exp_avg, a.exp_avg_sq, n, a.beta1,
                         a.beta2, a.eps, (const int64_t*)a.state, a.grad_scale, (const ScalerState*)sc, a.weight_decay,
                         a.decay_mask, (const ClipState*)clip, a.ema, a.ema_decay);
  }
  if (sc) hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(1), 0, s, sc);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_cross_entropy(const float* logits, const int64_t* labels, int64_t B, int64_t C, float* loss,
                      float* dlogits, float* ws, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(B > 0 && C > 0 && C <= 4096, SRK_ERR_INVALID, "cross_entropy: bad shape");
  SRK_REQUIRE(logits && labels && loss && ws, SRK_ERR_INVALID, "cross_entropy: null pointer");
  return srk::ce_launch(logits, labels, nullptr, nullptr, B, C, 0.f, loss, dlogits, ws, stream);
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
  return srk::ce_launch(logits, labels, partner, lam, B, C, smoothing, loss, dlogits, ws, stream);
  SRK_API_END
}

int srk_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, int64_t step, float grad_scale, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && step >= 1, SRK_ERR_INVALID, "adam: bad n/step");
  if (n == 0) return SRK_OK;
  if (int rc = srk::adam_buffers_terse("adam", param, grad, exp_avg, exp_avg_sq, n, true)) return rc;
  const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
  const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
  srk::ProfScope prof("adam", srk::as_stream(stream), 28.0 * (double)n);   // p,g,m,v read + p,m,v written
  hipLaunchKernelGGL(srk::adam_host_kernel, dim3((unsigned)srk::update_blocks(n)), dim3(srk::kAdamThreads), 0,
                     srk::as_stream(stream), param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, lr, (float)bc1,
                     (float)std::sqrt(bc2), grad_scale);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_adam_step_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                        float beta2, float eps, int64_t* state, float grad_scale, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && state, SRK_ERR_INVALID, "adam_state: bad n / null state");
  if (n == 0) return SRK_OK;   // before any launch: the step count does not advance
  if (int rc = srk::adam_buffers_terse("adam_state", param, grad, exp_avg, exp_avg_sq, n, (uintptr_t)state % 8 == 0))
    return rc;
  const srk::AdamArgs a{param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, state, grad_scale};
  return srk::adam_launch("adam_state", a, stream);
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

// With n == 0 the prep and the scaler update still run (the step counts, the scale may grow).
int srk_adam_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                         float beta2, float eps, int64_t* state, float grad_scale, int32_t* scaler, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 0 && state && scaler, SRK_ERR_INVALID, "adam_scaled: bad n / null state");
  if (int rc = srk::adam_buffers_terse("adam_scaled", param, grad, exp_avg, exp_avg_sq, n,
                                       (uintptr_t)state % 8 == 0 && (uintptr_t)scaler % 4 == 0))
    return rc;
  srk::AdamArgs a{param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, state, grad_scale};
  a.scaler = scaler;
  return srk::adam_launch("adam_scaled", a, stream);
  SRK_API_END
}

int64_t srk_adamw_workspace_floats(int64_t n) { return n < 0 ? 0 : srk::norm_blocks(n); }

int srk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                   float beta2, float eps, int64_t* state, float grad_scale, int32_t* scaler, float weight_decay,
                   const uint8_t* decay_mask, float max_norm, int32_t* clip_state, float* ema, float ema_decay,
                   float* ws, void* stream) {
  SRK_API_BEGIN
  const srk::AdamArgs a{param, grad,   exp_avg,      exp_avg_sq, n,          beta1, beta2,     eps, state,
                        grad_scale, scaler, weight_decay, decay_mask, max_norm, clip_state, ema, ema_decay, ws};
  return srk::adam_launch("adamw", a, stream);
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
