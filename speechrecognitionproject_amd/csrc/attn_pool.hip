// Attention pooling over time (include/srk.h srk_attn_pool_fwd / _bwd; nn.AttentionPool): a query scores every
// step of a [T][D] sequence, a softmax over time weights the steps and the weighted sum is the context.
//
// Forward and backward are the same three stages over one clip, so both run one kernel template:
//   1. T dot products over D of y_t with a vector u       (fwd: u = q, the scores; bwd: u = dctx, a_t)
//   2. a map over the T values                            (fwd: softmax -> alpha; bwd: ds_t = alpha_t (a_t - m))
//   3. the column sums  sum_t w_t y_t  over T             (fwd: w = alpha -> ctx; bwd: w = ds -> dq / scale)
// and the backward's dy_t = alpha_t dctx + scale ds_t q needs no y at all.  The work is memory bound
// (2 flops per byte of y), one workgroup of 16 waves owns a clip, and every sum has a fixed order (xor
// butterflies inside a wave, then LDS partials added in index order): no atomics, equal bits on every run.
//
//  * attn_pool_regs_kernel: T <= 64, D <= 1024, D % 4 == 0.  Thread (g, c) of 4 x 256 keeps the float4 of
//    columns 4c..4c+3 of rows g, g + 4, ... (<= 16 float4 = 64 VGPRs), so y is read once with 16-byte loads,
//    stage 1 costs each wave <= 16 butterflies and stage 3 is in-lane plus one 4-way LDS combine.
//  * attn_pool_2pass_kernel: every other shape.  Stage 1 streams one row per wave, stage 3 reads y again
//    (a clip that was just streamed: served by L2 / the Infinity Cache), float4 or, when D % 4 != 0 or a
//    tensor is not 16-byte aligned, scalar accesses.
#include <cmath>
#include <type_traits>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kThreads = 1024;   // 16 waves: one workgroup per CU
constexpr int kWaves = kThreads / 64;
constexpr int kMaxT = 1024;      // the entry points' domain (the two-pass stage 2 maps one t per thread)
constexpr int kRegRows = 16;     // register-resident rows per thread: T <= 4 * 16
constexpr int kRegCols = 256;    // float4 column slots: D <= 1024

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// float4 / float column slots behind one spelling (the two-pass kernel's VEC switch)
__device__ __forceinline__ void vload(const float* p, float4& v) { v = *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void vload(const float* p, float& v) { v = *p; }
__device__ __forceinline__ void vstore(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void vstore(float* p, const float& v) { *p = v; }
__device__ __forceinline__ void vzero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void vzero(float& v) { v = 0.f; }
__device__ __forceinline__ float vdot(const float4& a, const float4& b) {
  return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w);
}
__device__ __forceinline__ float vdot(const float& a, const float& b) { return a * b; }
__device__ __forceinline__ void vfma(float4& acc, float w, const float4& v) {
  acc.x += w * v.x;
  acc.y += w * v.y;
  acc.z += w * v.z;
  acc.w += w * v.w;
}
__device__ __forceinline__ void vfma(float& acc, float w, const float& v) { acc += w * v; }
__device__ __forceinline__ void vadd(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}
__device__ __forceinline__ void vadd(float& a, const float& b) { a += b; }
__device__ __forceinline__ void vscale(float4& a, float s) {
  a.x *= s;
  a.y *= s;
  a.z *= s;
  a.w *= s;
}
__device__ __forceinline__ void vscale(float& a, float s) { a *= s; }
// dy_t = alpha_t g + (scale ds_t) q
__device__ __forceinline__ float4 vmix(float a, const float4& g, float b, const float4& q) {
  return make_float4(a * g.x + b * q.x, a * g.y + b * q.y, a * g.z + b * q.z, a * g.w + b * q.w);
}
__device__ __forceinline__ float vmix(float a, const float& g, float b, const float& q) { return a * g + b * q; }

// u: q (forward) or dctx (backward).  out: ctx / dq.  Forward writes alpha_out; backward reads alpha_in and q and
// writes dy.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void attn_pool_regs_kernel(const float* __restrict__ y,
                                                                  const float* __restrict__ u,
                                                                  const float* __restrict__ q,
                                                                  const float* __restrict__ alpha_in, int T, int D,
                                                                  float scale, float* __restrict__ out,
                                                                  float* __restrict__ alpha_out,
                                                                  float* __restrict__ dy) {
  __shared__ float part[kWaves][kRegRows];    // stage 1: each wave's share of its 16 rows' dot products
  __shared__ float wt[64];                    // stage 2's result by t: alpha (fwd) / ds (bwd); 0 past T
  __shared__ float al[64];                    // bwd: alpha by t
  __shared__ float4 accp[3][kRegCols];        // stage 3: the column sums of row groups 1..3
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = tid & (kRegCols - 1), grp = tid >> 8;   // column slot, row group (4 waves each)
  const int col = 4 * c;
  const bool active = col < D;
  const size_t b = blockIdx.x;
  const float* yb = y + b * (size_t)T * D;

  float4 v[kRegRows];
#pragma unroll
  for (int r = 0; r < kRegRows; ++r) {
    const int t = grp + 4 * r;
    if (active && t < T) vload(yb + (size_t)t * D + col, v[r]);
    else vzero(v[r]);
  }
  float4 uv;
  if (active) vload(u + b * D + col, uv);
  else vzero(uv);

#pragma unroll
  for (int r = 0; r < kRegRows; ++r) {
    float p = 0.f;
    if (4 * r < T) p = wave_sum(vdot(v[r], uv));   // (uniform) slots past T hold zeros
    if (lane == 0) part[wave][r] = p;
  }
  __syncthreads();

  if (wave == 0) {   // T <= 64: one value per lane
    const int t = lane, g4 = t & 3, r = t >> 2;
    float s = (part[4 * g4][r] + part[4 * g4 + 1][r]) + (part[4 * g4 + 2][r] + part[4 * g4 + 3][r]);
    if (!BWD) {
      s = t < T ? s * scale : -INFINITY;
      const float m = wave_max(s);
      const float e = t < T ? expf(s - m) : 0.f;
      const float a = e / wave_sum(e);
      wt[t] = a;
      if (t < T) alpha_out[b * T + t] = a;
    } else {
      const float a = t < T ? alpha_in[b * T + t] : 0.f;
      const float m = wave_sum(a * s);
      wt[t] = a * (s - m);
      al[t] = a;
    }
  }
  __syncthreads();

  float4 acc;
  vzero(acc);
#pragma unroll
  for (int r = 0; r < kRegRows; ++r) vfma(acc, wt[grp + 4 * r], v[r]);
  if (BWD && active) {
    float4 qv;
    vload(q + b * D + col, qv);
    float* dyb = dy + b * (size_t)T * D;
#pragma unroll
    for (int r = 0; r < kRegRows; ++r) {
      const int t = grp + 4 * r;
      if (t < T) vstore(dyb + (size_t)t * D + col, vmix(al[t], uv, scale * wt[t], qv));
    }
  }
  if (grp > 0) accp[grp - 1][c] = acc;
  __syncthreads();
  if (grp == 0 && active) {
    vadd(acc, accp[0][c]);
    vadd(acc, accp[1][c]);
    vadd(acc, accp[2][c]);
    if (BWD) vscale(acc, scale);
    vstore(out + b * D + col, acc);
  }
}

// Sum / max of one value per thread over the workgroup, the same result in every thread (red: 16 floats).
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += red[w];
  __syncthreads();
  return s;
}

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) s = fmaxf(s, red[w]);
  __syncthreads();
  return s;
}

template <bool BWD, bool VEC>
__global__ __launch_bounds__(kThreads) void attn_pool_2pass_kernel(const float* __restrict__ y,
                                                                   const float* __restrict__ u,
                                                                   const float* __restrict__ q,
                                                                   const float* __restrict__ alpha_in, int T, int D,
                                                                   float scale, float* __restrict__ out,
                                                                   float* __restrict__ alpha_out,
                                                                   float* __restrict__ dy) {
  using V = typename std::conditional<VEC, float4, float>::type;
  constexpr int W = VEC ? 4 : 1;   // floats per column slot
  __shared__ float sc[kMaxT];      // stage 1's dot products, then stage 2's result (alpha / ds) by t
  __shared__ float al[kMaxT];      // bwd: alpha by t
  __shared__ float red[kWaves];
  __shared__ V accp[kThreads];     // stage 3: [row group][column slot] partial column sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t b = blockIdx.x;
  const float* yb = y + b * (size_t)T * D;
  const float* ub = u + b * D;

  // stage 1: a row per wave
  for (int t = wave; t < T; t += kWaves) {
    const float* row = yb + (size_t)t * D;
    float p = 0.f;
    for (int d = lane * W; d < D; d += 64 * W) {
      V a, s;
      vload(row + d, a);
      vload(ub + d, s);
      p += vdot(a, s);
    }
    p = wave_sum(p);
    if (lane == 0) sc[t] = p;
  }
  __syncthreads();

  // stage 2: T <= 1024, one value per thread
  if (!BWD) {
    const float s = tid < T ? sc[tid] * scale : -INFINITY;
    const float m = block_max(s, red);
    const float e = tid < T ? expf(s - m) : 0.f;
    const float a = e / block_sum(e, red);
    if (tid < T) {
      sc[tid] = a;
      alpha_out[b * T + tid] = a;
    }
  } else {
    const float a = tid < T ? alpha_in[b * T + tid] : 0.f;
    const float s = tid < T ? sc[tid] : 0.f;
    const float m = block_sum(a * s, red);
    if (tid < T) {
      sc[tid] = a * (s - m);
      al[tid] = a;
    }
  }
  __syncthreads();

  // stage 3: ncr column slots per sweep, the rows dealt to the kThreads / ncr row groups
  const int ncols = D / W;
  int ncr = 64;
  while (ncr < ncols && ncr < kThreads) ncr <<= 1;
  const int groups = kThreads / ncr;   // > 1 only when one sweep covers every column
  const int c = tid & (ncr - 1), grp = tid / ncr;
  float* dyb = BWD ? dy + b * (size_t)T * D : nullptr;
  for (int base = 0; base < ncols; base += ncr) {
    const int col = (base + c) * W;
    const bool active = base + c < ncols;
    V acc, uv, qv;
    vzero(acc);
    vzero(uv);
    vzero(qv);
    if (active) {
      if (BWD) {
        vload(ub + col, uv);
        vload(q + b * D + col, qv);
      }
#pragma unroll 4
      for (int t = grp; t < T; t += groups) {
        V a;
        vload(yb + (size_t)t * D + col, a);
        vfma(acc, sc[t], a);
        if (BWD) vstore(dyb + (size_t)t * D + col, vmix(al[t], uv, scale * sc[t], qv));
      }
    }
    if (groups > 1) {   // (uniform)
      accp[grp * ncr + c] = acc;
      __syncthreads();
      if (grp == 0)
        for (int g = 1; g < groups; ++g) vadd(acc, accp[g * ncr + c]);
    }
    if (grp == 0 && active) {
      if (BWD) vscale(acc, scale);
      vstore(out + b * D + col, acc);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BWD>
int launch(const float* y, const float* u, const float* q, const float* alpha_in, int64_t B, int64_t T, int64_t D,
           float scale, float* out, float* alpha_out, float* dy, hipStream_t s) {
  const bool vec = D % 4 == 0 && aligned16(y) && aligned16(u) && aligned16(out) && (!BWD || (aligned16(q) && aligned16(dy)));
  const bool regs = g_opt_attn_pool_regs && vec && T <= 4 * kRegRows && D <= 4 * kRegCols;
  // y read once (the backward writes dy as well), the [B][D] vectors, alpha
  const double bytes = 4.0 * ((BWD ? 2.0 : 1.0) * (double)B * T * D + (BWD ? 3.0 : 2.0) * (double)B * D + (double)B * T);
  ProfScope prof("attn_pool", s, bytes);
  prof.bytes(bytes);
  prof.detail("attn_pool_%s_kernel<%s%s> %lldx%lldx%lld", regs ? "regs" : "2pass", BWD ? "bwd" : "fwd",
              regs ? "" : (vec ? ",vec" : ",scalar"), (long long)B, (long long)T, (long long)D);
  const dim3 grid((unsigned)B), block(kThreads);
  if (regs)
    hipLaunchKernelGGL(attn_pool_regs_kernel<BWD>, grid, block, 0, s, y, u, q, alpha_in, (int)T, (int)D, scale, out,
                       alpha_out, dy);
  else if (vec)
    hipLaunchKernelGGL((attn_pool_2pass_kernel<BWD, true>), grid, block, 0, s, y, u, q, alpha_in, (int)T, (int)D,
                       scale, out, alpha_out, dy);
  else
    hipLaunchKernelGGL((attn_pool_2pass_kernel<BWD, false>), grid, block, 0, s, y, u, q, alpha_in, (int)T, (int)D,
                       scale, out, alpha_out, dy);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_attn_pool_fwd(const float* y, const float* q, int64_t B, int64_t T, int64_t D, float scale, float* ctx,
                      float* alpha, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(B >= 1 && B <= 0x7fffffffLL && T >= 1 && T <= srk::kMaxT && D >= 1 && D <= 4096, SRK_ERR_INVALID,
              "attn_pool_fwd: needs B >= 1, 1 <= T <= 1024, 1 <= D <= 4096, got B %lld T %lld D %lld", (long long)B,
              (long long)T, (long long)D);
  SRK_REQUIRE(std::isfinite(scale), SRK_ERR_INVALID, "attn_pool_fwd: scale is not finite");
  SRK_REQUIRE(y && q && ctx && alpha, SRK_ERR_INVALID, "attn_pool_fwd: null pointer");
  return srk::launch<false>(y, q, nullptr, nullptr, B, T, D, scale, ctx, alpha, nullptr, srk::as_stream(stream));
  SRK_API_END
}

int srk_attn_pool_bwd(const float* y, const float* q, const float* alpha, const float* dctx, int64_t B, int64_t T,
                      int64_t D, float scale, float* dy, float* dq, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(B >= 1 && B <= 0x7fffffffLL && T >= 1 && T <= srk::kMaxT && D >= 1 && D <= 4096, SRK_ERR_INVALID,
              "attn_pool_bwd: needs B >= 1, 1 <= T <= 1024, 1 <= D <= 4096, got B %lld T %lld D %lld", (long long)B,
              (long long)T, (long long)D);
  SRK_REQUIRE(std::isfinite(scale), SRK_ERR_INVALID, "attn_pool_bwd: scale is not finite");
  SRK_REQUIRE(y && q && alpha && dctx && dy && dq, SRK_ERR_INVALID, "attn_pool_bwd: null pointer");
  return srk::launch<true>(y, dctx, q, alpha, B, T, D, scale, dq, nullptr, dy, srk::as_stream(stream));
  SRK_API_END
}

}  // extern "C"
