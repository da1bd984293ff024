// Multi-head self-attention core (include/srk.h srk_mhsa_fwd / _bwd; nn.MultiheadSelfAttention): per (clip b, head h)
//   S = scale Q K^T,  P = softmax over each row of S (row maximum subtracted),  O = P V
// on the packed projection qkv [B][T][3 D] (D = H dh; columns [0, D) q, [D, 2D) k, [2D, 3D) v, head h owning columns
// h dh .. (h + 1) dh - 1 of each third), O written as o [B][T][D] with the heads side by side: no transposes.
// fp32 VALU arithmetic at every matmul precision; 1 <= T <= 128, dh % 4 == 0, 4 <= dh <= 64.
//
// One workgroup of 8 waves owns a (b, h).  Two [T][dh + 4] operands sit in LDS (the + 4 keeps 16-byte rows and
// spreads eight lanes' float4 row reads over all banks); a wave takes one PIVOT row at a time (staged into the wave's
// own LDS slice and read back as a broadcast) and works in two lane layouts:
//   rows:    lane c (and c + 64) owns row c of an LDS operand and computes dot(pivot, row c)  -> S, dP
//   columns: lane d < dh owns column d and computes sum_c w[c] M[c][d] with w broadcast from the wave's slice -> O, dQ, dK, dV
// Forward: K, V in LDS, pivot = q_i; writes o_i and the row's log-sum-exp lse[b][h][i] (all the backward needs: P is
// recomputed as exp(s - lse)).
// Backward, phase A (K, V in LDS; pivot = q_i, dO_i):  p, dp = dO_i V^T,  D_i = sum_c p_c dp_c  (= rowsum(dO o O),
//   so O is not read),  ds = p (dp - D_i),  dQ_i = scale ds K.   Phase B (Q, dO in LDS; pivot = k_j, v_j): the
//   column j of P and dS recomputed with lane = query row,  dV_j = sum_i p_ij dO_i,  dK_j = scale sum_i ds_ij Q_i.
// dK and dV sum over the query rows inside one wave, so every sum has a fixed order and nothing is atomic: equal
// inputs give equal bits.  Staging uses float4 global loads when every tensor is 16-byte aligned, scalar ones otherwise.
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxT = 128;
constexpr int kMaxDh = 64;
constexpr int kFwdSlice = kMaxDh + kMaxT;            // per wave: pivot q, weights p
constexpr int kBwdSlice = 2 * kMaxDh + 2 * kMaxT;    // per wave: two pivots, two weight rows

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

// Orders this wave's LDS traffic: what its lanes wrote before is visible to all of them after.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// T rows of dh floats from global (row stride ldg) into LDS rows of stride ld, by the whole workgroup
template <bool VEC>
__device__ __forceinline__ void stage(const float* __restrict__ g, size_t ldg, float* s, int ld, int T, int dh) {
  if (VEC) {
    const int c4 = dh >> 2;
    for (int i = threadIdx.x; i < T * c4; i += kThreads) {
      const int t = i / c4, c = i - t * c4;
      *reinterpret_cast<float4*>(s + t * ld + 4 * c) = *reinterpret_cast<const float4*>(g + (size_t)t * ldg + 4 * c);
    }
  } else {
    for (int i = threadIdx.x; i < T * dh; i += kThreads) {
      const int t = i / dh, c = i - t * dh;
      s[t * ld + c] = g[(size_t)t * ldg + c];
    }
  }
}

// dot over dh of the wave's pivot (a broadcast read) with this lane's LDS row
__device__ __forceinline__ float dot_row(const float* piv, const float* row, int dh) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  for (int d = 0; d < dh; d += 4) {
    const float4 p = *reinterpret_cast<const float4*>(piv + d), r = *reinterpret_cast<const float4*>(row + d);
    a0 += p.x * r.x;
    a1 += p.y * r.y;
    a2 += p.z * r.z;
    a3 += p.w * r.w;
  }
  return (a0 + a1) + (a2 + a3);
}

// sum_c w[c] M[c][d] over the T rows for this lane's column d (w: a broadcast read)
__device__ __forceinline__ float col_sum(const float* w, const float* M, int ld, int T, int d) {
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int c = 0;
  for (; c + 4 <= T; c += 4) {
    const float4 wv = *reinterpret_cast<const float4*>(w + c);
    a0 += wv.x * M[c * ld + d];
    a1 += wv.y * M[(c + 1) * ld + d];
    a2 += wv.z * M[(c + 2) * ld + d];
    a3 += wv.w * M[(c + 3) * ld + d];
  }
  for (; c < T; ++c) a0 += w[c] * M[c * ld + d];
  return (a0 + a1) + (a2 + a3);
}

inline size_t fwd_lds_bytes(int T, int dh) { return 4 * ((size_t)2 * T * (dh + 4) + kWaves * kFwdSlice); }
inline size_t bwd_lds_bytes(int T, int dh) { return 4 * ((size_t)2 * T * (dh + 4) + 2 * kMaxT + kWaves * kBwdSlice); }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void mhsa_fwd_kernel(const float* __restrict__ qkv, int H, int T, int dh,
                                                            float scale, float* __restrict__ o,
                                                            float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ld = dh + 4, D = H * dh;
  const size_t ldg = (size_t)3 * D;
  float* Ks = smem;
  float* Vs = Ks + T * ld;
  float* q = Vs + T * ld + wave * kFwdSlice;
  float* pw = q + kMaxDh;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const float* base = qkv + (size_t)b * T * ldg + (size_t)h * dh;

  stage<VEC>(base + D, ldg, Ks, ld, T, dh);
  stage<VEC>(base + 2 * D, ldg, Vs, ld, T, dh);
  __syncthreads();

  const int c0 = lane, c1 = lane + 64;
  for (int i = wave; i < T; i += kWaves) {   // (wave-uniform)
    wave_sync();   // the previous row's reads of q and pw are done
    if (lane < dh) q[lane] = base[(size_t)i * ldg + lane];
    wave_sync();
    const float s0 = c0 < T ? scale * dot_row(q, Ks + c0 * ld, dh) : -INFINITY;
    const float s1 = c1 < T ? scale * dot_row(q, Ks + c1 * ld, dh) : -INFINITY;
    const float m = wave_max(fmaxf(s0, s1));
    const float e0 = c0 < T ? expf(s0 - m) : 0.f, e1 = c1 < T ? expf(s1 - m) : 0.f;
    const float sum = wave_sum(e0 + e1);
    pw[c0] = e0 / sum;
    pw[c1] = e1 / sum;
    if (lane == 0) lse[((size_t)b * H + h) * T + i] = m + logf(sum);
    wave_sync();
    if (lane < dh) o[((size_t)b * T + i) * D + (size_t)h * dh + lane] = col_sum(pw, Vs, ld, T, lane);
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void mhsa_bwd_kernel(const float* __restrict__ qkv,
                                                            const float* __restrict__ lse,
                                                            const float* __restrict__ dO, int H, int T, int dh,
                                                            float scale, float* __restrict__ dqkv) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ld = dh + 4, D = H * dh;
  const size_t ldg = (size_t)3 * D;
  float* A1 = smem;                 // phase A: K; phase B: Q
  float* A2 = A1 + T * ld;          // phase A: V; phase B: dO
  float* Ls = A2 + T * ld;          // [kMaxT] this head's lse
  float* Dd = Ls + kMaxT;           // [kMaxT] D_i, written in phase A
  float* piv1 = Dd + kMaxT + wave * kBwdSlice;
  float* piv2 = piv1 + kMaxDh;
  float* w1 = piv2 + kMaxDh;
  float* w2 = w1 + kMaxT;
  const int b = blockIdx.x / H, h = blockIdx.x - b * H;
  const float* base = qkv + (size_t)b * T * ldg + (size_t)h * dh;
  const float* dOb = dO + (size_t)b * T * D + (size_t)h * dh;
  float* dbase = dqkv + (size_t)b * T * ldg + (size_t)h * dh;
  const int c0 = lane, c1 = lane + 64;

  stage<VEC>(base + D, ldg, A1, ld, T, dh);
  stage<VEC>(base + 2 * D, ldg, A2, ld, T, dh);
  for (int t = threadIdx.x; t < T; t += kThreads) Ls[t] = lse[((size_t)b * H + h) * T + t];
  __syncthreads();

  // phase A: pivot = query row i; lanes own keys
  for (int i = wave; i < T; i += kWaves) {   // (wave-uniform)
    wave_sync();
    if (lane < dh) {
      piv1[lane] = base[(size_t)i * ldg + lane];
      piv2[lane] = dOb[(size_t)i * D + lane];
    }
    wave_sync();
    const float li = Ls[i];
    float p0 = 0.f, p1 = 0.f, dp0 = 0.f, dp1 = 0.f;
    if (c0 < T) {
      p0 = expf(scale * dot_row(piv1, A1 + c0 * ld, dh) - li);
      dp0 = dot_row(piv2, A2 + c0 * ld, dh);
    }
    if (c1 < T) {
      p1 = expf(scale * dot_row(piv1, A1 + c1 * ld, dh) - li);
      dp1 = dot_row(piv2, A2 + c1 * ld, dh);
    }
    const float Di = wave_sum(p0 * dp0 + p1 * dp1);
    w2[c0] = p0 * (dp0 - Di);
    w2[c1] = p1 * (dp1 - Di);
    if (lane == 0) Dd[i] = Di;
    wave_sync();
    if (lane < dh) dbase[(size_t)i * ldg + lane] = scale * col_sum(w2, A1, ld, T, lane);
  }
  __syncthreads();

  stage<VEC>(base, ldg, A1, ld, T, dh);
  stage<VEC>(dOb, (size_t)D, A2, ld, T, dh);
  __syncthreads();

  // phase B: pivot = key row j; lanes own query rows
  for (int j = wave; j < T; j += kWaves) {   // (wave-uniform)
    wave_sync();
    if (lane < dh) {
      piv1[lane] = base[(size_t)j * ldg + D + lane];
      piv2[lane] = base[(size_t)j * ldg + 2 * D + lane];
    }
    wave_sync();
    float p0 = 0.f, p1 = 0.f, ds0 = 0.f, ds1 = 0.f;
    if (c0 < T) {
      p0 = expf(scale * dot_row(piv1, A1 + c0 * ld, dh) - Ls[c0]);
      ds0 = p0 * (dot_row(piv2, A2 + c0 * ld, dh) - Dd[c0]);
    }
    if (c1 < T) {
      p1 = expf(scale * dot_row(piv1, A1 + c1 * ld, dh) - Ls[c1]);
      ds1 = p1 * (dot_row(piv2, A2 + c1 * ld, dh) - Dd[c1]);
    }
    w1[c0] = p0;
    w1[c1] = p1;
    w2[c0] = ds0;
    w2[c1] = ds1;
    wave_sync();
    if (lane < dh) {
      dbase[(size_t)j * ldg + 2 * D + lane] = col_sum(w1, A2, ld, T, lane);
      dbase[(size_t)j * ldg + D + lane] = scale * col_sum(w2, A1, ld, T, lane);
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_shape(const char* who, int64_t B, int64_t H, int64_t T, int64_t dh, float scale) {
  SRK_REQUIRE(B >= 1 && H >= 1 && T >= 1 && T <= kMaxT && dh >= 4 && dh <= kMaxDh && dh % 4 == 0, SRK_ERR_INVALID,
              "mhsa_%s: needs B, H >= 1, 1 <= T <= 128, dh in 4..64 and a multiple of 4, got B %lld H %lld T %lld dh %lld",
              who, (long long)B, (long long)H, (long long)T, (long long)dh);
  const int64_t lim = 1LL << 31;
  // B H and B T 3 H dh below 2^31, without overflowing on the way (T dh 3 <= 24576)
  SRK_REQUIRE(B < lim && H < lim && B * H < lim && B * H * (3 * T * dh) < lim, SRK_ERR_INVALID,
              "mhsa_%s: qkv needs fewer than 2^31 elements, got B %lld H %lld T %lld dh %lld", who, (long long)B,
              (long long)H, (long long)T, (long long)dh);
  SRK_REQUIRE(std::isfinite(scale), SRK_ERR_INVALID, "mhsa_%s: scale is not finite", who);
  return SRK_OK;
}

// Raises the dynamic-LDS limit of all four kernels (both directions, float4 and scalar staging) to the domain's
// largest need, once per device and process: the first call of either entry point does it for every variant, so a
// variant first reached inside a stream capture (a misaligned tensor after an aligned warm-up) finds it done.
int raise_lds() {
  static std::atomic<uint64_t> done{0};   // bit per device index
  int dev = 0;
  SRK_CHECK_HIP(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return SRK_OK;
  const int fwd = (int)fwd_lds_bytes(kMaxT, kMaxDh), bwd = (int)bwd_lds_bytes(kMaxT, kMaxDh);
  const hipFuncAttribute attr = hipFuncAttributeMaxDynamicSharedMemorySize;
  SRK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_fwd_kernel<true>), attr, fwd));
  SRK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_fwd_kernel<false>), attr, fwd));
  SRK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_bwd_kernel<true>), attr, bwd));
  SRK_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mhsa_bwd_kernel<false>), attr, bwd));
  done.fetch_or(bit, std::memory_order_release);
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_mhsa_fwd(const float* qkv, int64_t B, int64_t H, int64_t T, int64_t dh, float scale, float* o, float* lse,
                 void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_shape("fwd", B, H, T, dh, scale)) return rc;
  SRK_REQUIRE(qkv && o && lse, SRK_ERR_INVALID, "mhsa_fwd: null pointer");
  using namespace srk;
  hipStream_t s = as_stream(stream);
  const bool vec = aligned16(qkv);   // o and lse are written by scalar stores
  const size_t lds = fwd_lds_bytes((int)T, (int)dh);
  const double n = (double)B * T * H * dh;
  const double bytes = 4.0 * (4.0 * n + (double)B * H * T);
  ProfScope prof("mhsa", s, 4.0 * (double)B * H * T * T * dh);
  prof.bytes(bytes);
  prof.detail("mhsa_fwd_kernel<%s> %lldx%lldx%lldx%lld", vec ? "vec" : "scalar", (long long)B, (long long)H,
              (long long)T, (long long)dh);
  const dim3 grid((unsigned)(B * H)), block(kThreads);
  if (int rc = raise_lds()) return rc;
  if (vec)
    hipLaunchKernelGGL(mhsa_fwd_kernel<true>, grid, block, lds, s, qkv, (int)H, (int)T, (int)dh, scale, o, lse);
  else
    hipLaunchKernelGGL(mhsa_fwd_kernel<false>, grid, block, lds, s, qkv, (int)H, (int)T, (int)dh, scale, o, lse);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_mhsa_bwd(const float* qkv, const float* lse, const float* d_o, int64_t B, int64_t H, int64_t T, int64_t dh,
                 float scale, float* dqkv, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_shape("bwd", B, H, T, dh, scale)) return rc;
  SRK_REQUIRE(qkv && lse && d_o && dqkv, SRK_ERR_INVALID, "mhsa_bwd: null pointer");
  using namespace srk;
  hipStream_t s = as_stream(stream);
  const bool vec = aligned16(qkv) && aligned16(d_o);   // dqkv is written by scalar stores
  const size_t lds = bwd_lds_bytes((int)T, (int)dh);
  const double n = (double)B * T * H * dh;
  const double bytes = 4.0 * (7.0 * n + (double)B * H * T);
  ProfScope prof("mhsa", s, 10.0 * (double)B * H * T * T * dh);   // the five products; S and dP are formed twice
  prof.bytes(bytes);
  prof.detail("mhsa_bwd_kernel<%s> %lldx%lldx%lldx%lld", vec ? "vec" : "scalar", (long long)B, (long long)H,
              (long long)T, (long long)dh);
  const dim3 grid((unsigned)(B * H)), block(kThreads);
  if (int rc = raise_lds()) return rc;
  if (vec)
    hipLaunchKernelGGL(mhsa_bwd_kernel<true>, grid, block, lds, s, qkv, lse, d_o, (int)H, (int)T, (int)dh, scale,
                       dqkv);
  else
    hipLaunchKernelGGL(mhsa_bwd_kernel<false>, grid, block, lds, s, qkv, lse, d_o, (int)H, (int)T, (int)dh, scale,
                       dqkv);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
