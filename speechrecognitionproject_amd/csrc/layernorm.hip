// LayerNorm over the last dimension of [M][D] with an optional fused residual (include/srk.h srk_layernorm_fwd /
// _bwd; nn.LayerNorm):  s = x (+ res),  y = (s - mean) rstd gamma + beta,  rstd = 1 / sqrt(var + eps), var biased.
//
// A row lives in the registers of a group of G lanes (G a power of two <= 64, so a group never leaves its wave): the
// mean is summed first, then the centred squares of the same registers (never E[s^2] - mean^2), so x and res are read
// once.  Sums over a row are xor butterflies inside the group: a fixed order.  Memory bound: 256 threads carry
// 256 / G rows per sweep.
//
// Rows far from zero (mean 1e3, spread 1): the fp32 sum x + res and the fp32 mean each lose the spread's low bits.
// Both kernels therefore centre in two steps around a first estimate mu0 of the mean (forward: the plain mean;
// backward: the saved one):  t = (x - mu0) + res — x - mu0 is exact where it matters and res is added to a small
// number — then  c = t - mean_D(t), whose mean is zero to rounding of the SPREAD.  The saved mean is mu0 + mean_D(t).
//
// Backward:  g = dy gamma,  xhat = c rstd (recomputed from x, res and the saved statistics),
//   ds = rstd (g - mean_D(g) - xhat mean_D(g xhat)),   dgamma = sum_m dy xhat,   dbeta = sum_m dy.
// The plan below fixes the launch for (M, D): every workgroup sweeps its rows in a grid-stride loop keeping the column
// sums of its lanes in registers, adds its row groups in index order through LDS and writes one [2][D] slab into the
// caller's workspace; a second launch adds the slabs in a fixed two-level order (16 runs of consecutive slabs, each
// in index order, then the runs in index order) into dgamma / dbeta (written, or with acc_beta != 0 added to acc_beta
// times what is there).  No atomics anywhere: equal inputs give equal bits.
//
// float4 column slots when D % 4 == 0 and every row tensor is 16-byte aligned, scalar slots otherwise.
#include <cmath>
#include <type_traits>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxD = 1024;
constexpr int kMaxBlocks = 1024;   // backward workgroups = workspace slabs
constexpr int kItersVec = 4;       // column slots per lane: 64 lanes x 4 float4 = 1024 columns
constexpr int kItersScalar = 16;   // 64 lanes x 16 floats
constexpr int kRedFloats = kThreads * 16;   // per-thread column sums of one kind: 4 float4 or 16 floats

// The one launch plan of (M, D, vec): the workspace query, the forward and the backward all read it.
struct LnPlan {
  int G;                // lanes per row
  int rows_per_block;   // 256 / G
  int blocks_fwd;       // one sweep each
  int blocks_bwd;       // grid-stride; the number of workspace slabs
};

LnPlan ln_plan(int64_t M, int64_t D, bool vec) {
  const int64_t cols = vec ? D / 4 : D;
  LnPlan p;
  p.G = 1;
  while (p.G < 64 && p.G < cols) p.G <<= 1;
  p.rows_per_block = kThreads / p.G;
  const int64_t sweeps = (M + p.rows_per_block - 1) / p.rows_per_block;
  p.blocks_fwd = (int)sweeps;
  p.blocks_bwd = (int)(sweeps < kMaxBlocks ? sweeps : kMaxBlocks);
  return p;
}

// The slab count never depends on the alignment of the call: the scalar plan has the larger G for a D (fewer rows
// per block, more sweeps), so its count bounds the vector plan's.
int64_t ln_ws_floats(int64_t M, int64_t D) { return 2 * D * (int64_t)ln_plan(M, D, false).blocks_bwd; }

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ void vload(const float* p, float4& v) { v = *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void vload(const float* p, float& v) { v = *p; }
__device__ __forceinline__ void vstore(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void vstore(float* p, const float& v) { *p = v; }
__device__ __forceinline__ float4 vset(float4, float a) { return make_float4(a, a, a, a); }
__device__ __forceinline__ float vset(float, float a) { return a; }
// (float4 arithmetic below is HIP's own componentwise operators)
__device__ __forceinline__ float hsum(const float4& a) { return (a.x + a.y) + (a.z + a.w); }
__device__ __forceinline__ float hsum(const float& a) { return a; }

template <bool VEC>
__global__ __launch_bounds__(kThreads) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int64_t M, int D, int G,
                                                          float eps, float* __restrict__ y, float* __restrict__ mean,
                                                          float* __restrict__ rstd) {
  using V = typename std::conditional<VEC, float4, float>::type;
  constexpr int W = VEC ? 4 : 1, ITERS = VEC ? kItersVec : kItersScalar;
  const int cols = D / W;
  const int grp = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const int64_t row = (int64_t)blockIdx.x * (kThreads / G) + grp;
  const bool live = row < M;   // a dead group still takes part in its wave's shuffles
  const size_t off = (size_t)(live ? row : 0) * D;

  V s[ITERS], r[ITERS];   // x, then the centred row; res
  float sum = 0.f;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int c = it * G + gl;
    s[it] = r[it] = vset(V(), 0.f);
    if (live && c < cols) {
      vload(x + off + (size_t)c * W, s[it]);
      if (res) vload(res + off + (size_t)c * W, r[it]);
    }
    sum += hsum(s[it] + r[it]);
  }
  const float mu0 = group_sum(sum, G) / (float)D;
  float tsum = 0.f;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int c = it * G + gl;
    if (c < cols) {
      s[it] = (s[it] - vset(V(), mu0)) + r[it];
      tsum += hsum(s[it]);
    }
  }
  const float corr = group_sum(tsum, G) / (float)D;
  const float mu = mu0 + corr;
  float sq = 0.f;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int c = it * G + gl;
    if (c < cols) {
      s[it] = s[it] - vset(V(), corr);
      sq += hsum(s[it] * s[it]);
    }
  }
  const float rs = 1.0f / sqrtf(group_sum(sq, G) / (float)D + eps);
  if (!live) return;
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int c = it * G + gl;
    if (c < cols) {
      V g, b;
      vload(gamma + (size_t)c * W, g);
      vload(beta + (size_t)c * W, b);
      vstore(y + off + (size_t)c * W, s[it] * rs * g + b);
    }
  }
  if (gl == 0) {
    mean[row] = mu;
    rstd[row] = rs;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ rstd,
                                                          const float* __restrict__ dy, int64_t M, int D, int G,
                                                          float* __restrict__ ds, float* __restrict__ ws) {
  using V = typename std::conditional<VEC, float4, float>::type;
  constexpr int W = VEC ? 4 : 1, ITERS = VEC ? kItersVec : kItersScalar;
  __shared__ __attribute__((aligned(16))) float red[2][kRedFloats];   // [dgamma | dbeta][group][slot][lane][W]
  const int cols = D / W;
  const int rpb = kThreads / G;
  const int grp = threadIdx.x / G, gl = threadIdx.x & (G - 1);
  const float invD = 1.0f / (float)D;

  V dg[ITERS], db[ITERS];   // gamma is re-read per row (an L1 hit): 16 registers fewer on the scalar path
#pragma unroll
  for (int it = 0; it < ITERS; ++it) dg[it] = db[it] = vset(V(), 0.f);

  for (int64_t row0 = (int64_t)blockIdx.x * rpb; row0 < M; row0 += (int64_t)gridDim.x * rpb) {   // (uniform)
    const int64_t row = row0 + grp;
    const bool live = row < M;
    const size_t off = (size_t)(live ? row : 0) * D;
    const float mu = live ? mean[row] : 0.f, rs = live ? rstd[row] : 0.f;
    V xh[ITERS], g[ITERS];
    float tsum = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = it * G + gl;
      xh[it] = g[it] = vset(V(), 0.f);
      if (live && c < cols) {
        vload(x + off + (size_t)c * W, xh[it]);
        xh[it] = xh[it] - vset(V(), mu);
        if (res) {
          V r;
          vload(res + off + (size_t)c * W, r);
          xh[it] = xh[it] + r;
        }
        vload(dy + off + (size_t)c * W, g[it]);   // dy for now
      }
      tsum += hsum(xh[it]);
    }
    const float corr = group_sum(tsum, G) * invD;   // what the saved fp32 mean is off by
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int c = it * G + gl;
      if (live && c < cols) {
        const V d = g[it];
        V gam;
        vload(gamma + (size_t)c * W, gam);
        xh[it] = (xh[it] - vset(V(), corr)) * rs;
        g[it] = d * gam;
        dg[it] = dg[it] + d * xh[it];
        db[it] = db[it] + d;
      }
      s1 += hsum(g[it]);
      s2 += hsum(g[it] * xh[it]);
    }
    const float m1 = group_sum(s1, G) * invD, m2 = group_sum(s2, G) * invD;
    if (live) {
#pragma unroll
      for (int it = 0; it < ITERS; ++it) {
        const int c = it * G + gl;
        if (c < cols) vstore(ds + off + (size_t)c * W, (g[it] - vset(V(), m1) - xh[it] * m2) * rs);
      }
    }
  }

  // this workgroup's slab: the row groups' register sums added in group order
#pragma unroll
  for (int it = 0; it < ITERS; ++it) {
    const int slot = ((grp * ITERS + it) * G + gl) * W;
    vstore(&red[0][slot], dg[it]);
    vstore(&red[1][slot], db[it]);
  }
  __syncthreads();
  float* slab = ws + (size_t)blockIdx.x * 2 * D;
  for (int col = threadIdx.x; col < D; col += kThreads) {
    const int c = col / W, w = col - c * W;
    const int it = c / G, l = c - it * G;
    float a = 0.f, b = 0.f;
    for (int gi = 0; gi < rpb; ++gi) {
      const int slot = ((gi * ITERS + it) * G + l) * W + w;
      a += red[0][slot];
      b += red[1][slot];
    }
    slab[col] = a;
    slab[D + col] = b;
  }
}

// out[which][col] = acc_beta * out + sum over the slabs, in a fixed two-level order: kFinParts threads per
// (which, col) each add a run of consecutive slabs in index order, then the runs' sums are added in index order.
// A workgroup owns kFinCols consecutive values of the [2 D] slab row (64-byte reads per run).
constexpr int kFinCols = 16, kFinParts = kThreads / kFinCols;
__global__ __launch_bounds__(kThreads) void ln_finalize_kernel(const float* __restrict__ ws, int slabs, int D,
                                                               float acc_beta, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta) {
  __shared__ float part[kFinParts][kFinCols];
  const int c = threadIdx.x % kFinCols, p = threadIdx.x / kFinCols;
  const int i = blockIdx.x * kFinCols + c;
  const int run = (slabs + kFinParts - 1) / kFinParts;
  const int lo = p * run, hi = lo + run < slabs ? lo + run : slabs;
  float a = 0.f;
  if (i < 2 * D) {
#pragma unroll 4
    for (int sl = lo; sl < hi; ++sl) a += ws[(size_t)sl * 2 * D + i];
  }
  part[p][c] = a;
  __syncthreads();
  if (p != 0 || i >= 2 * D) return;
  float s = part[0][c];
#pragma unroll
  for (int q = 1; q < kFinParts; ++q) s += part[q][c];
  float* out = i < D ? dgamma + i : dbeta + (i - D);
  *out = acc_beta != 0.f ? acc_beta * *out + s : s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_shape(const char* who, int64_t M, int64_t D) {
  SRK_REQUIRE(M >= 1 && D >= 1 && D <= kMaxD && M < (1LL << 31) && M * D < (1LL << 31), SRK_ERR_INVALID,
              "layernorm_%s: needs M >= 1, 1 <= D <= 1024, M D < 2^31, got M %lld D %lld", who, (long long)M,
              (long long)D);
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int64_t srk_layernorm_workspace_floats(int64_t M, int64_t D) {
  if (M < 1 || D < 1 || D > srk::kMaxD || M >= (1LL << 31) || M * D >= (1LL << 31)) return 0;
  return srk::ln_ws_floats(M, D);
}

int srk_layernorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, int64_t M, int64_t D,
                      float eps, float* y, float* mean, float* rstd, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_shape("fwd", M, D)) return rc;
  SRK_REQUIRE(std::isfinite(eps) && eps >= 0.f, SRK_ERR_INVALID, "layernorm_fwd: eps must be finite and >= 0");
  SRK_REQUIRE(x && gamma && beta && y && mean && rstd, SRK_ERR_INVALID, "layernorm_fwd: null pointer");
  using namespace srk;
  hipStream_t s = as_stream(stream);
  const bool vec = D % 4 == 0 && aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(y) &&
                   (!res || aligned16(res));
  const LnPlan p = ln_plan(M, D, vec);
  const double bytes = 4.0 * ((res ? 3.0 : 2.0) * (double)M * D + 2.0 * D + 2.0 * M);
  ProfScope prof("layernorm", s, bytes);
  prof.bytes(bytes);
  prof.detail("ln_fwd_kernel<%s%s> %lldx%lld G%d", vec ? "vec" : "scalar", res ? ",res" : "", (long long)M,
              (long long)D, p.G);
  const dim3 grid((unsigned)p.blocks_fwd), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(ln_fwd_kernel<true>, grid, block, 0, s, x, res, gamma, beta, M, (int)D, p.G, eps, y, mean, rstd);
  else
    hipLaunchKernelGGL(ln_fwd_kernel<false>, grid, block, 0, s, x, res, gamma, beta, M, (int)D, p.G, eps, y, mean,
                       rstd);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_layernorm_bwd(const float* x, const float* res, const float* gamma, const float* mean, const float* rstd,
                      const float* dy, int64_t M, int64_t D, float* ds, float* dgamma, float* dbeta, float acc_beta,
                      float* ws, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_shape("bwd", M, D)) return rc;
  SRK_REQUIRE(std::isfinite(acc_beta), SRK_ERR_INVALID, "layernorm_bwd: acc_beta is not finite");
  SRK_REQUIRE(x && gamma && mean && rstd && dy && ds && dgamma && dbeta && ws, SRK_ERR_INVALID,
              "layernorm_bwd: null pointer");
  using namespace srk;
  hipStream_t s = as_stream(stream);
  const bool vec = D % 4 == 0 && aligned16(x) && aligned16(gamma) && aligned16(dy) && aligned16(ds) &&
                   (!res || aligned16(res));
  const LnPlan p = ln_plan(M, D, vec);
  // the slab count is the workspace's (ln_ws_floats), whichever path the alignment picks: every slab is written (a
  // workgroup beyond the vector plan's sweeps writes zeros)
  const int slabs = ln_plan(M, D, false).blocks_bwd;
  const double bytes = 4.0 * ((res ? 4.0 : 3.0) * (double)M * D + 3.0 * D + 2.0 * M);
  ProfScope prof("layernorm", s, bytes);   // both launches: one record per backward
  prof.bytes(bytes);
  prof.detail("ln_bwd_kernel<%s%s> %lldx%lld G%d slabs %d", vec ? "vec" : "scalar", res ? ",res" : "", (long long)M,
              (long long)D, p.G, slabs);
  const dim3 grid((unsigned)slabs), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(ln_bwd_kernel<true>, grid, block, 0, s, x, res, gamma, mean, rstd, dy, M, (int)D, p.G, ds, ws);
  else
    hipLaunchKernelGGL(ln_bwd_kernel<false>, grid, block, 0, s, x, res, gamma, mean, rstd, dy, M, (int)D, p.G, ds, ws);
  SRK_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(ln_finalize_kernel, dim3((unsigned)((2 * D + kFinCols - 1) / kFinCols)), block, 0, s, ws, slabs,
                     (int)D, acc_beta, dgamma, dbeta);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
