// Per-channel energy normalisation (include/srk.h srk_pcen_fwd / _bwd; nn.PCEN): each band of a [T][C] feature
// map is divided by a smoothed version of its own recent energy and root-compressed, every constant learned per
// band.  Per column (clip b, channel c), with alpha, delta, r = exp(p[0..2][c]) and s = sigmoid(p[3][c]):
//   E[t] = exp(k x[t]) (k = log_scale; k == 0: E = x),  M[0] = E[0],  M[t] = (1 - s) M[t-1] + s E[t],
//   u = eps + M[t],  g = E[t] u^-alpha,  v = g + delta,  y[t] = v^r - delta^r.
//
// The smoother is a first-order recurrence along time and nothing couples two columns, so one thread owns one
// column, the column index flattened over b C + c (C = 120 leaves no lanes idle and consecutive lanes still read
// consecutive addresses inside a clip).  The dependent chain is one FMA per step; exp, log and the two powers
// (exp(a log u)) are off it.  A wave is a workgroup: B C / 64 waves spread over every CU, and at the plugin's
// 512 x 120 that is about one wave per SIMD, so the loads in flight per wave are what hides latency — the time
// loop runs in chunks of 14 steps (98 = 7 x 14): the chunk's loads are issued first, then the arithmetic; steps
// past the last whole chunk run one at a time.
//
//  * pcen_fwd_kernel: forward scan; M is written only when the caller will run the backward.
//  * pcen_bwd_kernel: reverse scan G[t] = du[t] + (1 - s) G[t+1] from t = T - 1, recomputing E, u, g, v from x and
//    the saved M; writes dx (optional) and each column's four parameter sums (float64 accumulators, in time
//    order) to ws[4][B C].
//  * pcen_dp_kernel: sums ws over the clips in a fixed order (16 row groups in index order, then the groups in
//    index order) and applies the chain rule to the raw parameters.  No atomics: equal inputs give equal bits.
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kBlock = 64;      // one wave per workgroup
constexpr int kChunk = 14;      // time steps whose loads are issued together
constexpr int kMaxT = 1024;     // the entry points' domain
constexpr int kMaxC = 1024;
constexpr int kDpCols = 64;     // pcen_dp_kernel: channels per workgroup ...
constexpr int kDpGroups = 16;   // ... times groups of clips

struct Consts {
  float alpha, delta, r, s, oms, ld, dr;   // oms = 1 - s, ld = log delta, dr = delta^r
};

__device__ __forceinline__ Consts load_consts(const float* __restrict__ p, int C, int c) {
  Consts k;
  k.alpha = expf(p[c]);
  k.ld = p[C + c];
  k.delta = expf(k.ld);
  k.r = expf(p[2 * C + c]);
  k.s = 1.f / (1.f + expf(-p[3 * C + c]));
  k.oms = 1.f - k.s;
  k.dr = expf(k.r * k.ld);
  return k;
}

template <bool DB>
__device__ __forceinline__ float energy(float x, float log_scale) {
  return DB ? expf(log_scale * x) : x;
}

// one forward step at a known E and M[t]
__device__ __forceinline__ float compress(const Consts& k, float E, float M, float eps) {
  const float g = E * expf(-k.alpha * logf(eps + M));
  return expf(k.r * logf(g + k.delta)) - k.dr;
}

template <bool DB, bool WRITE_M>
__global__ __launch_bounds__(kBlock) void pcen_fwd_kernel(const float* __restrict__ x, const float* __restrict__ p,
                                                          int cols, int T, int C, float log_scale, float eps,
                                                          float* __restrict__ y, float* __restrict__ m_out) {
  const int j = blockIdx.x * kBlock + threadIdx.x;   // column b C + c
  if (j >= cols) return;
  const int b = j / C, c = j - b * C;
  const Consts k = load_consts(p, C, c);
  const size_t base = (size_t)b * T * C + c;   // element (b, 0, c); step t is C * t further
  float M = 0.f;
  int t0 = 0;
  for (; t0 + kChunk <= T; t0 += kChunk) {
    float xs[kChunk];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) xs[i] = x[base + (size_t)(t0 + i) * C];
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const float E = energy<DB>(xs[i], log_scale);
      M = (t0 + i == 0) ? E : fmaf(k.oms, M, k.s * E);
      const size_t at = base + (size_t)(t0 + i) * C;
      y[at] = compress(k, E, M, eps);
      if (WRITE_M) m_out[at] = M;
    }
  }
  for (int t = t0; t < T; ++t) {
    const size_t at = base + (size_t)t * C;
    const float E = energy<DB>(x[at], log_scale);
    M = (t == 0) ? E : fmaf(k.oms, M, k.s * E);
    y[at] = compress(k, E, M, eps);
    if (WRITE_M) m_out[at] = M;
  }
}

// the four parameter sums of one column and the scan's carry
struct BwdState {
  double d_alpha = 0.0, d_delta = 0.0, d_r = 0.0, d_s = 0.0;
  float G = 0.f;   // G[t + 1]
};

// One reverse step at time t: x[t], M[t], M[t - 1] (unused at t == 0) and dy[t] -> dx[t].
template <bool DB>
__device__ __forceinline__ float bwd_step(const Consts& k, BwdState& st, int t, float xv, float Mt, float Mprev,
                                          float dyv, float log_scale, float eps) {
  const float E = energy<DB>(xv, log_scale);
  const float u = eps + Mt;
  const float lu = logf(u);
  const float ua = expf(-k.alpha * lu);   // u^-alpha
  const float g = E * ua;
  const float v = g + k.delta;
  const float lv = logf(v);
  const float vr = expf(k.r * lv);        // v^r
  const float dv = dyv * k.r * vr / v;
  st.d_r += (double)(dyv * (vr * lv - k.dr * k.ld));
  st.d_delta += (double)(dv - dyv * k.r * k.dr / k.delta);
  st.d_alpha += (double)(-(dv * g) * lu);
  const float du = -k.alpha * dv * g / u;
  const float G = fmaf(k.oms, st.G, du);
  st.G = G;
  float dE = dv * ua;
  if (t > 0) {
    dE = fmaf(k.s, G, dE);
    st.d_s += (double)(G * (E - Mprev));
  } else {
    dE += G;
  }
  return DB ? dE * E * log_scale : dE;
}

template <bool DB, bool WRITE_DX>
__global__ __launch_bounds__(kBlock) void pcen_bwd_kernel(const float* __restrict__ x, const float* __restrict__ p,
                                                          const float* __restrict__ m, const float* __restrict__ dy,
                                                          int cols, int T, int C, float log_scale, float eps,
                                                          float* __restrict__ dx, float* __restrict__ ws) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= cols) return;
  const int b = j / C, c = j - b * C;
  const Consts k = load_consts(p, C, c);
  const size_t base = (size_t)b * T * C + c;
  BwdState st;
  const int whole = (T / kChunk) * kChunk;   // steps [0, whole) run in chunks, [whole, T) one at a time, first
  float Mt = m[base + (size_t)(T - 1) * C];  // M[t] of the step about to run: the step before hands down M[t - 1]
  for (int t = T - 1; t >= whole; --t) {
    const size_t at = base + (size_t)t * C;
    const float Mprev = t > 0 ? m[at - C] : 0.f;
    const float r = bwd_step<DB>(k, st, t, x[at], Mt, Mprev, dy[at], log_scale, eps);
    if (WRITE_DX) dx[at] = r;
    Mt = Mprev;
  }
  for (int t0 = whole - kChunk; t0 >= 0; t0 -= kChunk) {
    float xs[kChunk], ds[kChunk], ms[kChunk];   // ms[i] = M[t0 + i - 1]
#pragma unroll
    for (int i = 0; i < kChunk; ++i) {
      const size_t at = base + (size_t)(t0 + i) * C;
      xs[i] = x[at];
      ds[i] = dy[at];
      ms[i] = m[t0 + i > 0 ? at - C : at];      // t == 0 has no predecessor: any in-bounds word, never used
    }
#pragma unroll
    for (int i = kChunk - 1; i >= 0; --i) {
      const float r = bwd_step<DB>(k, st, t0 + i, xs[i], Mt, ms[i], ds[i], log_scale, eps);
      if (WRITE_DX) dx[base + (size_t)(t0 + i) * C] = r;
      Mt = ms[i];
    }
  }
  ws[j] = (float)st.d_alpha;
  ws[(size_t)cols + j] = (float)st.d_delta;
  ws[2 * (size_t)cols + j] = (float)st.d_r;
  ws[3 * (size_t)cols + j] = (float)st.d_s;
}

// dp[q][c] = (sum over b of ws[q][b C + c]) * d(constant q)/d(raw parameter q).  Grid (ceil(C / 64), 4).
__global__ __launch_bounds__(kDpCols* kDpGroups) void pcen_dp_kernel(const float* __restrict__ ws,
                                                                     const float* __restrict__ p, int B, int C,
                                                                     float* __restrict__ dp) {
  __shared__ double part[kDpGroups][kDpCols];
  const int lane = threadIdx.x & (kDpCols - 1), grp = threadIdx.x / kDpCols;
  const int c = blockIdx.x * kDpCols + lane, q = blockIdx.y;
  double acc = 0.0;
  if (c < C) {
    const float* col = ws + (size_t)q * B * C + c;
#pragma unroll 8
    for (int b = grp; b < B; b += kDpGroups) acc += (double)col[(size_t)b * C];
  }
  part[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && c < C) {
    double sum = part[0][lane];
#pragma unroll
    for (int g = 1; g < kDpGroups; ++g) sum += part[g][lane];
    const float raw = p[q * C + c];
    float chain;
    if (q < 3) {
      chain = expf(raw);   // d exp(raw) / d raw
    } else {
      const float s = 1.f / (1.f + expf(-raw));
      chain = s * (1.f - s);
    }
    dp[q * C + c] = (float)(sum * (double)chain);
  }
}

int check(const char* fn, int64_t B, int64_t T, int64_t C, float log_scale, float eps) {
  SRK_REQUIRE(B >= 1 && T >= 1 && T <= kMaxT && C >= 1 && C <= kMaxC, SRK_ERR_INVALID,
              "%s: needs B >= 1, 1 <= T <= 1024, 1 <= C <= 1024, got B %lld T %lld C %lld", fn, (long long)B,
              (long long)T, (long long)C);
  SRK_REQUIRE(B < (int64_t(1) << 31) / (T * C) + 1 && B * T * C < (int64_t(1) << 31), SRK_ERR_INVALID,
              "%s: B T C must stay below 2^31, got B %lld T %lld C %lld", fn, (long long)B, (long long)T,
              (long long)C);
  SRK_REQUIRE(std::isfinite(eps) && eps > 0.f, SRK_ERR_INVALID, "%s: eps must be finite and > 0", fn);
  SRK_REQUIRE(std::isfinite(log_scale), SRK_ERR_INVALID, "%s: log_scale is not finite", fn);
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int64_t srk_pcen_workspace_floats(int64_t B, int64_t T, int64_t C) {
  (void)T;
  if (B < 1 || C < 1) return 0;
  return 4 * B * C;   // each column's four parameter sums
}

int srk_pcen_fwd(const float* x, const float* p, int64_t B, int64_t T, int64_t C, float log_scale, float eps, float* y,
                 float* m_out, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  if (int rc = check("pcen_fwd", B, T, C, log_scale, eps)) return rc;
  SRK_REQUIRE(x && p && y, SRK_ERR_INVALID, "pcen_fwd: null pointer");
  hipStream_t s = as_stream(stream);
  const int cols = (int)(B * C);
  const double bytes = 4.0 * ((double)B * T * C * (m_out ? 3.0 : 2.0) + 4.0 * C);
  ProfScope prof("pcen", s, bytes);
  prof.bytes(bytes);
  prof.detail("pcen_fwd_kernel<%s%s> %lldx%lldx%lld", log_scale != 0.f ? "exp" : "lin", m_out ? ",m" : "",
              (long long)B, (long long)T, (long long)C);
  const dim3 grid((unsigned)((cols + kBlock - 1) / kBlock)), block(kBlock);
#define SRK_PCEN_FWD(DB, WM)                                                                                   \
  hipLaunchKernelGGL((pcen_fwd_kernel<DB, WM>), grid, block, 0, s, x, p, cols, (int)T, (int)C, log_scale, eps, \
                     y, m_out)
  if (log_scale != 0.f) {
    if (m_out) SRK_PCEN_FWD(true, true);
    else SRK_PCEN_FWD(true, false);
  } else {
    if (m_out) SRK_PCEN_FWD(false, true);
    else SRK_PCEN_FWD(false, false);
  }
#undef SRK_PCEN_FWD
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_pcen_bwd(const float* x, const float* p, const float* m, const float* dy, int64_t B, int64_t T, int64_t C,
                 float log_scale, float eps, float* dx, float* dp, float* ws, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  if (int rc = check("pcen_bwd", B, T, C, log_scale, eps)) return rc;
  SRK_REQUIRE(x && p && m && dy && dp && ws, SRK_ERR_INVALID, "pcen_bwd: null pointer");
  hipStream_t s = as_stream(stream);
  const int cols = (int)(B * C);
  {
    const double bytes = 4.0 * ((double)B * T * C * (dx ? 4.0 : 3.0) + 4.0 * C + 4.0 * cols);
    ProfScope prof("pcen", s, bytes);
    prof.bytes(bytes);
    prof.detail("pcen_bwd_kernel<%s%s> %lldx%lldx%lld", log_scale != 0.f ? "exp" : "lin", dx ? ",dx" : "",
                (long long)B, (long long)T, (long long)C);
    const dim3 grid((unsigned)((cols + kBlock - 1) / kBlock)), block(kBlock);
#define SRK_PCEN_BWD(DB, WX)                                                                                      \
  hipLaunchKernelGGL((pcen_bwd_kernel<DB, WX>), grid, block, 0, s, x, p, m, dy, cols, (int)T, (int)C, log_scale, \
                     eps, dx, ws)
    if (log_scale != 0.f) {
      if (dx) SRK_PCEN_BWD(true, true);
      else SRK_PCEN_BWD(true, false);
    } else {
      if (dx) SRK_PCEN_BWD(false, true);
      else SRK_PCEN_BWD(false, false);
    }
#undef SRK_PCEN_BWD
    SRK_CHECK_HIP(hipGetLastError());
  }
  {
    const double bytes = 4.0 * (4.0 * cols + 8.0 * C);
    ProfScope prof("pcen", s, bytes);
    prof.bytes(bytes);
    prof.detail("pcen_dp_kernel %lldx%lld", (long long)B, (long long)C);
    const dim3 grid((unsigned)((C + kDpCols - 1) / kDpCols), 4), block(kDpCols * kDpGroups);
    hipLaunchKernelGGL(pcen_dp_kernel, grid, block, 0, s, ws, p, (int)B, (int)C, dp);
    SRK_CHECK_HIP(hipGetLastError());
  }
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
