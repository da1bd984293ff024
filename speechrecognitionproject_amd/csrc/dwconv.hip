// Depthwise 2-D convolution and global average pool on channels-last fp32 tensors (include/srk.h
// srk_dwconv2d_nhwc_fwd / _bwd, srk_avgpool_nhwc_fwd / _bwd; nn.DepthwiseConv2d, nn.GlobalAvgPool2d): the two
// primitives of a depthwise-separable CNN block the implicit-GEMM convolutions (K6, no groups) do not cover.
//
// A depthwise conv has KH KW multiply-adds per output element and no reduction over channels: there is no GEMM in
// it, the matrix cores have nothing to do and the kernels are bound by memory.  Lanes run along C (the contiguous
// axis), each lane owning 4 consecutive channels as one 16-byte load / store when C % 4 == 0 and every pointer is
// 16-byte aligned, one channel otherwise.  fp32 at every matmul precision.
//
//  * dwconv_fwd_kernel: a thread owns 4 consecutive output columns of one output row (3 x 3, the tuned case: each
//    input row's 6 (stride 1) or 9 (stride 2) columns are loaded once into registers and shared by the 4 outputs and
//    3 taps; its 36 weights are 9 float4 loads) or one output (every other kernel size, taps looped at run time).
//    Neighbouring threads' overlapping rows come from L1 / L2, so HBM sees x about once.  Padding taps are selected
//    to 0 after a load from a clamped (in-bounds, same clip) address.
//  * dwconv_dgrad3_kernel / dwconv_dgrad_kernel: the gather form.  A dx element sums the taps whose output position
//    exists: th = hi + ph - kh must be >= 0, a multiple of sh (parity test: sh is 1 or 2) and th / sh < Ho, the same
//    along W.  dx is written once, in full; no zero fill, no atomics.  3 x 3 (stride 2 along W with pw = 1) runs on
//    the forward's register tile transposed, 4 dx columns per thread with every load issued up front; every other
//    geometry on one element group per thread with the taps looped at run time.
//  * dwconv_wgrad_kernel + dwconv_wgrad_reduce_kernel: the output pixels are cut into at most 1024 contiguous
//    chunks, one per workgroup.  A workgroup is (256 / cols) pixel rows x cols channel groups; a thread walks its
//    chunk's pixels in index order with the partial sums of up to 9 taps (one tap group; blockIdx.y counts the groups,
//    so a 7 x 7 kernel makes 6 passes over x and dY instead of holding 49 x 4 partials) and of db in registers, the
//    rows are summed through LDS in row order, and the workgroup writes its slab ws[chunk][KH KW + 1][C].  The second
//    launch sums the slabs in a fixed order (4 interleaved groups in chunk order, then the groups in order) and
//    writes or adds (dw_accumulate) dw in torch's [C][1][KH][KW] layout and writes db.  No atomics anywhere: equal
//    inputs give equal bits.
//  * avgpool_fwd_kernel: one workgroup per (clip, 64 channel groups): rows stride the HW positions, LDS sum in row
//    order, divided by HW.  avgpool_bwd_kernel: dx = dy / HW, one thread per element group.
#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxK = 7;        // the entry points' domain: 1 <= KH, KW <= 7
constexpr int kTapGroup = 9;    // weight-gradient taps whose partial sums a thread keeps in registers
constexpr int kMaxSlabs = 1024; // weight-gradient workgroups along the pixels (4 per CU)
constexpr int kMaxCols = 64;    // channel groups per workgroup in the reducing kernels
constexpr int kRedCols = 64;    // dwconv_wgrad_reduce_kernel: slab entries per workgroup ...
constexpr int kRedGroups = 4;   // ... times interleaved groups of slabs

struct Geom {
  int N, H, W, C, KH, KW, ph, pw, sh, sw, Ho, Wo;
};

template <int V>
struct Pack {
  float v[V];
};

template <int V>
__device__ __forceinline__ Pack<V> ld(const float* __restrict__ p) {
  Pack<V> r;
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

template <int V>
__device__ __forceinline__ void st(float* __restrict__ p, const Pack<V>& r) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  } else {
    *p = r.v[0];
  }
}

template <int V>
__device__ __forceinline__ Pack<V> zero() {
  Pack<V> r;
#pragma unroll
  for (int i = 0; i < V; ++i) r.v[i] = 0.f;
  return r;
}

// KH_ = KW_ = 3 with SW_ = 1 or 2: the unrolled 4-outputs-per-thread form; KH_ = 0: any kernel size and stride.
template <int V, int KH_, int KW_, int SW_>
__global__ __launch_bounds__(kBlock) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, Geom g, int total,
                                                            float* __restrict__ y) {
  constexpr int TW = KH_ ? 4 : 1;   // outputs per thread along Wo
  int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int CG = g.C / V, WQ = (g.Wo + TW - 1) / TW;
  const int cg = idx % CG;
  idx /= CG;
  const int wq = idx % WQ;
  idx /= WQ;
  const int ho = idx % g.Ho, n = idx / g.Ho;
  const int c0 = cg * V;
  const float* __restrict__ xn = x + (size_t)n * g.H * g.W * g.C + c0;
  const int hi0 = ho * g.sh - g.ph;
  Pack<V> acc[TW];
#pragma unroll
  for (int j = 0; j < TW; ++j) acc[j] = bias ? ld<V>(bias + c0) : zero<V>();

  if constexpr (KH_ != 0) {
    constexpr int KK = KH_ * KW_, ND = (TW - 1) * SW_ + KW_;   // ND: input columns under the thread's outputs
    float wr[V * KK];   // channel i, tap t at i KK + t: contiguous in w
    if constexpr (V == 4) {
#pragma unroll
      for (int q = 0; q < KK; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(w + (size_t)c0 * KK + 4 * q);
        wr[4 * q] = t.x, wr[4 * q + 1] = t.y, wr[4 * q + 2] = t.z, wr[4 * q + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int q = 0; q < KK; ++q) wr[q] = w[(size_t)c0 * KK + q];
    }
    const int wi0 = wq * TW * SW_ - g.pw;
#pragma unroll
    for (int kh = 0; kh < KH_; ++kh) {
      const int hi = hi0 + kh;
      const bool hok = (unsigned)hi < (unsigned)g.H;
      const float* __restrict__ row = xn + (size_t)min(max(hi, 0), g.H - 1) * g.W * g.C;
      Pack<V> xv[ND];
#pragma unroll
      for (int d = 0; d < ND; ++d) {
        const int wi = wi0 + d;
        xv[d] = ld<V>(row + (size_t)min(max(wi, 0), g.W - 1) * g.C);   // in bounds, this clip; dropped when padding
        if (!(hok && (unsigned)wi < (unsigned)g.W)) xv[d] = zero<V>();
      }
#pragma unroll
      for (int kw = 0; kw < KW_; ++kw)
#pragma unroll
        for (int j = 0; j < TW; ++j)
#pragma unroll
          for (int i = 0; i < V; ++i)
            acc[j].v[i] = fmaf(wr[i * KK + kh * KW_ + kw], xv[j * SW_ + kw].v[i], acc[j].v[i]);
    }
  } else {
    const int KK = g.KH * g.KW;
    const int wi0 = wq * g.sw - g.pw;
    for (int kh = 0; kh < g.KH; ++kh) {
      const int hi = hi0 + kh;
      if ((unsigned)hi >= (unsigned)g.H) continue;
      for (int kw = 0; kw < g.KW; ++kw) {
        const int wi = wi0 + kw;
        if ((unsigned)wi >= (unsigned)g.W) continue;
        const Pack<V> xv = ld<V>(xn + ((size_t)hi * g.W + wi) * g.C);
#pragma unroll
        for (int i = 0; i < V; ++i)
          acc[0].v[i] = fmaf(w[(size_t)(c0 + i) * KK + kh * g.KW + kw], xv.v[i], acc[0].v[i]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < TW; ++j) {
    const int wo = wq * TW + j;
    if (wo < g.Wo) st<V>(y + (((size_t)n * g.Ho + ho) * g.Wo + wo) * g.C + c0, acc[j]);
  }
}

// 3 x 3 data gradient, 4 consecutive dx columns of one row per thread: the transposed form of the forward's register
// tile.  Row kh reads dY row (hi + ph - kh) / sh (when that is a whole, existing row); along W, SW_ = 1 reads the 6
// columns wi0 + pw - 2 ... wi0 + pw + 3, SW_ = 2 (pw = 1 only: the parity of each (column, tap) pair is then known
// at compile time, wi0 being a multiple of 4) the 3 columns wi0 / 2 ... wi0 / 2 + 2.  Every load is issued
// unconditionally from a clamped address of the same clip and selected to 0 where the tap does not exist.
template <int V, int SW_>
__global__ __launch_bounds__(kBlock) void dwconv_dgrad3_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                               Geom g, int total, float* __restrict__ dx) {
  constexpr int TW = 4, KK = 9, ND = SW_ == 1 ? 6 : 3;
  int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int CG = g.C / V, WQ = (g.W + TW - 1) / TW;
  const int cg = idx % CG;
  idx /= CG;
  const int wq = idx % WQ;
  idx /= WQ;
  const int hi = idx % g.H, n = idx / g.H;
  const int c0 = cg * V, wi0 = wq * TW;
  const float* __restrict__ dyn = dy + (size_t)n * g.Ho * g.Wo * g.C + c0;
  float wr[V * KK];   // channel i, tap t at i KK + t
  if constexpr (V == 4) {
#pragma unroll
    for (int q = 0; q < KK; ++q) {
      const float4 t = *reinterpret_cast<const float4*>(w + (size_t)c0 * KK + 4 * q);
      wr[4 * q] = t.x, wr[4 * q + 1] = t.y, wr[4 * q + 2] = t.z, wr[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < KK; ++q) wr[q] = w[(size_t)c0 * KK + q];
  }
  const int mh = g.sh - 1;
  const int wo0 = SW_ == 1 ? wi0 + g.pw - 2 : wi0 / 2;   // dY column of xv[0]
  Pack<V> acc[TW];
#pragma unroll
  for (int j = 0; j < TW; ++j) acc[j] = zero<V>();
#pragma unroll
  for (int kh = 0; kh < 3; ++kh) {
    const int th = hi + g.ph - kh;
    const int ho = th >> mh;
    const bool hok = th >= 0 && !(th & mh) && ho < g.Ho;
    const float* __restrict__ row = dyn + (size_t)min(max(ho, 0), g.Ho - 1) * g.Wo * g.C;
    Pack<V> dv[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
      const int wo = wo0 + d;
      dv[d] = ld<V>(row + (size_t)min(max(wo, 0), g.Wo - 1) * g.C);
      if (!(hok && (unsigned)wo < (unsigned)g.Wo)) dv[d] = zero<V>();
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw)
#pragma unroll
      for (int j = 0; j < TW; ++j) {
        // SW_ = 1: wo = wi0 + j + pw - kw = wo0 + j + 2 - kw.  SW_ = 2, pw = 1: tw = wi0 + j + 1 - kw, even pairs only
        if (SW_ == 2 && ((j + 1 - kw) & 1)) continue;
        const int d = SW_ == 1 ? j + 2 - kw : (j + 1 - kw) / 2;
        if (d < 0 || d >= ND) continue;   // SW_ = 2: tw = -1 (j = 0, kw = 2) has no column
#pragma unroll
        for (int i = 0; i < V; ++i) acc[j].v[i] = fmaf(wr[i * KK + kh * 3 + kw], dv[d].v[i], acc[j].v[i]);
      }
  }
#pragma unroll
  for (int j = 0; j < TW; ++j) {
    const int wi = wi0 + j;
    if (wi < g.W) st<V>(dx + (((size_t)n * g.H + hi) * g.W + wi) * g.C + c0, acc[j]);
  }
}

// K_ = 3: 3 x 3 unrolled; K_ = 0: any kernel size.
template <int V, int K_>
__global__ __launch_bounds__(kBlock) void dwconv_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                              Geom g, int total, float* __restrict__ dx) {
  int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int KH = K_ ? K_ : g.KH, KW = K_ ? K_ : g.KW, KK = KH * KW;
  const int CG = g.C / V;
  const int cg = idx % CG;
  idx /= CG;
  const int wi = idx % g.W;
  idx /= g.W;
  const int hi = idx % g.H, n = idx / g.H;
  const int c0 = cg * V;
  const float* __restrict__ dyn = dy + (size_t)n * g.Ho * g.Wo * g.C + c0;
  const float* __restrict__ wc = w + (size_t)c0 * KK;
  const int mh = g.sh - 1, mw = g.sw - 1;   // stride 1 or 2: parity mask and shift
  Pack<V> acc = zero<V>();
#pragma unroll
  for (int kh = 0; kh < KH; ++kh) {
    const int th = hi + g.ph - kh;
    const int ho = th >> mh;
    if (th < 0 || (th & mh) || ho >= g.Ho) continue;
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) {
      const int tw = wi + g.pw - kw;
      const int wo = tw >> mw;
      if (tw < 0 || (tw & mw) || wo >= g.Wo) continue;
      const Pack<V> d = ld<V>(dyn + ((size_t)ho * g.Wo + wo) * g.C);
#pragma unroll
      for (int i = 0; i < V; ++i) acc.v[i] = fmaf(wc[i * KK + kh * KW + kw], d.v[i], acc.v[i]);
    }
  }
  st<V>(dx + (((size_t)n * g.H + hi) * g.W + wi) * g.C + c0, acc);
}

// Grid (chunks, tap groups, channel tiles).  ws [chunks][KH KW + 1][C]; entry KH KW of a slab is db's.
template <int V>
__global__ __launch_bounds__(kBlock) void dwconv_wgrad_kernel(const float* __restrict__ x,
                                                              const float* __restrict__ dy, Geom g, int cols,
                                                              int chunk, int P, float* __restrict__ ws) {
  __shared__ float red[kBlock * V];
  const int rows = kBlock / cols;   // cols is a power of two <= 64
  const int col = threadIdx.x & (cols - 1), row = threadIdx.x / cols;
  const int CG = g.C / V, KK = g.KH * g.KW;
  const int cg = blockIdx.z * cols + col;
  const bool live = cg < CG;
  const int c0 = cg * V;
  const int t0 = blockIdx.y * kTapGroup;
  int khs[kTapGroup], kws[kTapGroup];
#pragma unroll
  for (int i = 0; i < kTapGroup; ++i) khs[i] = (t0 + i) / g.KW, kws[i] = (t0 + i) % g.KW;
  Pack<V> acc[kTapGroup], accb = zero<V>();
#pragma unroll
  for (int i = 0; i < kTapGroup; ++i) acc[i] = zero<V>();
  if (live) {
    const int pbeg = blockIdx.x * chunk, pend = min(P, pbeg + chunk);
    // One pixel's dY and its taps of x.  No branch in here: every load is issued unconditionally from a clamped
    // address (a valid pixel, a position inside the same clip) and selected to 0 where the pixel is past the chunk or
    // the tap is padding or past KH KW, so the loads of the two pixels of an iteration go out together.
    auto pixel = [&](int p, bool on) {
      const int wo = p % g.Wo, q = p / g.Wo;
      const int ho = q % g.Ho, n = q / g.Ho;
      Pack<V> d = ld<V>(dy + (size_t)p * g.C + c0);
      if (!on) d = zero<V>();
#pragma unroll
      for (int i = 0; i < V; ++i) accb.v[i] += d.v[i];
      const float* __restrict__ xn = x + (size_t)n * g.H * g.W * g.C + c0;
      const int hi0 = ho * g.sh - g.ph, wi0 = wo * g.sw - g.pw;
#pragma unroll
      for (int t = 0; t < kTapGroup; ++t) {
        const int hi = hi0 + khs[t], wi = wi0 + kws[t];
        Pack<V> xv = ld<V>(xn + ((size_t)min(max(hi, 0), g.H - 1) * g.W + min(max(wi, 0), g.W - 1)) * g.C);
        if (!(on && t0 + t < KK && (unsigned)hi < (unsigned)g.H && (unsigned)wi < (unsigned)g.W)) xv = zero<V>();
#pragma unroll
        for (int i = 0; i < V; ++i) acc[t].v[i] = fmaf(d.v[i], xv.v[i], acc[t].v[i]);
      }
    };
    for (int p = pbeg + row; p < pend; p += 2 * rows) {
      const bool on2 = p + rows < pend;
      pixel(p, true);
      pixel(on2 ? p + rows : p, on2);
    }
  }
  // the rows summed through LDS in row order, one quantity at a time: red[row][col][V]
  auto reduce = [&](const Pack<V>& a, int t, bool wanted) {
#pragma unroll
    for (int i = 0; i < V; ++i) red[threadIdx.x * V + i] = a.v[i];
    __syncthreads();
    if (row == 0 && live && wanted) {
      Pack<V> sum = zero<V>();
      for (int r = 0; r < rows; ++r)
#pragma unroll
        for (int i = 0; i < V; ++i) sum.v[i] += red[(r * cols + col) * V + i];
      st<V>(ws + ((size_t)blockIdx.x * (KK + 1) + t) * g.C + c0, sum);
    }
    __syncthreads();
  };
#pragma unroll
  for (int k = 0; k < kTapGroup; ++k) reduce(acc[k], t0 + k, t0 + k < KK);
  reduce(accb, KK, blockIdx.y == 0);   // entry KH KW of the slab: db, from the first tap group
}

// Entry e = t C + c of every slab summed over the nb slabs; dw[c][t] written or added to, db[c] written.
__global__ __launch_bounds__(kRedCols* kRedGroups) void dwconv_wgrad_reduce_kernel(const float* __restrict__ ws, int nb,
                                                                                   int KK, int C, int accumulate,
                                                                                   float* __restrict__ dw,
                                                                                   float* __restrict__ db) {
  __shared__ float part[kRedGroups][kRedCols];
  const int lane = threadIdx.x & (kRedCols - 1), grp = threadIdx.x / kRedCols;
  const int E = (KK + 1) * C;
  const int e = blockIdx.x * kRedCols + lane;
  float acc = 0.f;
  if (e < E) {
#pragma unroll 4
    for (int b = grp; b < nb; b += kRedGroups) acc += ws[(size_t)b * E + e];
  }
  part[grp][lane] = acc;
  __syncthreads();
  if (grp == 0 && e < E) {
    float sum = part[0][lane];
#pragma unroll
    for (int q = 1; q < kRedGroups; ++q) sum += part[q][lane];
    const int t = e / C, c = e - t * C;
    if (t < KK) {
      float* out = dw + (size_t)c * KK + t;
      *out = accumulate ? *out + sum : sum;
    } else if (db) {
      db[c] = sum;
    }
  }
}

// Grid (N, channel tiles).
template <int V>
__global__ __launch_bounds__(kBlock) void avgpool_fwd_kernel(const float* __restrict__ x, int HW, int C, int cols,
                                                             float* __restrict__ y) {
  __shared__ float red[kBlock * V];
  const int rows = kBlock / cols;
  const int col = threadIdx.x & (cols - 1), row = threadIdx.x / cols;
  const int CG = C / V;
  const int cg = blockIdx.y * cols + col, n = blockIdx.x;
  const bool live = cg < CG;
  Pack<V> acc = zero<V>();
  if (live) {
    const float* __restrict__ xn = x + (size_t)n * HW * C + cg * V;
#pragma unroll 4
    for (int p = row; p < HW; p += rows) {
      const Pack<V> v = ld<V>(xn + (size_t)p * C);
#pragma unroll
      for (int i = 0; i < V; ++i) acc.v[i] += v.v[i];
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) red[threadIdx.x * V + i] = acc.v[i];
  __syncthreads();
  if (row == 0 && live) {
    Pack<V> sum = zero<V>();
    for (int r = 0; r < rows; ++r)
#pragma unroll
      for (int i = 0; i < V; ++i) sum.v[i] += red[(r * cols + col) * V + i];
#pragma unroll
    for (int i = 0; i < V; ++i) sum.v[i] /= (float)HW;
    st<V>(y + (size_t)n * C + cg * V, sum);
  }
}

template <int V>
__global__ __launch_bounds__(kBlock) void avgpool_bwd_kernel(const float* __restrict__ dy, int HW, int C, int total,
                                                             float* __restrict__ dx) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int CG = C / V;
  const int cg = idx % CG, n = idx / CG / HW;
  Pack<V> v = ld<V>(dy + (size_t)n * C + cg * V);
#pragma unroll
  for (int i = 0; i < V; ++i) v.v[i] /= (float)HW;
  st<V>(dx + (size_t)idx * V, v);
}

// a b c d < 2^31 without overflowing (every factor >= 1)
bool below_2_31(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t lim = (int64_t(1) << 31) - 1;
  const int64_t rest[3] = {b, c, d};
  int64_t p = a;
  for (int64_t f : rest) {
    if (p > lim / f) return false;
    p *= f;
  }
  return true;
}

int check_dw(const char* fn, int64_t N, int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW, int64_t ph,
             int64_t pw, int64_t sh, int64_t sw, Geom* g) {
  SRK_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 1, SRK_ERR_INVALID, "%s: needs N, H, W, C >= 1, got %lld %lld %lld %lld",
              fn, (long long)N, (long long)H, (long long)W, (long long)C);
  SRK_REQUIRE(KH >= 1 && KH <= kMaxK && KW >= 1 && KW <= kMaxK, SRK_ERR_INVALID,
              "%s: needs 1 <= KH, KW <= 7, got %lld x %lld", fn, (long long)KH, (long long)KW);
  SRK_REQUIRE((sh == 1 || sh == 2) && (sw == 1 || sw == 2), SRK_ERR_INVALID, "%s: strides must be 1 or 2, got %lld, %lld",
              fn, (long long)sh, (long long)sw);
  SRK_REQUIRE(ph >= 0 && ph < KH && pw >= 0 && pw < KW, SRK_ERR_INVALID,
              "%s: needs 0 <= ph < KH and 0 <= pw < KW, got padding %lld, %lld", fn, (long long)ph, (long long)pw);
  SRK_REQUIRE(H + 2 * ph >= KH && W + 2 * pw >= KW, SRK_ERR_INVALID,
              "%s: the padded input %lld x %lld is smaller than the kernel %lld x %lld", fn, (long long)(H + 2 * ph),
              (long long)(W + 2 * pw), (long long)KH, (long long)KW);
  const int64_t Ho = (H + 2 * ph - KH) / sh + 1, Wo = (W + 2 * pw - KW) / sw + 1;
  SRK_REQUIRE(below_2_31(N, H, W, C) && below_2_31(N, Ho, Wo, C) && below_2_31(C, KH, KW, 1), SRK_ERR_INVALID,
              "%s: every tensor must stay below 2^31 elements, got N %lld H %lld W %lld C %lld", fn, (long long)N,
              (long long)H, (long long)W, (long long)C);
  *g = Geom{(int)N, (int)H, (int)W, (int)C, (int)KH, (int)KW, (int)ph, (int)pw, (int)sh, (int)sw, (int)Ho, (int)Wo};
  return SRK_OK;
}

int check_pool(const char* fn, int64_t N, int64_t HW, int64_t C) {
  SRK_REQUIRE(N >= 1 && HW >= 1 && C >= 1, SRK_ERR_INVALID, "%s: needs N, HW, C >= 1, got %lld %lld %lld", fn,
              (long long)N, (long long)HW, (long long)C);
  SRK_REQUIRE(below_2_31(N, HW, C, 1), SRK_ERR_INVALID, "%s: N HW C must stay below 2^31, got %lld %lld %lld", fn,
              (long long)N, (long long)HW, (long long)C);
  return SRK_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// channel groups per workgroup of the reducing kernels: the power of two >= min(groups, 64)
int cols_for(int groups) {
  int cols = 1;
  while (cols < groups && cols < kMaxCols) cols *= 2;
  return cols;
}

// weight-gradient workgroups along the pixels; the same for the vector and the scalar path (sized by the scalar
// one's rows, the larger count)
int slabs_for(const Geom& g) {
  const int64_t P = (int64_t)g.N * g.Ho * g.Wo;
  const int rows = kBlock / cols_for(g.C);
  const int64_t nb = (P + rows - 1) / rows;
  return (int)(nb < kMaxSlabs ? nb : kMaxSlabs);
}

}  // namespace
}  // namespace srk

extern "C" {

int64_t srk_dwconv2d_workspace_floats(int64_t N, int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW, int64_t ph,
                                      int64_t pw, int64_t sh, int64_t sw) {
  srk::Geom g;
  if (srk::check_dw("dwconv_workspace", N, H, W, C, KH, KW, ph, pw, sh, sw, &g)) return 0;
  return (int64_t)srk::slabs_for(g) * (KH * KW + 1) * C;
}

int srk_dwconv2d_nhwc_fwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, const float* w,
                          const float* bias, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw,
                          float* y, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  Geom g;
  if (int rc = check_dw("dwconv_fwd", N, H, W, C, KH, KW, ph, pw, sh, sw, &g)) return rc;
  SRK_REQUIRE(x && w && y, SRK_ERR_INVALID, "dwconv_fwd: null pointer");
  hipStream_t s = as_stream(stream);
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias);
  const bool k3 = KH == 3 && KW == 3;
  const int V = vec ? 4 : 1, TW = k3 ? 4 : 1;
  const int total = g.N * g.Ho * ((g.Wo + TW - 1) / TW) * (g.C / V);
  const double bytes = 4.0 * ((double)N * H * W * C + (double)N * g.Ho * g.Wo * C + (double)C * KH * KW + (bias ? C : 0));
  ProfScope prof("dwconv_fwd", s, bytes);
  prof.bytes(bytes);
  prof.detail("dwconv_fwd_kernel<%d,%s> %dx%dx%dx%d k%dx%d s%d,%d", V, k3 ? "3x3" : "any", g.N, g.H, g.W, g.C, g.KH,
              g.KW, g.sh, g.sw);
  const dim3 grid((unsigned)((total + kBlock - 1) / kBlock)), block(kBlock);
#define SRK_DW_FWD(V_, KH_, KW_, SW_) \
  hipLaunchKernelGGL((dwconv_fwd_kernel<V_, KH_, KW_, SW_>), grid, block, 0, s, x, w, bias, g, total, y)
  if (k3 && sw == 1) {
    if (vec) SRK_DW_FWD(4, 3, 3, 1);
    else SRK_DW_FWD(1, 3, 3, 1);
  } else if (k3) {
    if (vec) SRK_DW_FWD(4, 3, 3, 2);
    else SRK_DW_FWD(1, 3, 3, 2);
  } else {
    if (vec) SRK_DW_FWD(4, 0, 0, 0);
    else SRK_DW_FWD(1, 0, 0, 0);
  }
#undef SRK_DW_FWD
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_dwconv2d_nhwc_bwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, const float* w, int64_t KH,
                          int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw, const float* dy, float* dx,
                          float* dw, float* db, float* ws, int dw_accumulate, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  Geom g;
  if (int rc = check_dw("dwconv_bwd", N, H, W, C, KH, KW, ph, pw, sh, sw, &g)) return rc;
  SRK_REQUIRE(x && w && dy && dw && ws, SRK_ERR_INVALID, "dwconv_bwd: null pointer");
  hipStream_t s = as_stream(stream);
  const bool k3 = KH == 3 && KW == 3;
  const int KK = g.KH * g.KW;
  const double nx = (double)N * H * W * C, ny = (double)N * g.Ho * g.Wo * C;
  if (dx) {
    const bool vec = C % 4 == 0 && aligned16(dy) && aligned16(dx) && aligned16(w);
    const int V = vec ? 4 : 1;
    const bool tile = k3 && (sw == 1 || pw == 1);   // the register-tile kernel: 4 dx columns per thread
    const int total = g.N * g.H * (tile ? (g.W + 3) / 4 : g.W) * (g.C / V);
    const double bytes = 4.0 * (nx + ny + (double)C * KK);
    ProfScope prof("dwconv_dgrad", s, bytes);
    prof.bytes(bytes);
    prof.detail("dwconv_dgrad%s_kernel<%d,%s> %dx%dx%dx%d k%dx%d s%d,%d", tile ? "3" : "", V, k3 ? "3x3" : "any", g.N,
                g.H, g.W, g.C, g.KH, g.KW, g.sh, g.sw);
    const dim3 grid((unsigned)((total + kBlock - 1) / kBlock)), block(kBlock);
#define SRK_DW_DGRAD(V_, K_) hipLaunchKernelGGL((dwconv_dgrad_kernel<V_, K_>), grid, block, 0, s, dy, w, g, total, dx)
#define SRK_DW_DGRAD3(V_, SW_) \
  hipLaunchKernelGGL((dwconv_dgrad3_kernel<V_, SW_>), grid, block, 0, s, dy, w, g, total, dx)
    if (tile && sw == 1) {
      if (vec) SRK_DW_DGRAD3(4, 1);
      else SRK_DW_DGRAD3(1, 1);
    } else if (tile) {
      if (vec) SRK_DW_DGRAD3(4, 2);
      else SRK_DW_DGRAD3(1, 2);
    } else if (k3) {
      if (vec) SRK_DW_DGRAD(4, 3);
      else SRK_DW_DGRAD(1, 3);
    } else {
      if (vec) SRK_DW_DGRAD(4, 0);
      else SRK_DW_DGRAD(1, 0);
    }
#undef SRK_DW_DGRAD
#undef SRK_DW_DGRAD3
    SRK_CHECK_HIP(hipGetLastError());
  }
  const int nb = slabs_for(g);
  const int P = g.N * g.Ho * g.Wo;
  const int chunk = (P + nb - 1) / nb;
  const double slab_bytes = 4.0 * (double)nb * (KK + 1) * C;
  {
    const bool vec = C % 4 == 0 && aligned16(x) && aligned16(dy) && aligned16(ws);
    const int V = vec ? 4 : 1;
    const int groups = g.C / V, cols = cols_for(groups);
    const int tap_groups = (KK + kTapGroup - 1) / kTapGroup;
    const double bytes = 4.0 * (nx + ny) + slab_bytes;
    ProfScope prof("dwconv_wgrad", s, bytes);
    prof.bytes(bytes);
    prof.detail("dwconv_wgrad_kernel<%d> %dx%dx%dx%d k%dx%d s%d,%d", V, g.N, g.H, g.W, g.C, g.KH, g.KW, g.sh, g.sw);
    const dim3 grid((unsigned)nb, (unsigned)tap_groups, (unsigned)((groups + cols - 1) / cols)), block(kBlock);
    if (vec) hipLaunchKernelGGL(dwconv_wgrad_kernel<4>, grid, block, 0, s, x, dy, g, cols, chunk, P, ws);
    else hipLaunchKernelGGL(dwconv_wgrad_kernel<1>, grid, block, 0, s, x, dy, g, cols, chunk, P, ws);
    SRK_CHECK_HIP(hipGetLastError());
  }
  {
    const int E = (KK + 1) * g.C;
    const double bytes = slab_bytes + 4.0 * (double)C * KK * (dw_accumulate ? 2 : 1) + (db ? 4.0 * C : 0.0);
    ProfScope prof("dwconv_wgrad", s, bytes);
    prof.bytes(bytes);
    prof.detail("dwconv_wgrad_reduce_kernel<%s> %dx%dx%d", dw_accumulate ? "acc" : "set", nb, KK + 1, g.C);
    const dim3 grid((unsigned)((E + kRedCols - 1) / kRedCols)), block(kRedCols * kRedGroups);
    hipLaunchKernelGGL(dwconv_wgrad_reduce_kernel, grid, block, 0, s, ws, nb, KK, g.C, dw_accumulate ? 1 : 0, dw, db);
    SRK_CHECK_HIP(hipGetLastError());
  }
  return SRK_OK;
  SRK_API_END
}

int srk_avgpool_nhwc_fwd(const float* x, int64_t N, int64_t HW, int64_t C, float* y, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  if (int rc = check_pool("avgpool_fwd", N, HW, C)) return rc;
  SRK_REQUIRE(x && y, SRK_ERR_INVALID, "avgpool_fwd: null pointer");
  hipStream_t s = as_stream(stream);
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(y);
  const int V = vec ? 4 : 1;
  const int groups = (int)C / V, cols = cols_for(groups);
  const double bytes = 4.0 * ((double)N * HW * C + (double)N * C);
  ProfScope prof("avgpool", s, bytes);
  prof.bytes(bytes);
  prof.detail("avgpool_fwd_kernel<%d> %lldx%lldx%lld", V, (long long)N, (long long)HW, (long long)C);
  const dim3 grid((unsigned)N, (unsigned)((groups + cols - 1) / cols)), block(kBlock);
  if (vec) hipLaunchKernelGGL(avgpool_fwd_kernel<4>, grid, block, 0, s, x, (int)HW, (int)C, cols, y);
  else hipLaunchKernelGGL(avgpool_fwd_kernel<1>, grid, block, 0, s, x, (int)HW, (int)C, cols, y);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_avgpool_nhwc_bwd(const float* dy, int64_t N, int64_t HW, int64_t C, float* dx, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  if (int rc = check_pool("avgpool_bwd", N, HW, C)) return rc;
  SRK_REQUIRE(dy && dx, SRK_ERR_INVALID, "avgpool_bwd: null pointer");
  hipStream_t s = as_stream(stream);
  const bool vec = C % 4 == 0 && aligned16(dy) && aligned16(dx);
  const int V = vec ? 4 : 1;
  const int total = (int)(N * HW * (C / V));
  const double bytes = 4.0 * ((double)N * HW * C + (double)N * C);
  ProfScope prof("avgpool", s, bytes);
  prof.bytes(bytes);
  prof.detail("avgpool_bwd_kernel<%d> %lldx%lldx%lld", V, (long long)N, (long long)HW, (long long)C);
  const dim3 grid((unsigned)((total + kBlock - 1) / kBlock)), block(kBlock);
  if (vec) hipLaunchKernelGGL(avgpool_bwd_kernel<4>, grid, block, 0, s, dy, (int)HW, (int)C, total, dx);
  else hipLaunchKernelGGL(avgpool_bwd_kernel<1>, grid, block, 0, s, dy, (int)HW, (int)C, total, dx);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
