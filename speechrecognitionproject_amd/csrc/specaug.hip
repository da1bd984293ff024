// SpecAugment on a batch of feature clips (include/srk.h srk_specaug_apply / srk_specaug_draw; features.spec_augment):
// a time warp that moves frame c to frame w, up to 4 frequency masks and up to 4 time masks per clip, every random
// quantity an explicit int32 parameter that lives on the device.
//
// One workgroup owns one clip and stages it whole in LDS, always as the logical [T][S] image (S = the row stride,
// F or F | 1) whatever the layout in memory.  That buys four things at once:
//  * one HBM read and one HBM write per element — the warp reads frames i and i + 1 out of LDS;
//  * in-place operation (y == x) is safe: every read of the clip precedes the barrier, every write follows it;
//  * both layouts are read and written along their contiguous axis; the [F][T] layout is transposed on its way into
//    LDS and back, so the arithmetic — the mean's summation order included — is the same instruction stream on the
//    same image, and the two layouts' results are each other's transposes bit for bit;
//  * the mean fill is one extra pass over LDS, in the fixed order of the logical index t F + f.
// With the [F][T] layout, consecutive lanes write (and later read) LDS S words apart, so S is made odd where the
// padded image still fits; with [T][F] the image is the memory order and S = F.
//
// Per frame the warp needs two integer divisions (i = floor(s), a = frac(s)) and the time-mask test.  They are done
// once per frame into an LDS table {i or -1 when masked, a} where 2 T more words fit beside the clip (every feature
// shape of the project: T <= 98), and per element by the same function otherwise (long, narrow clips).
//
// The parameters are validated before anything is read through them; an invalid row turns its clip into NaN and the
// workgroup returns (K2-VTLP's convention, csrc/features.hip).
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kThreads = 512;             // 8 waves per clip
constexpr int kWaves = kThreads / 64;
constexpr int kMaxMasks = 4;              // NF, NT <= 4 (include/srk.h)
constexpr int kLdsWords = 16384;          // 64 KB per workgroup: two clips of any shape per CU, three filter banks
constexpr int kScratchWords = 16;         // the waves' partial sums of the mean
constexpr int kDrawThreads = 256;
static_assert(SRK_SPECAUG_MAX_ELEMS + kScratchWords <= kLdsWords, "the staged clip must fit the workgroup's LDS");
static_assert(kWaves <= kScratchWords, "one partial sum per wave");

// One clip's parameters as half-open ranges; slots past NF / NT are empty.
struct ClipParams {
  int c, w;
  int f_lo[kMaxMasks], f_hi[kMaxMasks], t_lo[kMaxMasks], t_hi[kMaxMasks];
};

// Reads and validates row `row` (P = 2 + 2 NF + 2 NT words).  Nothing but the row itself is read here.
__device__ __forceinline__ bool load_params(const int32_t* __restrict__ row, int NF, int NT, int T, int F,
                                            ClipParams& p) {
  p.c = row[0];
  p.w = row[1];
  bool ok = (p.c == p.w) ? (p.c >= 0 && p.c <= T - 1) : (p.c >= 1 && p.c <= T - 2 && p.w >= 1 && p.w <= T - 2);
#pragma unroll
  for (int j = 0; j < kMaxMasks; ++j) {
    p.f_lo[j] = p.f_hi[j] = p.t_lo[j] = p.t_hi[j] = 0;
    if (j < NF) {
      const int f0 = row[2 + 2 * j], fw = row[3 + 2 * j];
      const bool good = f0 >= 0 && fw >= 0 && f0 <= F && fw <= F - f0;   // no f0 + fw: it may overflow
      ok = ok && good;
      if (good) p.f_lo[j] = f0, p.f_hi[j] = f0 + fw;
    }
    if (j < NT) {
      const int t0 = row[2 + 2 * NF + 2 * j], tw = row[3 + 2 * NF + 2 * j];
      const bool good = t0 >= 0 && tw >= 0 && t0 <= T && tw <= T - t0;
      ok = ok && good;
      if (good) p.t_lo[j] = t0, p.t_hi[j] = t0 + tw;
    }
  }
  return ok;
}

__device__ __forceinline__ bool in_ranges(int v, const int (&lo)[kMaxMasks], const int (&hi)[kMaxMasks]) {
  bool m = false;
#pragma unroll
  for (int j = 0; j < kMaxMasks; ++j) m = m || (v >= lo[j] && v < hi[j]);
  return m;
}

// What output frame t reads: source frame i (and i + 1 when a != 0), or i = -1 for a masked frame.
struct Frame {
  int i;
  float a;
};

__device__ __forceinline__ Frame frame_of(int t, int T, const ClipParams& p) {
  Frame fr;
  fr.a = 0.f;
  if (in_ranges(t, p.t_lo, p.t_hi)) {
    fr.i = -1;
    return fr;
  }
  fr.i = t;
  if (p.c == p.w) return fr;
  // valid parameters with c != w have 1 <= c, w <= T - 2: both denominators are >= 1 and every product is < T^2
  int num, den, base;
  if (t <= p.w) {
    num = t * p.c, den = p.w, base = 0;
  } else {
    num = (t - p.w) * (T - 1 - p.c), den = T - 1 - p.w, base = p.c;
  }
  const int q = num / den, r = num - q * den;
  fr.i = base + q;   // <= T - 1, and <= T - 2 whenever r != 0
  fr.a = __fdiv_rn((float)r, (float)den);
  return fr;
}

// Flat index g = outer * D + inner of a [.][D] array, stepped without further divisions.
struct Pos {
  int outer, inner;
};

__device__ __forceinline__ Pos pos_of(int g, int D) {
  Pos p;
  p.outer = g / D;
  p.inner = g - p.outer * D;
  return p;
}

// advance by n_outer * D + n_inner with n_inner < D
__device__ __forceinline__ void pos_step(Pos& p, int n_outer, int n_inner, int D) {
  p.outer += n_outer;
  p.inner += n_inner;
  if (p.inner >= D) p.inner -= D, ++p.outer;
}

struct Image {
  const float* clip;   // LDS [T][S]
  const int* fi;       // LDS frame table (use_table)
  const float* fa;
  int T, S;
  bool use_table;
  float fill;
};

__device__ __forceinline__ float element(const Image& im, const ClipParams& p, int t, int f) {
  Frame fr;
  if (im.use_table) {
    fr.i = im.fi[t], fr.a = im.fa[t];
  } else {
    fr = frame_of(t, im.T, p);
  }
  if (fr.i < 0 || in_ranges(f, p.f_lo, p.f_hi)) return im.fill;
  const float x0 = im.clip[fr.i * im.S + f];
  if (fr.a == 0.f) return x0;   // a bit-exact copy; frame i + 1 (which may not exist) is not read
  const float x1 = im.clip[(fr.i + 1) * im.S + f];
  return __fadd_rn(x0, __fmul_rn(fr.a, __fsub_rn(x1, x0)));
}

// VEC: 16-byte global accesses (T F % 4 == 0, x and y 16-byte aligned).  x and y may be the same tensor.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void specaug_apply_kernel(const float* x, int T, int F, int S, int time_major,
                                                                 int use_table, const int32_t* __restrict__ params,
                                                                 int NF, int NT, int fill_mode, float fill_value,
                                                                 float* y) {
  extern __shared__ float4 lds4[];
  float* clip = reinterpret_cast<float*>(lds4);
  const int n = T * F, tid = threadIdx.x;
  const size_t b = blockIdx.x;
  const float* xb = x + b * (size_t)n;
  float* yb = y + b * (size_t)n;
  constexpr int kStep = VEC ? 4 : 1;                 // elements per thread and iteration
  const int groups = n / kStep;

  ClipParams p;
  if (!load_params(params + b * (size_t)(2 + 2 * NF + 2 * NT), NF, NT, T, F, p)) {   // uniform over the workgroup
    const float nan = __int_as_float(0x7fc00000);
    for (int g = tid; g < groups; g += kThreads) {
      if (VEC) reinterpret_cast<float4*>(yb)[g] = make_float4(nan, nan, nan, nan);
      else yb[g] = nan;
    }
    return;
  }

  // ---- stage the clip: memory order in, logical [T][S] image out
  const int D = time_major ? F : T;                  // the contiguous axis' length
  const int so = (kThreads * kStep) / D, si = (kThreads * kStep) - so * D;   // one iteration's stride as a Pos step
  if (time_major) {                                  // S == F: the image is the memory order
#pragma unroll 4                                     // a 98 x 120 clip is 6 loads per thread: keep them in flight
    for (int g = tid; g < groups; g += kThreads) {
      if (VEC) lds4[g] = reinterpret_cast<const float4*>(xb)[g];
      else clip[g] = xb[g];
    }
  } else {
    Pos at = pos_of(tid * kStep, D);                 // outer = f, inner = t
    for (int g = tid; g < groups; g += kThreads) {
      if (VEC) {
        const float4 v = reinterpret_cast<const float4*>(xb)[g];
        const float e[4] = {v.x, v.y, v.z, v.w};
        Pos q = at;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          clip[q.inner * S + q.outer] = e[j];
          pos_step(q, 0, 1, D);
        }
      } else {
        clip[at.inner * S + at.outer] = xb[g];
      }
      pos_step(at, so, si, D);
    }
  }
  __syncthreads();

  // ---- the frame table and the mean, both off the staged image
  float* scratch = clip + T * S;
  int* fi = reinterpret_cast<int*>(scratch + kScratchWords);
  float* fa = reinterpret_cast<float*>(fi + T);
  if (use_table) {
    for (int t = tid; t < T; t += kThreads) {
      const Frame fr = frame_of(t, T, p);
      fi[t] = fr.i;
      fa[t] = fr.a;
    }
  }
  if (fill_mode == 1) {
    // thread k adds the logical elements k, k + 512, ... in order; a butterfly over the wave; the 8 waves in order
    float acc = 0.f;
    if (S == F) {
      for (int e = tid; e < n; e += kThreads) acc += clip[e];
    } else {
      Pos at = pos_of(tid, F);
      const int mo = kThreads / F, mi = kThreads - mo * F;
      for (int e = tid; e < n; e += kThreads) {
        acc += clip[at.outer * S + at.inner];
        pos_step(at, mo, mi, F);
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if ((tid & 63) == 0) scratch[tid >> 6] = acc;
  }
  __syncthreads();

  Image im;
  im.clip = clip, im.fi = fi, im.fa = fa, im.T = T, im.S = S, im.use_table = use_table != 0;
  im.fill = fill_value;
  if (fill_mode == 1) {
    float sum = scratch[0];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) sum += scratch[wv];
    im.fill = __fdiv_rn(sum, (float)n);
  }

  // ---- write the clip in memory order
  Pos at = pos_of(tid * kStep, D);                   // time_major: (t, f), else (f, t)
  for (int g = tid; g < groups; g += kThreads) {
    if (VEC) {
      float e[4];
      Pos q = at;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        e[j] = time_major ? element(im, p, q.outer, q.inner) : element(im, p, q.inner, q.outer);
        pos_step(q, 0, 1, D);
      }
      reinterpret_cast<float4*>(yb)[g] = make_float4(e[0], e[1], e[2], e[3]);
    } else {
      yb[g] = time_major ? element(im, p, at.outer, at.inner) : element(im, p, at.inner, at.outer);
    }
    pos_step(at, so, si, D);
  }
}

// r_i(n) of include/srk.h: the high 32 bits of the hash scaled into [0, n)
__device__ __forceinline__ int draw_below(uint64_t seed, uint64_t i, int n) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (int)(((z >> 32) * (uint64_t)n) >> 32);
}

// One workgroup for the whole batch (a clip's P <= 18 draws are a few hundred integer instructions), so the counter
// can advance in the same launch: every thread has read the state before the barrier, thread 0 writes it after.
__global__ __launch_bounds__(kDrawThreads) void specaug_draw_kernel(uint64_t* state, int B, int T, int F, int W, int NF,
                                                                    int f_max, int NT, int t_max, int32_t* out) {
  const uint64_t seed = state[0] + 0xD1B54A32D192ED03ull * state[1];
  const int P = 2 + 2 * NF + 2 * NT;
  for (int b = threadIdx.x; b < B; b += kDrawThreads) {
    const uint64_t i0 = (uint64_t)b * P;
    int32_t* o = out + (size_t)b * P;
    int c = 0, w = 0;
    if (W > 0) {
      c = W + 1 + draw_below(seed, i0, T - 2 * W - 2);
      w = c - W + draw_below(seed, i0 + 1, 2 * W + 1);
    }
    o[0] = c;
    o[1] = w;
    for (int j = 0; j < NF; ++j) {
      const int fw = draw_below(seed, i0 + 2 + 2 * j, f_max + 1);
      o[2 + 2 * j] = draw_below(seed, i0 + 3 + 2 * j, F - fw + 1);
      o[3 + 2 * j] = fw;
    }
    for (int j = 0; j < NT; ++j) {
      const int tw = draw_below(seed, i0 + 2 + 2 * NF + 2 * j, t_max + 1);
      o[2 + 2 * NF + 2 * j] = draw_below(seed, i0 + 3 + 2 * NF + 2 * j, T - tw + 1);
      o[3 + 2 * NF + 2 * j] = tw;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) state[1] += 1;
}

int check_shape(const char* fn, int64_t B, int64_t T, int64_t F, int NF, int NT) {
  SRK_REQUIRE(B >= 1 && B < (int64_t(1) << 31) && T >= 1 && F >= 1 && T <= (int64_t(1) << 30) &&
                  F <= (int64_t(1) << 30),
              SRK_ERR_INVALID, "%s: needs B, T, F >= 1 (B < 2^31; T, F <= 2^30), got B %lld T %lld F %lld", fn,
              (long long)B, (long long)T, (long long)F);
  SRK_REQUIRE(NF >= 0 && NF <= kMaxMasks && NT >= 0 && NT <= kMaxMasks, SRK_ERR_INVALID,
              "%s: needs 0 <= NF, NT <= 4, got NF %d NT %d", fn, NF, NT);
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_specaug_apply(const float* x, int64_t B, int64_t T, int64_t F, int time_major, const int32_t* params, int NF,
                      int NT, int fill_mode, float fill_value, float* y, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  if (int rc = check_shape("specaug_apply", B, T, F, NF, NT)) return rc;
  SRK_REQUIRE(T * F <= SRK_SPECAUG_MAX_ELEMS, SRK_ERR_INVALID,
              "specaug_apply: a clip of %lld x %lld elements is above SRK_SPECAUG_MAX_ELEMS (%d)", (long long)T,
              (long long)F, SRK_SPECAUG_MAX_ELEMS);
  SRK_REQUIRE(time_major == 0 || time_major == 1, SRK_ERR_INVALID, "specaug_apply: time_major must be 0 or 1, got %d",
              time_major);
  SRK_REQUIRE(fill_mode == 0 || fill_mode == 1, SRK_ERR_INVALID,
              "specaug_apply: fill_mode must be 0 (value) or 1 (clip mean), got %d", fill_mode);
  SRK_REQUIRE(std::isfinite(fill_value), SRK_ERR_INVALID, "specaug_apply: fill_value is not finite");
  SRK_REQUIRE(x && params && y, SRK_ERR_INVALID, "specaug_apply: null pointer");
  hipStream_t s = as_stream(stream);
  const int n = (int)(T * F), P = 2 + 2 * NF + 2 * NT;
  // the row stride of the LDS image and whether the frame table fits beside it (see the head of this file)
  int S = (int)F;
  if (!time_major && (int)T * ((int)F | 1) + 2 * (int)T + kScratchWords <= kLdsWords) S = (int)F | 1;
  const int image = (int)T * S + kScratchWords;
  const int use_table = image + 2 * (int)T <= kLdsWords;
  const size_t lds_bytes = 4 * (size_t)(image + (use_table ? 2 * (int)T : 0));
  const bool vec = n % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  const double bytes = (double)B * (8.0 * n + 4.0 * P);
  ProfScope prof("specaug", s, bytes);
  prof.bytes(bytes);
  prof.detail("specaug_apply_kernel<%s,%s%s> %lldx%lldx%lld", vec ? "v4" : "s1", time_major ? "tf" : "ft",
              use_table ? "" : ",direct", (long long)B, (long long)T, (long long)F);
  const dim3 grid((unsigned)B), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(specaug_apply_kernel<true>, grid, block, lds_bytes, s, x, (int)T, (int)F, S, time_major,
                       use_table, params, NF, NT, fill_mode, fill_value, y);
  else
    hipLaunchKernelGGL(specaug_apply_kernel<false>, grid, block, lds_bytes, s, x, (int)T, (int)F, S, time_major,
                       use_table, params, NF, NT, fill_mode, fill_value, y);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_specaug_draw(uint64_t* state, int64_t B, int64_t T, int64_t F, int W, int NF, int f_max, int NT, int t_max,
                     int32_t* params_out, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  if (int rc = check_shape("specaug_draw", B, T, F, NF, NT)) return rc;
  SRK_REQUIRE(W >= 0 && (W == 0 || T >= 2 * (int64_t)W + 3), SRK_ERR_INVALID,
              "specaug_draw: needs W >= 0 and, with W > 0, T >= 2 W + 3, got W %d T %lld", W, (long long)T);
  SRK_REQUIRE(f_max >= 0 && f_max <= F, SRK_ERR_INVALID, "specaug_draw: f_max %d outside [0, F = %lld]", f_max,
              (long long)F);
  SRK_REQUIRE(t_max >= 0 && t_max <= T, SRK_ERR_INVALID, "specaug_draw: t_max %d outside [0, T = %lld]", t_max,
              (long long)T);
  SRK_REQUIRE(state && params_out, SRK_ERR_INVALID, "specaug_draw: null pointer");
  hipStream_t s = as_stream(stream);
  const double bytes = 4.0 * (double)B * (2 + 2 * NF + 2 * NT) + 32.0;
  ProfScope prof("specaug_draw", s, bytes);
  prof.bytes(bytes);
  prof.detail("specaug_draw_kernel %lld clips", (long long)B);
  hipLaunchKernelGGL(specaug_draw_kernel, dim3(1), dim3(kDrawThreads), 0, s, state, (int)B, (int)T, (int)F, W, NF, f_max,
                     NT, t_max, params_out);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
