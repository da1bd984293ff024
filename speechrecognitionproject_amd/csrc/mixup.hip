// Mixup on a batch of PCM clips (include/srk.h srk_mixup_draw / srk_mixup_apply; features.mixup_draw / mixup): clip b
// becomes lam_b x_b + (1 - lam_b) x_partner(b), the partner and the weight explicit device arrays.
//
// The apply is a stream: two reads and one write per element, nothing reused, so it is laid out for HBM alone.
//  * A workgroup of 256 threads owns one chunk of kChunk = 4096 consecutive elements of one row: a row of 16000
//    samples is 4 chunks, a batch of 256 rows 1024 workgroups (4 per CU); one row of 7 elements is one workgroup.
//  * Each thread moves kUnroll = 4 groups a whole workgroup apart, so every wave instruction reads 1 KiB (16-byte
//    path) of consecutive addresses, and all 8 loads are issued before the first store.
//  * partner[b] and lam[b] are the same for the whole workgroup: the validity test is uniform, and an invalid row's
//    workgroups store NaN without forming an address from the row's values (the SpecAugment convention).
// The arithmetic is fp32 under fp contract(off): four roundings, no fused multiply-add (the ISA has v_pk_mul_f32 and
// v_pk_add_f32 only), so numpy float32 restates it bit for bit.
//
// The draw is one workgroup for the whole batch (a clip's Beta draw is at most 64 double pow, B <= 2^24 and in
// practice a few hundred), so the counter advances in the same launch, as in csrc/specaug.hip.
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;
constexpr int kChunk = kThreads * kUnroll * 4;   // elements of one row per workgroup, either path
constexpr int kDrawThreads = 256;

// VEC: 16-byte accesses (n % 4 == 0, x and out 16-byte aligned: every row starts aligned).  G = elements per access.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void mixup_apply_kernel(const float* __restrict__ x, int B, int64_t n,
                                                               int chunks, const int32_t* __restrict__ partner,
                                                               const float* __restrict__ lam,
                                                               float* __restrict__ out) {
  // Plain operators under contract(off): the _rn intrinsics are inline functions compiled under the translation
  // unit's fp-contract=fast, and their product and sum were fused into v_pk_fma_f32 when used here.
#pragma clang fp contract(off)
  constexpr int G = VEC ? 4 : 1;
  constexpr int kIters = kChunk / (kThreads * G);          // 4 (16-byte path) or 16 (scalar path)
  const int b = (int)(blockIdx.x / (unsigned)chunks);      // < B: the grid is B * chunks
  const int chunk = (int)(blockIdx.x - (unsigned)b * (unsigned)chunks);
  const int64_t groups = n / G;                            // accesses per row
  const int64_t g0 = (int64_t)chunk * (kChunk / G) + threadIdx.x;
  float* ob = out + (size_t)b * (size_t)n;

  const int p = partner[b];
  const float l = lam[b];
  if (!(p >= 0 && p < B && l >= 0.f && l <= 1.f)) {        // NaN fails both comparisons
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t g = g0 + (int64_t)j * kThreads;
      if (g < groups) {
        if (VEC) reinterpret_cast<float4*>(ob)[g] = make_float4(nan, nan, nan, nan);
        else ob[g] = nan;
      }
    }
    return;
  }
  const float w = 1.0f - l;
  const float* xb = x + (size_t)b * (size_t)n;
  const float* xp = x + (size_t)p * (size_t)n;
  if (VEC) {
    float4 a[kIters], c[kIters];
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t g = g0 + (int64_t)j * kThreads;
      if (g < groups) {
        a[j] = reinterpret_cast<const float4*>(xb)[g];
        c[j] = reinterpret_cast<const float4*>(xp)[g];
      }
    }
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t g = g0 + (int64_t)j * kThreads;
      if (g < groups)
        reinterpret_cast<float4*>(ob)[g] = make_float4(l * a[j].x + w * c[j].x, l * a[j].y + w * c[j].y,
                                                       l * a[j].z + w * c[j].z, l * a[j].w + w * c[j].w);
    }
  } else {
    float a[kIters], c[kIters];
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t g = g0 + (int64_t)j * kThreads;
      if (g < groups) a[j] = xb[g], c[j] = xp[g];
    }
#pragma unroll
    for (int j = 0; j < kIters; ++j) {
      const int64_t g = g0 + (int64_t)j * kThreads;
      if (g < groups) ob[g] = l * a[j] + w * c[j];
    }
  }
}

// z_i of include/srk.h
__device__ __forceinline__ uint64_t hash_at(uint64_t seed, uint64_t i) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double uniform_at(uint64_t seed, uint64_t i) {
  return (double)(hash_at(seed, i) >> 11) * (1.0 / 9007199254740992.0);
}

// Every thread has read the state before the barrier; thread 0 advances the counter after it.
__global__ __launch_bounds__(kDrawThreads) void mixup_draw_kernel(uint64_t* state, int B, double alpha,
                                                                  int32_t* __restrict__ partner,
                                                                  float* __restrict__ lam) {
#pragma clang fp contract(off)
  const uint64_t seed = state[0] + 0xD1B54A32D192ED03ull * state[1];
  const double inv = 1.0 / alpha;
  int r = 0;
  if (B > 1) r = 1 + (int)(((hash_at(seed, 64ull * (uint64_t)B) >> 32) * (uint64_t)(B - 1)) >> 32);   // in [1, B - 1]
  for (int b = threadIdx.x; b < B; b += kDrawThreads) {
    double l = 1.0;
    if (B > 1) {
      for (int k = 0; k < SRK_MIXUP_TRIALS; ++k) {
        const uint64_t i = ((uint64_t)b * SRK_MIXUP_TRIALS + (uint64_t)k) * 2;
        const double U = uniform_at(seed, i), V = uniform_at(seed, i + 1);
        const double X = inv == 1.0 ? U : pow(U, inv), Y = inv == 1.0 ? V : pow(V, inv);
        const double S = X + Y;
        if (S > 0.0 && S <= 1.0) {
          l = X / S;
          l = fmax(l, 1.0 - l);
          break;
        }
      }
    }
    lam[b] = (float)l;
    int q = b + r;                       // < 2 B <= 2^25
    partner[b] = q >= B ? q - B : q;
  }
  __syncthreads();
  if (threadIdx.x == 0) state[1] += 1;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_mixup_draw(uint64_t* state, int64_t B, double alpha, int32_t* partner, float* lam, void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  SRK_REQUIRE(B >= 1 && B <= (int64_t(1) << 24), SRK_ERR_INVALID, "mixup_draw: needs 1 <= B <= 2^24, got %lld",
              (long long)B);
  SRK_REQUIRE(std::isfinite(alpha) && alpha >= 0.1 && alpha <= 1.0, SRK_ERR_INVALID,
              "mixup_draw: alpha must be in [0.1, 1], got %g", alpha);
  SRK_REQUIRE(state && partner && lam, SRK_ERR_INVALID, "mixup_draw: null pointer");
  hipStream_t s = as_stream(stream);
  const double bytes = 8.0 * (double)B + 32.0;
  ProfScope prof("mixup_draw", s, bytes);
  prof.bytes(bytes);
  prof.detail("mixup_draw_kernel %lld clips", (long long)B);
  hipLaunchKernelGGL(mixup_draw_kernel, dim3(1), dim3(kDrawThreads), 0, s, state, (int)B, alpha, partner, lam);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

int srk_mixup_apply(const float* x, int64_t B, int64_t n, const int32_t* partner, const float* lam, float* out,
                    void* stream) {
  SRK_API_BEGIN
  using namespace srk;
  constexpr int64_t kMax = (int64_t(1) << 31) - 1;
  SRK_REQUIRE(B >= 1 && B <= kMax && n >= 1 && n <= kMax, SRK_ERR_INVALID,
              "mixup_apply: needs 1 <= B, n <= 2^31 - 1, got B %lld n %lld", (long long)B, (long long)n);
  const int64_t chunks = (n + kChunk - 1) / kChunk;
  SRK_REQUIRE(B <= kMax / chunks, SRK_ERR_INVALID, "mixup_apply: B %lld x n %lld needs more than 2^31 - 1 workgroups",
              (long long)B, (long long)n);
  SRK_REQUIRE(x && partner && lam && out, SRK_ERR_INVALID, "mixup_apply: null pointer");
  const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
  const uintptr_t span = (uintptr_t)B * (uintptr_t)n * sizeof(float);
  SRK_REQUIRE(xa + span <= oa || oa + span <= xa, SRK_ERR_INVALID,
              "mixup_apply: out overlaps x (the call is out of place: a row is read as its own and as a partner's)");
  hipStream_t s = as_stream(stream);
  const bool vec = n % 4 == 0 && (xa & 15) == 0 && (oa & 15) == 0;
  const double bytes = 12.0 * (double)B * (double)n;
  ProfScope prof("mixup", s, bytes);
  prof.bytes(bytes);
  prof.detail("mixup_apply_kernel<%s> %lldx%lld", vec ? "v4" : "s1", (long long)B, (long long)n);
  const dim3 grid((unsigned)(B * chunks)), block(kThreads);
  if (vec)
    hipLaunchKernelGGL(mixup_apply_kernel<true>, grid, block, 0, s, x, (int)B, n, (int)chunks, partner, lam, out);
  else
    hipLaunchKernelGGL(mixup_apply_kernel<false>, grid, block, 0, s, x, (int)B, n, (int)chunks, partner, lam, out);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
  SRK_API_END
}

}  // extern "C"
