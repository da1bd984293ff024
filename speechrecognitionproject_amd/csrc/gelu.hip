// GELU, erf form (include/srk.h srk_gelu_fwd / _bwd; nn.GELU): y = x Phi(x), dx = dy (Phi(x) + x phi(x)) with
// Phi(x) = erfc(-x / sqrt 2) / 2 and phi(x) = exp(-x^2 / 2) / sqrt(2 pi).  erfc keeps the left tail's relative
// accuracy (1 + erf cancels there) and saturates to 0 / 2, so every finite x gives a finite y and dx: at |x| large
// x^2 overflows to +inf, exp(-inf) = 0 and x * 0 = 0.  NaN propagates through both.
//
// One element per lane slot, memory bound (8 / 12 bytes per element).  16-byte aligned tensors run float4 slots with
// the n % 4 tail on scalar slots of the same launch; any misaligned base runs scalar slots throughout.
#include <cmath>

#include "srk_internal.h"

namespace srk {
namespace {

constexpr int kThreads = 256;
constexpr float kRsqrt2 = 0.70710678118654752440f;
constexpr float kRsqrt2Pi = 0.39894228040143267794f;

__device__ __forceinline__ float cdf(float x) { return 0.5f * erfcf(-x * kRsqrt2); }
__device__ __forceinline__ float gelu(float x) { return x * cdf(x); }
__device__ __forceinline__ float dgelu(float x, float dy) {
  return dy * (cdf(x) + x * (kRsqrt2Pi * expf(-0.5f * x * x)));
}

// slots [0, n4): float4 i; slots [n4, n4 + tail): element 4 n4 + (slot - n4).  VEC false: n4 = 0, tail = n.
template <bool BWD>
__global__ __launch_bounds__(kThreads) void gelu_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                        int64_t n4, int64_t tail, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n4) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float4 r;
    if (BWD) {
      const float4 g = reinterpret_cast<const float4*>(dy)[i];
      r = make_float4(dgelu(v.x, g.x), dgelu(v.y, g.y), dgelu(v.z, g.z), dgelu(v.w, g.w));
    } else {
      r = make_float4(gelu(v.x), gelu(v.y), gelu(v.z), gelu(v.w));
    }
    reinterpret_cast<float4*>(out)[i] = r;
  } else if (i < n4 + tail) {
    const int64_t e = 4 * n4 + (i - n4);
    out[e] = BWD ? dgelu(x[e], dy[e]) : gelu(x[e]);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BWD>
int launch(const float* x, const float* dy, int64_t n, float* out, hipStream_t s) {
  const bool vec = aligned16(x) && aligned16(out) && (!BWD || aligned16(dy));
  const int64_t n4 = vec ? n / 4 : 0, tail = n - 4 * n4;
  const double bytes = 4.0 * (BWD ? 3.0 : 2.0) * (double)n;
  ProfScope prof("gelu", s, bytes);
  prof.bytes(bytes);
  prof.detail("gelu_kernel<%s,%s> %lld", BWD ? "bwd" : "fwd", vec ? "vec" : "scalar", (long long)n);
  const int64_t slots = n4 + tail;
  const dim3 grid((unsigned)((slots + kThreads - 1) / kThreads)), block(kThreads);
  hipLaunchKernelGGL(gelu_kernel<BWD>, grid, block, 0, s, x, dy, n4, tail, out);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
}

}  // namespace
}  // namespace srk

extern "C" {

int srk_gelu_fwd(const float* x, int64_t n, float* y, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 1 && n < (1LL << 31), SRK_ERR_INVALID, "gelu_fwd: needs 1 <= n < 2^31, got %lld", (long long)n);
  SRK_REQUIRE(x && y, SRK_ERR_INVALID, "gelu_fwd: null pointer");
  return srk::launch<false>(x, nullptr, n, y, srk::as_stream(stream));
  SRK_API_END
}

int srk_gelu_bwd(const float* x, const float* dy, int64_t n, float* dx, void* stream) {
  SRK_API_BEGIN
  SRK_REQUIRE(n >= 1 && n < (1LL << 31), SRK_ERR_INVALID, "gelu_bwd: needs 1 <= n < 2^31, got %lld", (long long)n);
  SRK_REQUIRE(x && dy && dx, SRK_ERR_INVALID, "gelu_bwd: null pointer");
  return srk::launch<true>(x, dy, n, dx, srk::as_stream(stream));
  SRK_API_END
}

}  // extern "C"
