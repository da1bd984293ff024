// Internal helpers shared by every translation unit of libsrk.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>

#include "../../include/srk.h"
#include "options.h"

namespace srk {

// Thread-local last-error text, read back through srk_last_error() (include/srk.h).
void set_error(const char* fmt, ...);

#define SRK_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      ::srk::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return SRK_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

#define SRK_REQUIRE(cond, code, ...)     \
  do {                                   \
    if (!(cond)) {                       \
      ::srk::set_error(__VA_ARGS__);     \
      return (code);                     \
    }                                    \
  } while (0)

// Wraps the body of every extern "C" entry point: C++ exceptions never cross the C ABI.
#define SRK_API_BEGIN try {
#define SRK_API_END                                              \
  }                                                              \
  catch (const std::exception& e) {                              \
    ::srk::set_error("exception: %s", e.what());                 \
    return SRK_ERR_INTERNAL;                                     \
  }                                                              \
  catch (...) {                                                  \
    ::srk::set_error("unknown exception");                       \
    return SRK_ERR_INTERNAL;                                     \
  }

// Per-device constant tables (twiddles, windows, filterbanks, DCT), uploaded once by srk_init.
struct DeviceTables {
  bool ready = false;
  // FFT twiddles exp(-2*pi*i*t/M), float2 interleaved
  float2* tw256 = nullptr;     // M = 256 (fbank, N = 512)
  float2* tw320 = nullptr;     // M = 320 (mfcc / spec, N = 640)
  float2* post512 = nullptr;   // exp(-2*pi*i*k/512), k = 0..256
  float2* post640 = nullptr;   // exp(-2*pi*i*k/640), k = 0..320
  double* hamming400 = nullptr;
  double* tukey640 = nullptr;
  double* hann640 = nullptr;
  float* hann640f = nullptr;   // fp32 copies for the register-FFT kernels
  float* tukey640f = nullptr;
  float* hamming400f = nullptr;
  // filter banks as lane pairs (filter l and nf - 1 - l, balancing narrow and wide triangles):
  // meta {lo_a, cnt_a, lo_b, cnt_b}, weights of a then b, zero padded to a fixed tap count
  int4* fbp_meta = nullptr; float* fbp_w = nullptr;     // fbank: 60 pairs x 12 taps
  double* fb_hz = nullptr;     // [122] the fbank's unwarped mel points in Hz (K2-VTLP warps them per clip)
  float* dct = nullptr;        // [13][128] orthonormal DCT-II
  // Slaney mel as fixed 16-tap windows (zero-padded, start clamped so lo+16 <= bins)
  int* mel16_lo = nullptr; float* mel16_w = nullptr;   // [128], [128][16]
  float* mel16_wt = nullptr;                           // [16][128] (lane-coalesced)
  // Slaney mel as 64 lane pairs (a narrow filter <= 3 bins, a wide one <= 15 bins, bank-conflict-free
  // window starts; runtime.hip): {start_a, start_b, filter_a, filter_b} and [18][64] weights
  // (taps 0..2 from start_a, taps 3..17 from start_b)
  int4* melq_lo = nullptr; float* melq_w = nullptr;
  double spec_scale = 0.0;     // 1 / (fs * sum(w^2)) for the Tukey window
};

// Returns the tables for the current HIP device, building them on first use.
int get_tables(const DeviceTables** out);
// The host copy of DeviceTables::fb_hz (122 doubles, built on first use; no GPU needed).
const double* fbank_hz_points();

// Matrix-core operand precision of the GEMM-shaped kernels (srk_set_option "matmul_precision"):
// 0 = fp32 (exact fp32 MFMA, the reference's arithmetic), 1 = bf16, 2 = fp16 operands (rounded to
// nearest-even when staged into LDS) with fp32 accumulation and fp32 inputs / outputs.
enum MatmulPrec { kPrecF32 = 0, kPrecBF16 = 1, kPrecF16 = 2 };
int matmul_prec();
// Scoped override of matmul_prec() on this host thread (p < 0: no override): the conv forward passes under
// "conv_fwd_fp32" run their whole dispatch at fp32.
extern thread_local int t_prec_override;
struct PrecScope {
  int saved;
  explicit PrecScope(int p) : saved(t_prec_override) {
    if (p >= 0) t_prec_override = p;
  }
  ~PrecScope() { t_prec_override = saved; }
};

// Bumped whenever a library scratch buffer is (re)allocated: a captured HIP graph that refers to the
// old buffer must not be replayed (srk_scratch_generation; graphs.GraphedStep checks it).
extern std::atomic<int64_t> g_scratch_gen;
// Grow-only library scratch: one buffer per device, handed out again until a larger one is asked for.  Every
// use declares its own instance (runtime.hip); srk_set_option("release_scratch") frees them all.
class ScratchPool {
 public:
  ScratchPool() : next_(head_) { head_ = this; }
  ScratchPool(const ScratchPool&) = delete;
  ScratchPool& operator=(const ScratchPool&) = delete;
  // *out = at least `floats` floats on the current device.  Growing synchronizes the device, frees the old buffer
  // and bumps g_scratch_gen; a failed allocation leaves the device's slot empty.
  int get(size_t floats, float** out);
  // Free every buffer of every instance (device-synchronizing; bumps g_scratch_gen).
  static int release_all();

 private:
  struct Slot {
    float* p = nullptr;
    size_t floats = 0;
  };
  Slot slots_[64];   // by device index
  std::mutex mu_;
  ScratchPool* next_;           // the instances, linked as they are constructed
  static ScratchPool* head_;
};

// Runtime options (srk_set_option): options.h states each one once; these are its variables, defined in runtime.hip.
#define SRK_DECLARE_OPTION(type, var, name, accepts, def, doc) extern type var;
#define SRK_HOOKED_OPTION(name, hook, accepts, def, doc)
SRK_OPTION_LIST(SRK_DECLARE_OPTION, SRK_HOOKED_OPTION)
#undef SRK_DECLARE_OPTION
#undef SRK_HOOKED_OPTION
// What the hooked options store (matmul_precision: matmul_prec() above).
extern unsigned long long* g_opt_gru_trace;   // "gru_trace_ptr": device buffer or nullptr
extern unsigned g_opt_gru_dc_offset;          // "gru_dc_offset_ns" in ticks of 10 ns
extern int g_opt_gru_dwhh_fused;              // "gru_dwhh_fused": 0, or an odd value (bit 0 = fused)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// RAII event pair around one kernel launch (prof.hip); inert unless srk_prof_enable(1).
// `work` = the launch's ALGORITHMIC flops (matrix kernels) or bytes (streaming kernels).
class ProfScope {
 public:
  ProfScope(const char* name, hipStream_t s, double work = 0.0);
  ~ProfScope();
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
  // The launch's kernel and shape ("gemm_f32_kernel<NT,256x128> 13056x3072x1024"), printf-style;
  // srk_prof_kernels groups records by (name, detail).  No-op (no formatting) when profiling is off.
  void detail(const char* fmt, ...) __attribute__((format(printf, 2, 3)));
  // The launch's ALGORITHMIC HBM bytes (matrix kernels, whose `work` is flops): each operand tensor read
  // once + the output written once — what PMC traffic is priced against.
  void bytes(double b) { bytes_ = b; }
  // Whether this scope records (profiling on): callers skip building a detail string otherwise.
  bool on() const { return a_ != nullptr; }

 private:
  const char* name_;
  hipStream_t s_;
  void* a_;
  double work_;
  double bytes_ = 0.0;
  unsigned long long opened_ = 0;   // this scope's number among the thread's scopes (innermost-wins nesting)
  char detail_[96];
};

}  // namespace srk
