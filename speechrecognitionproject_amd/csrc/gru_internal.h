// Internal interface between gru.hip (entry points, per-step kernels) and gru_persistent.hip
// (one-launch-per-layer recurrence kernels).
#pragma once
#include <algorithm>

#include "srk_internal.h"

namespace srk {

// Arrival counters / per-producer flags of the persistent kernels ([2 directions][groups <= 4] at a
// 64-B stride, or [2][G][32] flags: words 0..255; the fp32 two-chain kernels' per-wave flags
// [2 dir][G][2 chains][2 row blocks][32 slices][2 k halves]: words 0..2047), the XCD census in
// words kCensusOff..+8; zeroed by zero_counters_kernel over exactly this block before every launch.
constexpr int kCounterFloats = 4096;
constexpr int kCensusOff = 4080;
// Word indices of the step-ordering state inside that block — host + device, so the kernels and
// srk_gru_audit_words (a host-side check of every word a launch plan touches) share one arithmetic.
__host__ __device__ constexpr int pw_counter(int dir, int G, int group) { return (dir * G + group) * 16; }
__host__ __device__ constexpr int pw_flag64(int dir, int G, int group, int slot) { return (dir * G + group) * 32 + slot; }
__host__ __device__ constexpr int pw_flag_lp2(int dir, int G, int group, int slot) { return (dir * G + group) * 16 + slot; }
__host__ __device__ constexpr int pw_flag_dc(int dir, int G, int group, int c, int rb, int slot) {
  return (((dir * G + group) * 2 + c) * 2 + rb) * 64 + slot;
}
// Hand-off ring depth of the persistent kernels (slots per direction in the workspace): the fp32
// two-chain kernels need 3 (a wave waits only for the producers of its k half, see gru_persistent.hip)
constexpr int kHandoffSlots = 3;
constexpr int kFusedIn = 64;   // widest layer input whose projection the forward kernels fuse

struct GruPArgs {
  int B, T, H;
  int G;                 // 64-row groups in this launch
  int b_begin, b_end;    // batch rows [b_begin, b_end) of this launch
  const float* gi;       // fwd: [B*T][6H]
  const float* w_hh;     // [2][3H][H]
  const float* b_hh;     // [2][3H]
  float* y;              // fwd output [B][T][2H] (also the h hand-off buffer)
  const float* y_in;     // bwd: the forward output
  float* gates;          // [2][T][B][4H]
  const float* dy;       // bwd: [B][T][2H]
  float* dgi;            // bwd: [B*T][6H]
  float* dgh;            // bwd: [2][B][T][3H] (also the dg hand-off buffer)
  float* dgh_edge;       // bwd: [2][B][3H]
  float* xbuf;           // hand-off ping-pong: fwd h [2 dir][2][B][H], bwd dg [2 dir][2][B][3H]
  unsigned* counters;    // kCounterFloats words
  int flags;             // 1: per-producer step flags [2][G][32] (sc1 stores) instead of arrival counters
  int xcd_local;         // 1: try the XCD-local hand-off (census at launch; plain stores kept in the XCD's L2)
  // 16-bit operand outputs of the bf16 / fp16 kernels (nullptr = off), for the GEMMs of the layer:
  uint16_t* y16;         // fwd: h [B][T][2H] rounded to 16 bit
  uint16_t* dgi16;       // bwd: dgi [B*T][6H] (replaces the fp32 dgi)
  uint16_t* dgh16;       // bwd: dgh [2][B][T][3H], edge rows zero (replaces dgh / dgh_edge)
  float* dbias;          // bwd with dgi16: bias-gradient partials [chunk * (256 / rows per group) + group][2 dir][4][H]
                         //   (sum over t and the group's rows of dar, daz, dan, dan * r)
  int chunk;             // index of this launch's 64*G-row batch chunk
  // fused small input projection (in <= kFusedIn, the 39 MFCC features of model_mfcc_bgru.py:25):
  // with x_in set the forward kernels compute gi_t = x_t W_ih^T + b_ih themselves (gi unused)
  const float* x_in;     // [B][T][in]
  const float* w_ih;     // [2][3H][in]
  const float* b_ih;     // [2][3H]
  int in;
  unsigned long long* trace;   // optional per-(workgroup, step) timestamps (tools/gru_trace.py)
  unsigned* health;      // host-pinned, device-mapped word: set when a spin-wait gives up (srk_health_check)
  unsigned spin_limit;   // s_sleep polls before a wait gives up (~2 s by default)
  unsigned dc_offset;    // fp32 two-chain kernels: chain 1 starts this many s_memrealtime ticks (10 ns) late
  int fast_cell;         // fp32 two-chain forward: hardware exp / rcp in the cell (v_exp_f32, v_rcp_f32)
  int dc_prio;           // fp32 two-chain kernels: 0 = equal priority, 1 / 2 = chain 0 / 1 at s_setprio 1
  // 16-bit backward with the recurrent weight gradient fused in (gru_dwhh_fused_parts): h_prev in 16 bit
  // (the forward's y16) and the per-(chunk, row group) partial dW_hh [part][2 dir][3H][H], summed by
  // dwhh_reduce_kernel
  const uint16_t* y16_in;
  float* dw_part;
  int dw_mode;           // option gru_dwhh_fused bits: 2 = h_prev fetched after the exchange barrier, 4 = recurrence waves at prio 1
  int one_dir;           // fp32 kernels: 1 = the forward direction only (0 = both).  Same grid, placement and census; the
                         //   reverse direction's workgroups return right after place() (srk_gru_top_last_*)
};

// The GRU cell's nonlinearities, shared by the recurrence kernels and the single-cell kernels of gru.hip.
__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
// 16-bit kernels and the fp32 two-chain forward (option gru_fp32_fast_cell): the hardware exp / reciprocal
// forms (v_exp_f32, v_rcp_f32: ~1 ulp) keep the cell epilogue short on the step-to-step chain.
__device__ __forceinline__ float sigmoid_fast(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 2.0f * sigmoid_fast(2.0f * x) - 1.0f; }

size_t fwd_lds_bytes(int H);
size_t bwd_lds_bytes(int H);

// Which kernel runs the recurrence of one direction of travel (forward or backward pass) of a layer.
enum GruVariant {
  kGruStep = 0,   // no persistent kernel: the per-step kernels of gru.hip
  kGruF32,        // fp32, 4 waves
  kGruDc,         // fp32, two row chains per workgroup (option gru_fp32_dual_chain), gi / dgi in memory
  kGruDcFused,    // the two-chain forward with the fused input projection (in <= kFusedIn)
  kGruLp,         // 16-bit, 64 rows x 16 units
  kGruLp2,        // 16-bit, 32 x 32 (option gru_lp_32x32)
  kGruLp2Wide,    // its 64-row form (RB = 4) for B > 256: up to 512 rows per launch (option gru_lp_wide)
  kGruLp2Dw,      // the 32 x 32 backward with the recurrent weight gradient fused in (option gru_dwhh_fused)
  kGruLp2Ow,      // the 32 x 32 forward with output / input worker waves (option gru_fwd_worker)
};
// The option values the selection rule reads (gru_opts(): the current srk_set_option state)
struct GruOpts {
  int persistent, lp2, lp_wide, dc, fast_cell, dwhh_fused, fwd_worker;
};
GruOpts gru_opts();
// "Does variant v's kernel (at prec, this direction of travel) fit one workgroup per CU?": > 0 yes.  For the base
// kernels (kGruF32, kGruLp) `grid` workgroups must also be co-resident on the device; kGruDc asks for all three
// two-chain kernels.  gru_fit_measured is the device's answer (cached per kernel, one query per process); the
// host-side audit passes "everything fits".
using GruFitFn = int (*)(GruVariant v, int prec, bool backward, int grid);
int gru_fit_measured(GruVariant v, int prec, bool backward, int grid);
// The launch plan of one recurrence: everything gru_persistent_launch, the workspace users in gru.hip and
// srk_gru_audit_words need to know about the variant.
struct GruRecPlan {
  GruVariant variant = kGruStep;
  int prec = 0;
  const void* kernel = nullptr;   // void (*)(GruPArgs)
  int block = 0;
  size_t lds = 0;
  int rows_per_launch = 0;   // batch rows per launch (chunk)
  int rows_g = 0;            // batch rows per workgroup group
  int slices = 0;            // unit slices (workgroups per group and direction)
  int bias_part_rows = 0;    // 16-bit backward: batch rows per bias-gradient partial (256-row chunks)
  int dw_parts = 0;          // kGruLp2Dw: partials of dW_hh the kernel writes (chunks x 8), else 0
  bool fast_cell = false;    // fp32 forward cells evaluated with sigmoid_fast / tanh_fast (two-chain kernel + option)
  const char* suffix = "";   // of the profiler detail string
};
// THE selection rule.  in_fused: the input width when the forward kernel projects the input itself, else 0;
// out16: the launch has its 16-bit outputs (forward y16, backward dgi16 / dgh16).  variant == kGruStep when the
// persistent kernels cannot run this layer (option off, H, 32-bit buffer offsets, co-residency).
GruRecPlan gru_rec_plan(int64_t B, int64_t T, int64_t H, int in_fused, int prec, bool backward, bool out16,
                        const GruOpts& o, GruFitFn fits);
// Enqueue the whole recurrence (all T steps; batch split into the plan's co-resident chunks).
int gru_persistent_launch(GruPArgs a, const GruRecPlan& plan, bool backward, hipStream_t s);

// Host-pinned health word (device-mapped pointer in *dev): non-zero once any persistent-kernel
// spin-wait has given up; read without a device synchronization by srk_health_check.
int health_word(unsigned** host, unsigned** dev);

}  // namespace srk
