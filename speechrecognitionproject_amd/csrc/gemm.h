// Internal GEMM interface (row-major):  C[M,N] = alpha * op(A) * op(B) + beta * C (+ bias)
//   op(A) = A [M,K] (lda)       or A^T with A stored [K,M] when ta
//   op(B) = B [K,N] (ldb)       or B^T with B stored [N,K] when tb
// bias_mode: 0 none, 1 bias[N] added to every row, 2 bias[M] added to every column.
// Batched over `batch` with element strides sA/sB/sC (0 = shared operand).
// Long-K shapes are split over K internally (deterministic slab reduction, grow-only scratch).
#pragma once
#include "srk_internal.h"

namespace srk {

struct GemmDesc {
  int64_t M = 0, N = 0, K = 0;
  const float* A = nullptr; int64_t lda = 0; bool ta = false;
  const float* B = nullptr; int64_t ldb = 0; bool tb = false;
  float* C = nullptr; int64_t ldc = 0;
  float alpha = 1.f, beta = 0.f;
  const float* bias = nullptr; int bias_mode = 0;
  int batch = 1; int64_t sA = 0, sB = 0, sC = 0;
  // optional fused row sums of op(A): rowsum[m] = rowsum_beta * rowsum[m] + sum_k op(A)[m, k]
  float* rowsum = nullptr; float rowsum_beta = 0.f;
  int64_t sRS = 0;   // batched launches: batch z's row sums at rowsum + z sRS
  // matrix-core operand precision (MatmulPrec); -1 = the process setting (srk_set_option)
  int prec = -1;
  // 16-bit operands already in memory (bf16 / fp16 per `prec`, same layouts and leading dimensions
  // in elements): when BOTH are set they replace A / B and no rounding happens on chip (half the
  // operand bytes).  No fused row sums on this path.
  const uint16_t* A16 = nullptr;
  const uint16_t* B16 = nullptr;
  // A launch that computes PART of a larger GEMM and must give its elements that GEMM's bits (an element's sum
  // order depends on the kernel and the K split, not on the tile grid): no_split = never split K (the larger GEMM
  // is known not to); plan_batch > 1 = choose the kernel and the K split as the batched launch of plan_batch
  // such products would, while running `batch` of them.
  bool no_split = false;
  int plan_batch = 0;
  // plan_M > 0 = choose the kernel and the K split as the GEMM with M = plan_M would (this launch computes some
  // of that GEMM's rows).  pin_splits > 0 = take exactly pin_splits K slabs of pin_kchunk each (a multiple of the
  // kernel's K-tile, K within the last slab): an operand whose all-zero k blocks were deleted slab by slab
  // (PackPlan) keeps the slabs of the GEMM it came from.
  int64_t plan_M = 0;
  int pin_splits = 0;
  int64_t pin_kchunk = 0;
  // k_live > 0 (gemm_f32_klive only; gemm_plan ignores these four): columns k >= k_live of op(A) are zero in every
  // row but the live rows live_first, live_first + live_stride, ... (live_count of them; stride >= 8 as in PackPlan).
  int64_t k_live = 0, live_first = 0, live_stride = 0, live_count = 0;
};

// Enqueue on `stream`; returns SRK_OK or an srk_status.
int gemm_f32(const GemmDesc& d, hipStream_t stream);

// Pin `part` (some rows / columns of `full`, the same K) to full's K split, so that its elements get full's bits
// whatever tile its own shape takes.  True with part.pin_splits / pin_kchunk set when both plan on one kernel family
// (same K-tile, same precision) and full is neither skinny nor stream-K; false, pins cleared, otherwise.
bool gemm_f32_pin_as(const GemmDesc& full, GemmDesc& part);

// What gemm_plan decides for `d`, for callers that build part-GEMMs of it: whether it runs on gemm_p32_kernel
// without stream-K, and its K split (count, slab length).  False when the plan fails or is another kernel's.
bool gemm_f32_p32_split(const GemmDesc& d, int* splits, int64_t* kchunk);

// Up to 4 part-GEMMs in ONE gemm_p32_kernel launch (a captured graph is a chain of kernels: parts that each
// fill half of the CUs share the chip only inside one launch).  Every member must plan as the non-stream-K
// gemm_p32_kernel of one (ta, tb) instantiation, batch 1; anything else is refused.  Members run longest K slab
// first; each gets the split reductions gemm_f32 would issue after it.  An element's bits are those of its
// member's own gemm_f32 call.
constexpr int kGemmGroupMax = 4;
int gemm_f32_group(const GemmDesc* ds, int n, hipStream_t stream);
// Process-start switch SRK_GEMM_GROUP (default 1): 0 = callers issue their part-GEMMs as before (A/B measurements).
bool gemm_group_enabled();

// A stream-K gemm_p32_kernel GEMM whose op(A) is zero at k >= d.k_live in all rows but d's live rows, without the
// K-tiles known to be zero: the launch of gemm_f32(d) with the same cuts, every segment clipped to k_live (a
// segment past it does nothing), the fixup over the live runs, then one kernel that recomputes the live rows over
// the full K with the full plan's cuts and run order.  An element's bits depend on its accumulator chain and on
// where K is cut, and a K-tile whose A rows are zero leaves every chain as it was, so the result equals
// gemm_f32(d) on the zero-filled operand bit for bit -- up to the sign of a zero (x + (+0) against no add), and for
// finite B only (the full GEMM turns 0 * inf into NaN, this one never multiplies it).  Columns k >= k_live of the
// dead rows are never read.  gemm_f32_klive_ok: the plan of d is the fp32 stream-K gemm_p32_kernel, non-transposed
// A, batch 1, alpha 1, beta 0, no bias, no row sums, k_live a positive multiple of the K-tile below K, stride >= 8,
// every live row below M; gemm_f32_klive refuses anything else with SRK_ERR_INVALID.
bool gemm_f32_klive_ok(const GemmDesc& d);
int gemm_f32_klive(const GemmDesc& d, hipStream_t stream);
// Process-start switch SRK_GEMM_KLIVE (default 1): 0 = callers keep the full GEMM (A/B measurements).
bool gemm_klive_enabled();

// Zero-block packing of a K dimension whose only nonzero A rows are `count` live rows first, first + stride, ...
// (stride >= 8, so each sits in an 8-aligned k block of its own).  Every 8-block holding a live row is kept, in
// the slab (of `slab` k, a multiple of 16) of its original k and at its own place k mod 8 in the block; every
// slab is padded with zero blocks to the common length pslab (a multiple of 16).  gemm_p32_kernel walks K in 8-deep
// blocks with one accumulator chain per element, and an all-zero block leaves every chain as it was, so the
// packed GEMM pinned to nslabs x pslab has the bits of the full one (up to the sign of a zero).
struct PackPlan {
  int64_t K = 0, slab = 0, first = 0, stride = 0, count = 0;
  int64_t nslabs = 0, pslab = 0;
  // live rows of slab s: indices [lo(s), lo(s + 1))
  __host__ __device__ int64_t lo(int64_t s) const {
    const int64_t k0 = s * slab;
    if (s >= nslabs) return count;
    if (k0 <= first) return 0;
    const int64_t b = (k0 - first + stride - 1) / stride;
    return b < count ? b : count;
  }
  // source row of packed row kp, or -1 for a row of a zero block; *live = it is the block's live row
  __host__ __device__ int64_t src(int64_t kp, bool* live) const {
    const int64_t s = kp / pslab, r = kp - s * pslab, b = lo(s) + (r >> 3);
    *live = false;
    if (b >= lo(s + 1)) return -1;
    const int64_t k = first + b * stride, row = (k & ~(int64_t)7) + (r & 7);
    *live = row == k;
    return row;
  }
};
// Fills `p` (SRK_ERR_INVALID on bad arguments: K, count < 1, slab not a positive multiple of 16, first < 0,
// stride < 8, a live row at or past K).
int pack_plan(int64_t K, int64_t slab, int64_t first, int64_t stride, int64_t count, PackPlan& p);
// One kernel: Ap [nslabs pslab][wa] = the live rows of A (lda) at their packed places, zeros elsewhere;
// Bp [nslabs pslab][wb] = the rows of B (ldb) of the kept blocks, zeros in zero blocks and for k >= K.
// wa, wb, lda, ldb multiples of 4; 16-B aligned pointers.
int gemm_pack_rows(const PackPlan& p, const float* A, int64_t lda, int64_t wa, const float* B, int64_t ldb, int64_t wb,
                   float* Ap, float* Bp, hipStream_t stream);

// Whether gemm_f32 accepts `d` with batch > 1 AND fused row sums (the fp32-operand ping-pong
// kernel only); callers fall back to one launch per batch entry otherwise.
bool gemm_f32_batched_rowsum_ok(const GemmDesc& d);

// Column sums: out[n] = beta*out[n] + sum_m X[m, n] (X row-major [M,N], ldx).
int colsum_f32(const float* X, int64_t M, int64_t N, int64_t ldx, float* out, float beta, hipStream_t stream);

}  // namespace srk
