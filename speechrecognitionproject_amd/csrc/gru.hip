// K5: bidirectional GRU layer forward / backward (PyTorch gate convention [r; z; n], h0 = 0),
// replacing nn.GRU(bidirectional=True, batch_first=True) at models/model_mfcc_bgru.py:25,35,
// model_spec_bgru.py:23,33 and model_resnet_bgru.py:130,135.
//
//   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
//   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h
//
// Forward  = one MFMA GEMM for the input projections of BOTH directions and all T steps
//            (gi = x W_ih_cat^T + b_ih, [B*T, 6H]), then T launches of a fused recurrence step
//            kernel: gh = h_{t-1} W_hh^T on the matrix cores with the gate math as its epilogue.
// Backward = T launches of a fused step kernel (dh_{t} = dy_t + dgh_{t+1} W_hh + dh_{t+1} z_{t+1},
//            then the gate derivatives as epilogue), followed by the weight-gradient GEMMs
//            (dW_ih = dgi^T x, dW_hh = dgh^T h_prev with K = B*T) and column sums for the biases.
//
// On H = 512 the T step launches are ONE launch per batch chunk of a persistent recurrence kernel
// (gru_persistent.hip; gru_rec_plan picks the variant), and in bf16 / fp16 mode the GEMM operands live in memory
// in 16 bit.
//
// Workspace (fp32, caller-owned; sizes in srk_gru_workspace_floats; struct GruWs below is the layout):
//   fwd:  gi [B*T, 6H] | gates [2][T][B][4H] (r, z, n, W_hn h + b_hn)       — kept for backward
//   bwd:  dgi [B*T, 6H] | dgh [2][B][T][3H] | dgh_edge [2][B][3H] | dhz [2][B][H]
//   both, each block 64-float aligned: | the persistent kernels' hand-off ring | their kCounterFloats step-ordering
//   words | the in4 pad block (in % 4 != 0) | the 16-bit block (H = 512: x16, W16, y16 / bias partials, dW_ih
//   and dx at width in8); srk_gru_top_last_bwd appends its [B][T][2H] dy.
#include <algorithm>

#include "gemm.h"
#include "gru_internal.h"

namespace srk {
namespace {

// Recurrence step tiling.  One workgroup = 64 batch rows x 16 hidden units of one direction
// (all three gates: 48 columns of W_hh for the forward step), 4 waves = 4 x 16 rows.
// Both operands are staged ROW-major in LDS (row pitch BK+4 floats) and read as float4: for
// MFMA k-substep s a lane with k-quad q uses k = kbase + 4q + s, for A and B alike (any fixed
// permutation of k is a valid GEMM order), so one ds_read_b128 feeds four v_mfma_f32_16x16x4_f32.
// Workgroup -> (direction, batch group, unit slice) is XCD-aware: the 32 workgroups that share
// an XCD (blockIdx % 8, observed round-robin dispatch) take the slices of ONE (direction, group)
// pair, so that direction's W_hh (3 MB fp32) stays resident in that XCD's 4 MB L2 from one step
// launch to the next.  (Placement only changes speed, never results.)
constexpr int kRows = 64;    // batch rows per workgroup
constexpr int kUnits = 16;   // hidden units per workgroup
constexpr int kBK = 128;     // k per LDS stage
constexpr int kPitch = kBK + 4;

struct GruArgs {
  int B, T, H, in;
  int G, S;             // batch groups (ceil(B/64)), unit slices (H/16)
  const float* y_in;    // fwd: y (h_prev source); bwd: y
  float* y;             // fwd output [B][T][2H]
  const float* gi;      // [B*T][6H]
  const float* w_hh;    // [2][3H][H]
  const float* b_hh;    // [2][3H]
  float* gates;         // [2][T][B][4H]
  const float* dy;      // [B][T][2H]
  float* dgi;           // [B*T][6H]
  float* dgh;           // [2][B][T][3H]
  float* dgh_edge;      // [2][B][3H]
  float* dhz;           // [2][B][H]
};

// Native 4-float vector: HIP's float4 is a struct whose copies lower to memcpy, which SROA cannot
// keep in registers (a float4 staging array ends up in scratch); ext_vector loads/stores do not.
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4f ld4(const float* p) { return *reinterpret_cast<const v4f*>(p); }
__device__ __forceinline__ void st4(float* p, v4f v) { *reinterpret_cast<v4f*>(p) = v; }

__device__ __forceinline__ void map_block(const GruArgs& a, int& dir, int& group, int& slice) {
  const int nwg = 2 * a.G * a.S;
  const int b = blockIdx.x, xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  const int pair = wgid / a.S;
  slice = wgid % a.S;
  dir = pair / a.G;
  group = pair % a.G;
}

// ------------------------------------------------------------------ forward step
// gh[b, g*H + j] = sum_k h_prev[b, k] W_hh[g*H + j, k];  epilogue = the GRU cell.
__global__ __launch_bounds__(256) void gru_fwd_step_kernel(GruArgs a, int step) {
  constexpr int WR = 3 * kUnits;                        // W rows (gate columns) per workgroup
  constexpr int VA = kRows * kBK / 4 / 256;             // float4 per thread per stage: 8
  constexpr int VW = WR * kBK / 4 / 256;                // 6
  __shared__ __attribute__((aligned(16))) float smem[2 * (kRows + WR) * kPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  int dir, group, slice;
  map_block(a, dir, group, slice);
  const int B = a.B, T = a.T, H = a.H;
  const int t = dir == 0 ? step : T - 1 - step;
  const int tprev = dir == 0 ? t - 1 : t + 1;
  const int b0 = group * kRows, j0 = slice * kUnits;
  const float* __restrict__ W = a.w_hh + (size_t)dir * 3 * H * H;

  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (step > 0) {
    v4f ra[VA], rw[VW];
    auto load = [&](int k0) {
#pragma unroll
      for (int i = 0; i < VA; ++i) {
        const int v = tid + i * 256, row = v / (kBK / 4), kq = (v % (kBK / 4)) * 4;
        const int b = b0 + row;
        const v4f x = ld4(a.y_in + ((size_t)(b < B ? b : B - 1) * T + tprev) * 2 * H + dir * H + k0 + kq);
        ra[i] = b < B ? x : v4f{0.f, 0.f, 0.f, 0.f};   // clamped row + select: no exec-masked loads
      }
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        const int v = tid + i * 256, c = v / (kBK / 4), kq = (v % (kBK / 4)) * 4;
        const int g = c / kUnits, jj = c % kUnits;
        rw[i] = ld4(W + (size_t)(g * H + j0 + jj) * H + k0 + kq);
      }
    };
    auto store = [&](int buf) {
      float* As = smem + buf * (kRows + WR) * kPitch;
      float* Ws = As + kRows * kPitch;
#pragma unroll
      for (int i = 0; i < VA; ++i) {
        const int v = tid + i * 256, row = v / (kBK / 4), kq = (v % (kBK / 4)) * 4;
        st4(As + row * kPitch + kq, ra[i]);
      }
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        const int v = tid + i * 256, c = v / (kBK / 4), kq = (v % (kBK / 4)) * 4;
        st4(Ws + c * kPitch + kq, rw[i]);
      }
    };
    const int nk = H / kBK;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) load((kt + 1) * kBK);
      const float* As = smem + cur * (kRows + WR) * kPitch;
      const float* Ws = As + kRows * kPitch;
#pragma unroll
      for (int kb = 0; kb < kBK; kb += 16) {
        const v4f av = ld4(As + (wave * 16 + lr) * kPitch + kb + 4 * lq);
        v4f wv[3];
#pragma unroll
        for (int g = 0; g < 3; ++g) wv[g] = ld4(Ws + (g * kUnits + lr) * kPitch + kb + 4 * lq);
#pragma unroll
        for (int g = 0; g < 3; ++g) {
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv[g].x, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv[g].y, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv[g].z, acc[g], 0, 0, 0);
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv[g].w, acc[g], 0, 0, 0);
        }
      }
      asm volatile("" ::: "memory");      // keep the stage-k+1 LDS store (and its vmcnt wait)
      __builtin_amdgcn_sched_barrier(0);   // after this stage's MFMAs
      if (kt + 1 < nk) store(cur ^ 1);
      __syncthreads();
    }
  }

  // epilogue: lane owns rows 16*wave + 4*lq + r, unit j = j0 + lr, all three gates
  const int j = j0 + lr;
  const float bhr = a.b_hh[dir * 3 * H + j], bhz = a.b_hh[dir * 3 * H + H + j], bhn = a.b_hh[dir * 3 * H + 2 * H + j];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + wave * 16 + lq * 4 + r;
    if (b >= B) continue;
    const float* gi = a.gi + ((size_t)b * T + t) * 6 * H + dir * 3 * H;
    const float ghn = acc[2][r] + bhn;
    const float rg = sigmoidf_(gi[j] + (acc[0][r] + bhr));
    const float zg = sigmoidf_(gi[H + j] + (acc[1][r] + bhz));
    const float ng = tanhf(gi[2 * H + j] + rg * ghn);
    const float hp = step > 0 ? a.y_in[((size_t)b * T + tprev) * 2 * H + dir * H + j] : 0.f;
    const float h = (1.0f - zg) * ng + zg * hp;
    a.y[((size_t)b * T + t) * 2 * H + dir * H + j] = h;
    float* gs = a.gates + (((size_t)dir * T + t) * B + b) * 4 * H;
    gs[j] = rg;
    gs[H + j] = zg;
    gs[2 * H + j] = ng;
    gs[3 * H + j] = ghn;
  }
}

// ------------------------------------------------------------------ backward step
// dh_rec[b, j] = sum_c dgh_next[b, c] W_hh[c, j] (c over 3H);  epilogue = the cell derivatives.
__global__ __launch_bounds__(256) void gru_bwd_step_kernel(GruArgs a, int step) {
  constexpr int VA = kRows * kBK / 4 / 256;             // 8
  constexpr int VW = kBK * kUnits / 4 / 256;            // 2
  __shared__ __attribute__((aligned(16))) float smem[2 * (kRows + kUnits) * kPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  int dir, group, slice;
  map_block(a, dir, group, slice);
  const int B = a.B, T = a.T, H = a.H;
  const int t = dir == 0 ? T - 1 - step : step;          // time processed now
  const int tnext = dir == 0 ? t + 1 : t - 1;           // processed by the previous step
  const int tprev = dir == 0 ? t - 1 : t + 1;           // h_prev source
  const bool edge = (step == T - 1);                    // h_prev = 0 here
  const int b0 = group * kRows, j0 = slice * kUnits;
  const float* __restrict__ W = a.w_hh + (size_t)dir * 3 * H * H;
  const float* __restrict__ dghn = a.dgh + (size_t)dir * B * T * 3 * H;   // [B][T][3H] of this dir

  typedef float f32x4 __attribute__((ext_vector_type(4)));
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  if (step > 0) {
    v4f ra[VA], rw[VW];
    auto load = [&](int k0) {
#pragma unroll
      for (int i = 0; i < VA; ++i) {
        const int v = tid + i * 256, row = v / (kBK / 4), kq = (v % (kBK / 4)) * 4;
        const int b = b0 + row;
        const v4f x = ld4(dghn + ((size_t)(b < B ? b : B - 1) * T + tnext) * 3 * H + k0 + kq);
        ra[i] = b < B ? x : v4f{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int i = 0; i < VW; ++i) {   // W_hh[k0 + kr][j0 .. j0+15], 4 units per float4
        const int v = tid + i * 256, kr = v / (kUnits / 4), jq = (v % (kUnits / 4)) * 4;
        rw[i] = ld4(W + (size_t)(k0 + kr) * H + j0 + jq);
      }
    };
    auto store = [&](int buf) {
      float* As = smem + buf * (kRows + kUnits) * kPitch;
      float* Ws = As + kRows * kPitch;    // [unit][k]
#pragma unroll
      for (int i = 0; i < VA; ++i) {
        const int v = tid + i * 256, row = v / (kBK / 4), kq = (v % (kBK / 4)) * 4;
        st4(As + row * kPitch + kq, ra[i]);
      }
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        const int v = tid + i * 256, kr = v / (kUnits / 4), jq = (v % (kUnits / 4)) * 4;
        Ws[(jq + 0) * kPitch + kr] = rw[i].x;
        Ws[(jq + 1) * kPitch + kr] = rw[i].y;
        Ws[(jq + 2) * kPitch + kr] = rw[i].z;
        Ws[(jq + 3) * kPitch + kr] = rw[i].w;
      }
    };
    const int nk = 3 * H / kBK;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) load((kt + 1) * kBK);
      const float* As = smem + cur * (kRows + kUnits) * kPitch;
      const float* Ws = As + kRows * kPitch;
#pragma unroll
      for (int kb = 0; kb < kBK; kb += 16) {
        const v4f av = ld4(As + (wave * 16 + lr) * kPitch + kb + 4 * lq);
        const v4f wv = ld4(Ws + lr * kPitch + kb + 4 * lq);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv.x, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv.y, acc[1], 0, 0, 0);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv.z, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv.w, acc[1], 0, 0, 0);
      }
      asm volatile("" ::: "memory");      // keep the stage-k+1 LDS store (and its vmcnt wait)
      __builtin_amdgcn_sched_barrier(0);   // after this stage's MFMAs
      if (kt + 1 < nk) store(cur ^ 1);
      __syncthreads();
    }
  }

  const int j = j0 + lr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + wave * 16 + lq * 4 + r;
    if (b >= B) continue;
    float* dhz = a.dhz + ((size_t)dir * B + b) * H + j;
    float dh = a.dy[((size_t)b * T + t) * 2 * H + dir * H + j];
    if (step > 0) dh += (acc[0][r] + acc[1][r]) + *dhz;
    const float* gs = a.gates + (((size_t)dir * T + t) * B + b) * 4 * H;
    const float rg = gs[j], zg = gs[H + j], ng = gs[2 * H + j], ghn = gs[3 * H + j];
    const float hp = edge ? 0.f : a.y_in[((size_t)b * T + tprev) * 2 * H + dir * H + j];
    const float dn = dh * (1.0f - zg);
    const float daz = dh * (hp - ng) * zg * (1.0f - zg);
    const float dan = dn * (1.0f - ng * ng);
    const float dar = dan * ghn * rg * (1.0f - rg);
    float* dgi = a.dgi + ((size_t)b * T + t) * 6 * H + dir * 3 * H;
    dgi[j] = dar;
    dgi[H + j] = daz;
    dgi[2 * H + j] = dan;
    float* dg = edge ? a.dgh_edge + ((size_t)dir * B + b) * 3 * H
                     : a.dgh + (((size_t)dir * B + b) * T + t) * 3 * H;
    dg[j] = dar;
    dg[H + j] = daz;
    dg[2 * H + j] = dan * rg;
    if (edge) {   // keep the h_prev = 0 row out of the dW_hh GEMM (see layer_bwd)
      float* z0 = a.dgh + (((size_t)dir * B + b) * T + t) * 3 * H;
      z0[j] = 0.f; z0[H + j] = 0.f; z0[2 * H + j] = 0.f;
    }
    *dhz = dh * zg;
  }
}

// ------------------------------------------------------------------ last-step top layer (srk_gru_top_last_*)
// A top layer whose consumer reads row T-1 of y only (fc(last_step(gru(x)[0])), model_mfcc_bgru.py:43-44).
// y_last[b][:] = y[b][T-1][:]  (C = 2H)
__global__ void gather_last_kernel(const float* __restrict__ y, int64_t B, int T, int C, float* __restrict__ y_last) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * C) return;
  const int64_t b = i / C;
  y_last[i] = y[(b * T + T - 1) * C + (i - b * C)];
}
// dy[b][t][:] = t == T - 1 ? dy_last[b][:] : 0: the [B][T][2H] gradient the backward recurrence reads (4 | C)
__global__ void pad_last_kernel(const float* __restrict__ dy_last, int64_t B, int T, int C, float* __restrict__ dy) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c4 = C / 4;
  if (i >= B * T * c4) return;
  const int64_t row = i / c4, b = row / T;
  const int c = (int)(i - row * c4) * 4;
  v4f v = v4f{0.f, 0.f, 0.f, 0.f};
  if (row - b * T == T - 1) {
    const float* s = dy_last + b * C + c;
    v = v4f{s[0], s[1], s[2], s[3]};
  }
  st4(dy + i * 4, v);
}
// X[r][c0 .. c0 + cols) = 0 for r < rows (4 | cols, c0, ld): the reverse direction's dgi columns, which the
// forward-only backward recurrence leaves unwritten, ahead of GEMMs that read whole rows
__global__ void zero_cols_kernel(float* __restrict__ X, int64_t rows, int cols, int c0, int ld) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, c4 = cols / 4;
  if (i >= rows * c4) return;
  const int64_t r = i / c4;
  st4(X + r * ld + c0 + (i - r * c4) * 4, v4f{0.f, 0.f, 0.f, 0.f});
}
// The reverse direction's row T-1 is its FIRST step: one cell from h = 0, so gh = b_hh and h = (1 - z) n (the
// arithmetic of the persistent kernels' step 0, cell functions included: FAST as gru_fp32_fast_cell()).  Reads
// gi[(b, T-1)][3H:6H]; writes y[b][T-1][H:2H], the whole y_last row (its forward half copied from y) and the saved
// gates of (dir 1, t = T-1) unit-interleaved (store_gates_il's layout), as the backward reads them.
template <bool FAST>
__global__ void rev_cell_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ b_hh, int64_t B, int T,
                                    int H, float* __restrict__ y, float* __restrict__ y_last,
                                    float* __restrict__ gates) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * H) return;
  const int64_t b = i / H, row = b * T + T - 1;
  const int j = (int)(i - b * H);
  const float* g = gi + row * 6 * H + 3 * H;
  const float bhr = b_hh[3 * H + j], bhz = b_hh[4 * H + j], ghn = b_hh[5 * H + j];
  float rg, zg, ng;
  if (FAST) {
    rg = sigmoid_fast(g[j] + bhr);
    zg = sigmoid_fast(g[H + j] + bhz);
    ng = tanh_fast(g[2 * H + j] + rg * ghn);
  } else {
    rg = sigmoidf_(g[j] + bhr);
    zg = sigmoidf_(g[H + j] + bhz);
    ng = tanhf(g[2 * H + j] + rg * ghn);
  }
  const float h = (1.0f - zg) * ng;
  y[row * 2 * H + H + j] = h;
  y_last[b * 2 * H + H + j] = h;
  y_last[b * 2 * H + j] = y[row * 2 * H + j];
  st4(gates + (((int64_t)T + T - 1) * B + b) * 4 * H + 4 * j, v4f{rg, zg, ng, ghn});
}
// Its backward: the cell derivatives at h_prev = 0 from dy_last[:, H:], written where the full backward recurrence
// leaves them: dgi[(b, T-1)][3H:6H] = (dar, daz, dan) and dgh_edge[1][b] = (dar, daz, dan r).
__global__ void rev_cell_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ dy_last, int64_t B, int T,
                                    int H, float* __restrict__ dgi, float* __restrict__ dgh_edge) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * H) return;
  const int64_t b = i / H;
  const int j = (int)(i - b * H);
  const v4f gv = ld4(gates + (((int64_t)T + T - 1) * B + b) * 4 * H + 4 * j);
  const float rg = gv.x, zg = gv.y, ng = gv.z, ghn = gv.w;
  const float dh = dy_last[b * 2 * H + H + j];
  const float dn = dh * (1.0f - zg);
  const float daz = dh * (0.f - ng) * zg * (1.0f - zg);
  const float dan = dn * (1.0f - ng * ng);
  const float dar = dan * ghn * rg * (1.0f - rg);
  float* d = dgi + (b * T + T - 1) * 6 * H + 3 * H;
  d[j] = dar;
  d[H + j] = daz;
  d[2 * H + j] = dan;
  float* e = dgh_edge + (B + b) * 3 * H;
  e[j] = dar;
  e[H + j] = daz;
  e[2 * H + j] = dan * rg;
}

int check_dims(int64_t B, int64_t T, int64_t in, int64_t H) {
  SRK_REQUIRE(B > 0 && T > 0 && in > 0 && H > 0, SRK_ERR_INVALID, "gru: dims must be positive");
  SRK_REQUIRE(H % kBK == 0, SRK_ERR_INVALID, "gru: hidden size must be a multiple of 128");
  SRK_REQUIRE(B * T * 6 * H < ((int64_t)1 << 40), SRK_ERR_INVALID, "gru: problem too large");
  return SRK_OK;
}

// Input widths that are not a multiple of 4 (the 39 MFCC features of model_mfcc_bgru.py:25):
// the input-projection GEMMs run on a copy of x / W_ih padded with zero columns to a multiple of
// 4, so they take the 16-B vector (and LDS-DMA / buffer-load) paths; a zero column adds exact
// zeros to every dot product.  dW_ih is produced at the padded width and its first `in` columns
// are written (or added) into the caller's tensor.
__global__ void pad_cols_kernel(const float* __restrict__ src, int64_t rows, int cols, float* __restrict__ dst,
                                int colsp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * colsp) return;
  const int64_t r = i / colsp;
  const int c = (int)(i - r * colsp);
  dst[i] = c < cols ? src[r * cols + c] : 0.f;
}
__global__ void unpad_cols_kernel(const float* __restrict__ src, int64_t rows, int colsp, float* __restrict__ dst,
                                  int cols, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * cols) return;
  const int64_t r = i / cols;
  const int c = (int)(i - r * cols);
  const float v = src[r * colsp + c];
  dst[i] = accumulate ? dst[i] + v : v;
}
// bf16 / fp16 mode: fp32 [rows][cols] -> 16-bit [rows][colsp] (zero columns past cols), rounded to
// nearest-even — the GEMM operands of the layer that are not produced by the recurrence kernels.
template <bool F16>
__global__ void to16_kernel(const float* __restrict__ src, int64_t rows, int cols, uint16_t* __restrict__ dst,
                            int colsp) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * colsp) return;
  const int64_t r = i / colsp;
  const int c = (int)(i - r * colsp);
  const float v = c < cols ? src[r * cols + c] : 0.f;
  if (F16) {
    const _Float16 h = (_Float16)v;
    dst[i] = __builtin_bit_cast(uint16_t, h);
  } else {
    const __bf16 h = (__bf16)v;
    dst[i] = __builtin_bit_cast(uint16_t, h);
  }
}
// Dense case (no column padding, 8 | n, 16-B aligned): 8 elements per thread, two 16-B loads and one
// 16-B store, no index division.
template <bool F16>
__global__ void to16_vec8_kernel(const float* __restrict__ src, int64_t n8, uint16_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef unsigned u4 __attribute__((ext_vector_type(4)));
  typedef __attribute__((ext_vector_type(8))) typename std::conditional<F16, _Float16, __bf16>::type e8;
  const f4 a = *reinterpret_cast<const f4*>(src + 8 * i), b = *reinterpret_cast<const f4*>(src + 8 * i + 4);
  const e8 h = __builtin_convertvector((__attribute__((ext_vector_type(8))) float){a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}, e8);
  *reinterpret_cast<u4*>(dst + 8 * i) = __builtin_bit_cast(u4, h);
}

// The launch of this file's elementwise kernels: one thread per element (or vector) of n, 256-thread blocks.
template <class... P, class... A>
int launch256(void (*kernel)(P...), int64_t n, hipStream_t s, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, static_cast<P>(args)...);
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
}

int to16(const float* src, int64_t rows, int64_t cols, uint16_t* dst, int64_t colsp, hipStream_t s) {
  const int64_t n = rows * colsp;
  const bool f16 = matmul_prec() == kPrecF16;
  if (cols == colsp && n % 8 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0)
    return launch256(f16 ? to16_vec8_kernel<true> : to16_vec8_kernel<false>, n / 8, s, src, n / 8, dst);
  return launch256(f16 ? to16_kernel<true> : to16_kernel<false>, n, s, src, rows, cols, dst, colsp);
}
// Bias gradients from the 16-bit backward kernel's partials [part][2 dir][4][H] (sums of dar, daz,
// dan, dan * r), summed over the valid (chunk, group) parts in order: db_ih = (dar, daz, dan),
// db_hh = (dar, daz, dan * r); `accumulate` adds into the caller's tensors.
__device__ __forceinline__ void dbias_reduce_at(int i, const float* __restrict__ part, int nparts, int B, int H,
                                                int rows_per_part, float* __restrict__ db_ih,
                                                float* __restrict__ db_hh, int accumulate) {
  if (i >= 2 * 3 * H) return;   // i over [2 dir][3][H]
  const int dir = i / (3 * H), g = (i / H) % 3, j = i % H;
  const int per_chunk = 256 / rows_per_part;
  float si = 0.f, sh = 0.f;
  for (int p = 0; p < nparts; ++p) {
    if ((p / per_chunk) * 256 + (p % per_chunk) * rows_per_part >= B) continue;   // (chunk, group) without rows
    const float* q = part + ((size_t)p * 2 + dir) * 4 * H;
    si += q[g * H + j];
    sh += q[(g == 2 ? 3 : g) * H + j];
  }
  db_ih[i] = accumulate ? db_ih[i] + si : si;
  db_hh[i] = accumulate ? db_hh[i] + sh : sh;
}
__global__ void dbias_reduce_kernel(const float* __restrict__ part, int nparts, int B, int H, int rows_per_part,
                                    float* __restrict__ db_ih, float* __restrict__ db_hh, int accumulate) {
  dbias_reduce_at(blockIdx.x * blockDim.x + threadIdx.x, part, nparts, B, H, rows_per_part, db_ih, db_hh, accumulate);
}

// Both reductions of the fused 16-bit backward in one launch.  Blocks [0, dw_blocks): dW_hh[dir] (+)= sum
// over the partials [part][2 dir][3H][H] in part order (deterministic), 4 consecutive columns per thread
// (part p = chunk * 8 + group covers batch rows 256 chunk + 32 group ..; parts past the batch were never
// written and are skipped).  The rest: the bias gradients, as dbias_reduce_kernel.
__global__ void dwhh_dbias_reduce_kernel(const float* __restrict__ part, int nparts, int B, int64_t per_dir,
                                         float* __restrict__ dw, int accumulate, int dw_blocks,
                                         const float* __restrict__ bpart, int bparts, int H, int rows_per_part,
                                         float* __restrict__ db_ih, float* __restrict__ db_hh) {
  if ((int)blockIdx.x >= dw_blocks) {
    dbias_reduce_at(((int)blockIdx.x - dw_blocks) * blockDim.x + threadIdx.x, bpart, bparts, B, H, rows_per_part,
                    db_ih, db_hh, accumulate);
    return;
  }
  const int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i4 * 4 >= 2 * per_dir) return;
  const int64_t o = i4 * 4, dir = o / per_dir, e = o - dir * per_dir;
  v4f acc = accumulate ? *reinterpret_cast<const v4f*>(dw + o) : v4f{0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < nparts; ++p) {
    if ((p / 8) * 256 + (p % 8) * 32 >= B) continue;
    acc += *reinterpret_cast<const v4f*>(part + ((size_t)p * 2 + dir) * per_dir + e);
  }
  *reinterpret_cast<v4f*>(dw + o) = acc;
}

// grow-only scratch of the fused backward's dW_hh partials (graph-safe: bumps g_scratch_gen on growth)
ScratchPool g_gs;

inline int64_t pad4(int64_t v) { return (v + 3) / 4 * 4; }
inline bool padded_in(int64_t in) { return in % 4 != 0; }
int pad_cols(const float* src, int64_t rows, int64_t cols, float* dst, hipStream_t s) {
  return launch256(pad_cols_kernel, rows * pad4(cols), s, src, rows, cols, dst, pad4(cols));
}

}  // namespace
}  // namespace srk

using srk::GemmDesc;

namespace {

int64_t up64(int64_t v) { return (v + 63) / 64 * 64; }
int64_t in8_of(int64_t in) { return (in + 7) / 8 * 8; }

// THE layout of a layer's forward or backward workspace: every member's offset in floats, built once per call.
// Blocks start 64-float aligned; the backward finds the forward's saved members with the forward's GruWs.
struct GruWs {
  // forward: gi [B*T][6H] | gates [2][T][B][4H] (r, z, n, W_hn h + b_hn; kept for the backward)
  int64_t gi = 0, gates = 0;
  // backward: dgi [B*T][6H] | dgh [2][B][T][3H] | dgh_edge [2][B][3H] | dhz [2][B][H]; on the 16-bit path dgi16
  // [B*T][6H] (at dgi) and dgh16 [2][B][T][3H] alias the fp32 dgi region, unused in that mode
  int64_t dgi = 0, dgh = 0, dgh_edge = 0, dhz = 0, dgh16 = 0;
  // the persistent kernels' hand-off ring in MFMA-fragment order (fwd: h [2 dir][kHandoffSlots][rows][H], bwd: dg
  // [2 dir][kHandoffSlots][rows][3H]; rows = the 64-row groups of one launch chunk: <= 512, or B rounded up to 64),
  // then their kCounterFloats step-ordering words (gru_persistent.hip)
  int64_t xbuf = 0, counters = 0;
  // for an input width that is no multiple of 4 (srk::padded_in), at width in4:
  //   fwd: x padded [B*T][in4] (kept for the backward's dW_ih) | W_ih padded [6H][in4]
  //   bwd: W_ih padded [6H][in4] | dW_ih padded [6H][in4] | dx padded [B*T][in4]
  int64_t xpad = 0, wpad = 0, dwpad = 0, dxpad = 0;
  // H == 512, the block of the 16-bit path (GruPath::h16), at width in8:
  //   fwd: x16 [B*T][in8] | W_ih16 [6H][in8] | y16 [B*T][2H]       (16-bit elements, kept for the backward)
  //   bwd: bias partials [8 * chunks][2][4][H] | dW_ih [6H][in8] | dx [B*T][in8]   (fp32; the last two are only
  //        there when in8 != in)
  int64_t x16 = 0, w16 = 0, y16 = 0;
  int64_t part = 0, dwpad8 = 0, dxpad8 = 0;
  int64_t total = 0;       // srk_gru_workspace_floats
  int64_t dy = 0;          // srk_gru_top_last_bwd: the [B][T][2H] gradient behind the layer's workspace
  int64_t top_total = 0;   // srk_gru_top_last_workspace_floats
};

GruWs gru_ws(int64_t B, int64_t T, int64_t in, int64_t H, bool backward) {
  GruWs w;
  const int64_t BT = B * T, in4 = srk::pad4(in), in8 = in8_of(in);
  const int64_t ring = srk::kHandoffSlots * std::min<int64_t>(up64(B), 512) * H;
  if (!backward) {
    w.gates = BT * 6 * H;
    w.xbuf = up64(w.gates + 2 * T * B * 4 * H);
    w.counters = w.xbuf + 2 * ring;
  } else {
    w.dgh = BT * 6 * H;
    w.dgh16 = BT * 6 * H / 2;
    w.dgh_edge = w.dgh + 2 * BT * 3 * H;
    w.dhz = w.dgh_edge + 2 * B * 3 * H;
    w.xbuf = up64(w.dhz + 2 * B * H);
    w.counters = w.xbuf + 6 * ring;
  }
  const int64_t pad = up64(w.counters + srk::kCounterFloats);
  int64_t e = pad + 64;
  if (srk::padded_in(in)) {
    if (!backward) {
      w.xpad = pad;
      w.wpad = w.xpad + BT * in4;
    } else {
      w.wpad = pad;
      w.dwpad = w.wpad + 6 * H * in4;
      w.dxpad = w.dwpad + 6 * H * in4;
    }
    e += BT * in4 + (backward ? 2 : 1) * 6 * H * in4 + 64;
  }
  w.total = e = up64(e);
  if (H == 512 && !backward) {
    w.x16 = e;
    w.w16 = w.x16 + up64(BT * in8 / 2 + 1);
    w.y16 = w.w16 + up64(6 * H * in8 / 2 + 1);
    w.total = w.y16 + up64(BT * 2 * H / 2 + 1) + 64;
  } else if (H == 512) {
    w.part = e;
    w.dwpad8 = w.part + up64((B + 255) / 256 * 8 * 2 * 4 * H);   // <= 8 partials per 256-row chunk
    w.dxpad8 = w.dwpad8 + up64(6 * H * in8);
    w.total = (in8 != in ? w.dxpad8 + up64(BT * in8) : w.dwpad8) + 64;
  }
  w.dy = w.total;
  w.top_total = w.total + (backward ? up64(BT * 2 * H) : 0);
  return w;
}

// How one entry-point call runs its layer, decided once: the recurrence plan of each direction of travel and the
// path they put the layer on.
struct GruPath {
  srk::GruRecPlan fwd, bwd;
  // both directions of travel on the persistent kernels, or neither (they hand the saved gates over
  // unit-interleaved, the per-step kernels in the plain layout)
  bool persistent = false;
  // the 16-bit path: a 16-bit precision, the persistent kernels, and 32-bit byte offsets for the 16-bit operands
  // in memory (x16 / W16 / y16, dgi16 / dgh16); every GEMM of the layer reads those
  bool h16 = false;
  // srk_gru_top_last_*: modes 1 .. 3 (option gru_top_last) exist on the fp32 persistent path only (top_last_ok);
  // everywhere else 0 = the full layer, exactly what srk_gru_layer_* compute
  bool top_last_ok = false;
  int top_last = 0;
};

GruPath gru_path(int64_t B, int64_t T, int64_t in, int64_t H) {
  GruPath p;
  const int prec = srk::matmul_prec();
  const srk::GruOpts o = srk::gru_opts();
  const bool out16 = prec != srk::kPrecF32 && (double)B * T * 6 * H * 2 < 2147483647.0 &&
                     (double)B * T * in8_of(in) * 2 < 2147483647.0;
  // (a persistent forward projects an input of in <= kFusedIn itself)
  p.fwd = srk::gru_rec_plan(B, T, H, in <= srk::kFusedIn ? (int)in : 0, prec, false, out16, o, srk::gru_fit_measured);
  p.bwd = srk::gru_rec_plan(B, T, H, 0, prec, true, out16, o, srk::gru_fit_measured);
  p.persistent = p.fwd.variant != srk::kGruStep && p.bwd.variant != srk::kGruStep;
  p.h16 = p.persistent && out16;
  p.top_last_ok = prec == srk::kPrecF32 && H == 512 && p.persistent;
  p.top_last = p.top_last_ok ? srk::g_opt_gru_top_last : 0;
  return p;
}

// The GruPArgs fields every persistent launch of a layer sets: dims, recurrent weights, hand-off ring, counters.
srk::GruPArgs rec_args(int64_t B, int64_t T, int64_t H, const float* w_hh, float* ws, const GruWs& L) {
  srk::GruPArgs p{};
  p.B = (int)B; p.T = (int)T; p.H = (int)H;
  p.w_hh = w_hh;
  p.xbuf = ws + L.xbuf;
  p.counters = reinterpret_cast<unsigned*>(ws + L.counters);
  return p;
}

inline uint16_t* u16(float* p) { return reinterpret_cast<uint16_t*>(p); }
inline const uint16_t* u16(const float* p) { return reinterpret_cast<const uint16_t*>(p); }

}  // namespace

extern "C" {

int64_t srk_gru_workspace_floats(int64_t B, int64_t T, int64_t in, int64_t H, int backward) {
  return gru_ws(B, T, in, H, backward != 0).total;
}

int srk_gru_layer_fwd(const float* x, int64_t B, int64_t T, int64_t in, int64_t H, const float* w_ih,
                      const float* w_hh, const float* b_ih, const float* b_hh, float* y, float* ws, void* stream) {
  return srk_gru_layer_fwd_x16(x, nullptr, B, T, in, H, w_ih, w_hh, b_ih, b_hh, y, ws, stream);
}

int64_t srk_gru_y16_offset(int64_t B, int64_t T, int64_t in, int64_t H) {
  if (srk::check_dims(B, T, in, H) || H != 512 || !gru_path(B, T, in, H).h16) return -1;
  return gru_ws(B, T, in, H, false).y16;
}

// One layer forward.  top_last >= 2 (GruPath::top_last, with y_last): only row T-1 of y is used, so the reverse
// direction is its one cell at t = T-1 (rev_cell_fwd_kernel) and its rows t < T-1 of gi / y / the gates are never
// written.
static int layer_fwd(const float* x, const void* x16_in, int64_t B, int64_t T, int64_t in, int64_t H,
                     const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* y,
                     float* ws, const GruPath& path, int top_last, float* y_last, hipStream_t s) {
  const bool rev_cell = top_last >= 2;
  SRK_REQUIRE(!rev_cell || (path.persistent && !path.h16 && y_last), SRK_ERR_INTERNAL,
              "gru_fwd: rev_cell off the fp32 persistent path");
  const GruWs L = gru_ws(B, T, in, H, false);
  const int64_t BT = B * T;
  float* gi = ws + L.gi;
  float* gates = ws + L.gates;
  uint16_t* y16 = nullptr;
  const bool fuse = path.persistent && in <= srk::kFusedIn;   // the kernel projects the input itself (no gi GEMM)
  if (path.h16) {   // 16-bit operands in memory: x, W_ih rounded once, h written by the kernel
    const int64_t in8 = in8_of(in);
    uint16_t* x16 = u16(ws + L.x16);
    uint16_t* w16 = u16(ws + L.w16);
    y16 = u16(ws + L.y16);
    // x16_in: the producer's copy of x (the previous layer's y16), used as it is: in == in8 only
    SRK_REQUIRE(!x16_in || (in8 == in && reinterpret_cast<uintptr_t>(x16_in) % 16 == 0), SRK_ERR_INVALID,
                "gru_fwd: a ready 16-bit x needs in % 8 == 0 and 16-B alignment");
    if (x16_in) x16 = const_cast<uint16_t*>(static_cast<const uint16_t*>(x16_in));
    else if (int rc = srk::to16(x, BT, in, x16, in8, s)) return rc;
    // W16: the gi GEMM's operand; with the fused projection only the backward's dx needs it (rounded there)
    if (!fuse) {
      if (int rc = srk::to16(w_ih, 6 * H, in, w16, in8, s)) return rc;
      GemmDesc g;   // gi[B*T, 6H] = x16 * W16^T + b_ih
      g.M = BT; g.N = 6 * H; g.K = in8;
      g.A16 = x16; g.lda = in8;
      g.B16 = w16; g.ldb = in8; g.tb = true;
      g.C = gi; g.ldc = 6 * H;
      g.bias = b_ih; g.bias_mode = 1;
      if (int rc = srk::gemm_f32(g, s)) return rc;
    }
  } else {
    const float* xa = x;
    const float* wa = w_ih;
    const int64_t ink = srk::pad4(in);
    if (srk::padded_in(in)) {   // zero-pad the input width to a multiple of 4 (vector GEMM paths)
      if (int rc = srk::pad_cols(x, BT, in, ws + L.xpad, s)) return rc;
      if (int rc = srk::pad_cols(w_ih, 6 * H, in, ws + L.wpad, s)) return rc;
      xa = ws + L.xpad;
      wa = ws + L.wpad;
    }
    if (!fuse) {
      // gi[B*T, 6H] = x[B*T, in] * W_ih_cat[6H, in]^T + b_ih_cat (rev_cell: the forward direction's 3H columns)
      GemmDesc g;
      g.M = BT; g.N = rev_cell ? 3 * H : 6 * H; g.K = ink;
      g.A = xa; g.lda = ink;
      g.B = wa; g.ldb = ink; g.tb = true;
      g.C = gi; g.ldc = 6 * H;
      g.bias = b_ih; g.bias_mode = 1;
      if (top_last == 3) {   // the K split of the full projection: its bits at every shape
        GemmDesc full = g;
        full.N = 6 * H;
        srk::gemm_f32_pin_as(full, g);
      }
      if (int rc = srk::gemm_f32(g, s)) return rc;
    }
    if (rev_cell) {
      // gi[(b, T-1)][3H:6H] = x[b, T-1, :] * W_ih[1]^T + b_ih[1]: B strided rows, where the full GEMM puts them
      GemmDesc g;
      g.M = B; g.N = 3 * H; g.K = ink;
      g.A = xa + (T - 1) * ink; g.lda = T * ink;
      g.B = wa + 3 * H * ink; g.ldb = ink; g.tb = true;
      g.C = gi + (T - 1) * 6 * H + 3 * H; g.ldc = T * 6 * H;
      g.bias = b_ih + 3 * H; g.bias_mode = 1;
      if (top_last == 3) {   // mode 3: the full projection's sum order, its K split included; unsplit failing that
        GemmDesc full;
        full.M = BT; full.N = 6 * H; full.K = ink;
        full.A = xa; full.lda = ink;
        full.B = wa; full.ldb = ink; full.tb = true;
        full.C = gi; full.ldc = 6 * H;
        full.bias = b_ih; full.bias_mode = 1;
        if (!srk::gemm_f32_pin_as(full, g)) g.no_split = true;
      }
      if (int rc = srk::gemm_f32(g, s)) return rc;
    }
  }
  if (path.persistent) {
    srk::GruPArgs p = rec_args(B, T, H, w_hh, ws, L);
    p.gi = gi; p.b_hh = b_hh; p.y = y; p.gates = gates; p.y16 = y16;
    if (fuse) { p.x_in = x; p.w_ih = w_ih; p.b_ih = b_ih; p.in = (int)in; }
    p.one_dir = rev_cell ? 1 : 0;
    if (int rc = srk::gru_persistent_launch(p, path.fwd, false, s)) return rc;
    if (rev_cell)   // after the recurrence: y_last's forward half is its last step
      return srk::launch256(path.fwd.fast_cell ? srk::rev_cell_fwd_kernel<true> : srk::rev_cell_fwd_kernel<false>,
                            B * H, s, gi, b_hh, B, T, H, y, y_last, gates);
    return SRK_OK;
  }
  srk::GruArgs a{};
  a.B = (int)B; a.T = (int)T; a.H = (int)H; a.in = (int)in;
  a.y_in = y; a.y = y; a.gi = gi; a.w_hh = w_hh; a.b_hh = b_hh; a.gates = gates;
  a.G = (int)((B + srk::kRows - 1) / srk::kRows);
  a.S = (int)(H / srk::kUnits);
  const dim3 grid((unsigned)(2 * a.G * a.S));
  for (int step = 0; step < T; ++step) {
    srk::ProfScope prof("gru_fwd_step", s, step > 0 ? 2.0 * 2.0 * (double)B * 3 * H * H : 0.0);   // 2 dirs x [B,H]x[H,3H]
    hipLaunchKernelGGL(srk::gru_fwd_step_kernel, grid, dim3(256), 0, s, a, step);
  }
  SRK_CHECK_HIP(hipGetLastError());
  return SRK_OK;
}

int srk_gru_layer_fwd_x16(const float* x, const void* x16_in, int64_t B, int64_t T, int64_t in, int64_t H,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* y,
                          float* ws, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_dims(B, T, in, H)) return rc;
  SRK_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && y && ws, SRK_ERR_INVALID, "gru_fwd: null pointer");
  return layer_fwd(x, x16_in, B, T, in, H, w_ih, w_hh, b_ih, b_hh, y, ws, gru_path(B, T, in, H), 0, nullptr,
                   srk::as_stream(stream));
  SRK_API_END
}

int64_t srk_gru_top_last_workspace_floats(int64_t B, int64_t T, int64_t in, int64_t H, int backward) {
  return gru_ws(B, T, in, H, backward != 0).top_total;
}

int srk_gru_top_last_fwd(const float* x, const void* x16_in, int64_t B, int64_t T, int64_t in, int64_t H,
                         const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* y,
                         float* y_last, float* ws, int* mode, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_dims(B, T, in, H)) return rc;
  SRK_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && y && y_last && ws && mode, SRK_ERR_INVALID,
              "gru_top_last_fwd: null pointer");
  hipStream_t s = srk::as_stream(stream);
  const GruPath path = gru_path(B, T, in, H);
  *mode = path.top_last;
  if (int rc = layer_fwd(x, x16_in, B, T, in, H, w_ih, w_hh, b_ih, b_hh, y, ws, path, *mode, y_last, s)) return rc;
  if (*mode < 2)   // modes 0 and 1 ran the full layer: y_last is its row T-1
    return srk::launch256(srk::gather_last_kernel, B * 2 * H, s, y, B, T, 2 * H, y_last);
  return SRK_OK;
  SRK_API_END
}

int srk_gru_layer_bwd(const float* x, int64_t B, int64_t T, int64_t in, int64_t H, const float* w_ih,
                      const float* w_hh, const float* y, const float* ws_fwd, const float* dy, float* dx,
                      float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int accumulate, float* ws,
                      void* stream) {
  return srk_gru_layer_bwd_x16(x, nullptr, B, T, in, H, w_ih, w_hh, y, ws_fwd, dy, dx, dw_ih, dw_hh, db_ih, db_hh,
                               accumulate, ws, stream);
}

// One layer backward.  top_last (srk_gru_top_last_bwd, the forward's top_last_mode): dy is zero but for its rows
// (b, T-1) = dy_last, so after the recurrence the reverse direction's dgi is zero but for those B rows, its dgh is
// zero everywhere (the live step has h_prev = 0: its dgh sits in dgh_edge[1]) and dW_hh[1] = 0.  Modes 1 and 2 issue
// only the GEMM work that is not identically zero; modes 2 and 3 replace the reverse recurrence by its one cell
// (rev_cell_bwd_kernel), leaving dgh[1] (and in mode 2 the reverse dgi rows t < T-1) unwritten and unread.  Mode 3
// zero-fills those dgi rows and keeps the full dW_ih / dx GEMMs: every result then has the full layer's bits (the
// grouped dW launch and the clipped dx below keep those bits without reading the zeros, and then the fill goes).
static int layer_bwd(const float* x, const void* x16_in, int64_t B, int64_t T, int64_t in, int64_t H,
                     const float* w_ih, const float* w_hh, const float* y, const float* ws_fwd, const float* dy,
                     const float* dy_last, const GruPath& path, int top_last, float* dx, float* dw_ih, float* dw_hh,
                     float* db_ih, float* db_hh, int accumulate, float* ws, hipStream_t s) {
  SRK_REQUIRE(!top_last || (path.persistent && !path.h16 && dy_last), SRK_ERR_INTERNAL,
              "gru_bwd: top_last off the fp32 persistent path");
  const int64_t BT = B * T;
  const GruWs L = gru_ws(B, T, in, H, true), F = gru_ws(B, T, in, H, false);   // F: the forward's, inside ws_fwd
  const bool h16 = path.h16;
  float* dgi = ws + L.dgi;
  float* dgh = ws + L.dgh;
  float* dgh_edge = ws + L.dgh_edge;
  float* gates = const_cast<float*>(ws_fwd + F.gates);
  // The operand set of the layer's GEMMs: fp32 at width in4, or (16-bit path) 16-bit at width in8 — dgi16 / dgh16
  // from the kernel, x16 / W16 / y16 from the forward (x16_in: its ready copy, srk_gru_layer_fwd_x16).  pad: dW_ih
  // and dx come out at that width in a pad buffer and their first `in` columns go to the caller's tensors.
  struct Mat {
    const float* f;
    const uint16_t* h;
    Mat at(int64_t off) const { return {f ? f + off : nullptr, h ? h + off : nullptr}; }
  };
  const auto set_a = [](GemmDesc& g, Mat m) { g.A = m.f; g.A16 = m.h; };
  const auto set_b = [](GemmDesc& g, Mat m) { g.B = m.f; g.B16 = m.h; };
  const int64_t ld = h16 ? in8_of(in) : srk::pad4(in);
  const bool pad = ld != in;
  float* wpad = pad && !h16 ? ws + L.wpad : nullptr;                // fp32: [6H][in4]
  float* dwpad = pad ? ws + (h16 ? L.dwpad8 : L.dwpad) : nullptr;   // [6H][ld]
  float* dxpad = pad ? ws + (h16 ? L.dxpad8 : L.dxpad) : nullptr;   // [BT][ld]
  Mat m_dgi{dgi, nullptr}, m_dgh{dgh, nullptr}, m_x{pad ? ws_fwd + F.xpad : x, nullptr},
      m_w{pad ? wpad : w_ih, nullptr}, m_y{y, nullptr};
  if (h16) {
    m_dgi = {nullptr, u16(ws + L.dgi)};
    m_dgh = {nullptr, u16(ws + L.dgh16)};
    m_x = {nullptr, x16_in ? static_cast<const uint16_t*>(x16_in) : u16(ws_fwd + F.x16)};
    m_w = {nullptr, u16(ws_fwd + F.w16)};   // (rounded below where the fused-projection forward left it unwritten)
    m_y = {nullptr, u16(ws_fwd + F.y16)};
  }
  int rc;
  const float beta = accumulate ? 1.f : 0.f;   // autograd .grad accumulation in the GEMM epilogues
  // Mode 3, decided before the recurrence (its zero fill depends on both).  Grouped (last-step
  // top layer): the full dW_ih GEMM multiplies the reverse half's BT - B zero rows, and the forward dW_hh planned
  // as the two-direction launch fills half of the CUs.  Both keep their bits as parts: the dW_ih forward half on the
  // full GEMM's kernel and K split, the reverse half with its all-zero 8-deep k blocks deleted slab by slab
  // (PackPlan), the dW_hh as before; the three share one launch.  dx_klive: the full dx GEMM, stream-K, without the
  // K-tiles of the reverse half (gemm_f32_klive), its B live rows (b, T-1) completed over the full K.
  bool grouped = false;
  GemmDesc full, hh;   // the one dW_ih GEMM of the ungrouped path | the two-direction dW_hh launch
  srk::PackPlan pp;
  if (top_last == 3 && !h16 && T >= 16 && srk::gemm_group_enabled()) {
    full.M = 6 * H; full.N = ld; full.K = BT;
    full.A = dgi; full.lda = 6 * H; full.ta = true;
    full.B = m_x.f; full.ldb = ld;
    full.C = pad ? dwpad : dw_ih; full.ldc = ld; full.beta = pad ? 0.f : beta;
    full.rowsum = db_ih; full.rowsum_beta = beta;
    hh.M = 3 * H; hh.N = H; hh.K = BT - 1;
    hh.ta = true; hh.lda = 3 * H; hh.ldb = 2 * H;
    hh.A = dgh + 3 * H; hh.B = y;
    hh.C = dw_hh; hh.ldc = H; hh.beta = beta;
    hh.batch = 2; hh.sA = BT * 3 * H - 3 * H; hh.sB = 3 * H; hh.sC = 3 * H * H;
    hh.rowsum = db_hh; hh.rowsum_beta = beta; hh.sRS = 3 * H;
    int splits = 0;
    int64_t kchunk = 0;
    grouped = srk::gemm_f32_p32_split(full, &splits, &kchunk) && splits > 1 && srk::g_opt_gru_dwhh_batched &&
              srk::gemm_f32_batched_rowsum_ok(hh) && srk::pack_plan(BT, kchunk, T - 1, T, B, pp) == SRK_OK &&
              pp.nslabs == splits;
  }
  GemmDesc gdx;   // dx[BT, in] = dgi[BT, 6H] * W_ih_cat[6H, in]
  gdx.M = BT; gdx.N = ld; gdx.K = (top_last == 1 || top_last == 2) ? 3 * H : 6 * H;
  set_a(gdx, m_dgi); gdx.lda = 6 * H;
  set_b(gdx, m_w); gdx.ldb = ld;
  gdx.C = pad ? dxpad : dx; gdx.ldc = ld;
  bool dx_klive = false;
  if (dx && top_last == 3 && !h16 && srk::gemm_klive_enabled()) {
    gdx.k_live = 3 * H; gdx.live_first = T - 1; gdx.live_stride = T; gdx.live_count = B;
    dx_klive = srk::gemm_f32_klive_ok(gdx);
    if (!dx_klive) gdx.k_live = 0;
  }
  // the recurrent weight gradient accumulated inside the recurrence kernel (partials per row group)
  const int dw_parts = h16 ? path.bwd.dw_parts : 0;
  if (path.persistent) {
    srk::GruPArgs p = rec_args(B, T, H, w_hh, ws, L);
    p.y_in = y; p.gates = gates; p.dy = dy;
    if (h16) {   // the kernel writes dgi16 / dgh16 and the bias-gradient partials
      p.dgi16 = const_cast<uint16_t*>(m_dgi.h); p.dgh16 = const_cast<uint16_t*>(m_dgh.h); p.dbias = ws + L.part;
      if (dw_parts) {
        if ((rc = srk::g_gs.get((size_t)dw_parts * 2 * 3 * H * H, &p.dw_part))) return rc;
        p.y16_in = m_y.h;
      }
    } else {
      p.dgi = dgi; p.dgh = dgh; p.dgh_edge = dgh_edge;
      p.one_dir = top_last >= 2 ? 1 : 0;
    }
    if ((rc = srk::gru_persistent_launch(p, path.bwd, true, s))) return rc;
    if (h16) {
      const int prows = path.bwd.bias_part_rows, bparts = (int)((B + 255) / 256 * (256 / prows));
      if (dw_parts) {   // dW_hh and the bias gradients from their partials: one launch
        const int64_t per_dir = 3 * H * H, n4 = 2 * per_dir / 4;
        const int dw_blocks = (int)((n4 + 255) / 256);
        srk::ProfScope prof("gru_dwhh_reduce", s, 4.0 * (dw_parts + 2) * 2 * per_dir);
        hipLaunchKernelGGL(srk::dwhh_dbias_reduce_kernel, dim3((unsigned)(dw_blocks + (6 * H + 255) / 256)), dim3(256),
                           0, s, p.dw_part, dw_parts, (int)B, per_dir, dw_hh, (int)accumulate, dw_blocks, p.dbias,
                           bparts, (int)H, prows, db_ih, db_hh);
        SRK_CHECK_HIP(hipGetLastError());
      } else if ((rc = srk::launch256(srk::dbias_reduce_kernel, 6 * H, s, p.dbias, bparts, B, H, prows, db_ih, db_hh,
                                      accumulate))) {
        return rc;
      }
    }
    // top_last == 3: the full dW_ih / dx GEMMs below read whole dgi rows: the reverse columns' true value, zero.
    // Nothing reads them when dW_ih goes through the group (its packing copies the live rows only) and dx through
    // gemm_f32_klive.
    const bool rev_unread = grouped && (!dx || dx_klive);
    if (top_last == 3 && !rev_unread && (rc = srk::launch256(srk::zero_cols_kernel, BT * 3 * H / 4, s, dgi, BT, 3 * H, 3 * H, 6 * H)))
      return rc;
    if (top_last >= 2 && (rc = srk::launch256(srk::rev_cell_bwd_kernel, B * H, s, gates, dy_last, B, T, H, dgi, dgh_edge)))
      return rc;
  } else {
    srk::GruArgs a{};
    a.B = (int)B; a.T = (int)T; a.H = (int)H; a.in = (int)in;
    a.y_in = y; a.w_hh = w_hh; a.gates = gates;
    a.dy = dy; a.dgi = dgi; a.dgh = dgh; a.dgh_edge = dgh_edge; a.dhz = ws + L.dhz;
    a.G = (int)((B + srk::kRows - 1) / srk::kRows);
    a.S = (int)(H / srk::kUnits);
    const dim3 grid((unsigned)(2 * a.G * a.S));
    for (int step = 0; step < T; ++step) {
      srk::ProfScope prof("gru_bwd_step", s, step > 0 ? 2.0 * 2.0 * (double)B * 3 * H * H : 0.0);   // 2 dirs x [B,3H]x[3H,H]
      hipLaunchKernelGGL(srk::gru_bwd_step_kernel, grid, dim3(256), 0, s, a, step);
    }
    SRK_CHECK_HIP(hipGetLastError());
  }

  // fp32: the bias gradients are fused row sums of the GEMMs' A operands (16-bit: from the kernel's partials, above)
  const bool sums = !h16;
  // modes 1 and 2: the reverse direction's dgi taken as its B live rows (b, T-1), lda = T 6H; mode 3 keeps the full
  // dW_ih / dx GEMMs (their sums' order, so their bits) and drops only the reverse dW_hh
  const bool rev_last = top_last == 1 || top_last == 2;
  const Mat m_dgi_rev = m_dgi.at((T - 1) * 6 * H + 3 * H);
  if (grouped) {
    const int64_t rows = pp.nslabs * pp.pslab;
    float* packed = nullptr;   // A' [rows][3H] | B' [rows][ld]
    if ((rc = srk::g_gs.get((size_t)rows * (3 * H + ld), &packed))) return rc;
    if ((rc = srk::gemm_pack_rows(pp, dgi + 3 * H, 6 * H, 3 * H, m_x.f, ld, ld, packed, packed + rows * 3 * H, s)))
      return rc;
    GemmDesc m[3];
    m[0] = full;   // the forward half: rows 0 .. 3H of the full GEMM
    m[0].M = 3 * H; m[0].plan_M = 6 * H;
    m[1] = hh;     // the forward direction of the two-direction launch
    m[1].batch = 1; m[1].plan_batch = 2;
    m[2] = m[0];   // the reverse half over the packed K
    m[2].K = rows; m[2].pin_splits = (int)pp.nslabs; m[2].pin_kchunk = pp.pslab;
    m[2].A = packed; m[2].lda = 3 * H;
    m[2].B = packed + rows * 3 * H;
    m[2].C = full.C + 3 * H * ld;
    m[2].rowsum = db_ih + 3 * H;
    if ((rc = srk::gemm_f32_group(m, 3, s))) return rc;
    if (pad && (rc = srk::launch256(srk::unpad_cols_kernel, 6 * H * in, s, dwpad, 6 * H, ld, dw_ih, in, accumulate)))
      return rc;
    if (!accumulate) {   // dW_hh[1] = 0; db_hh[1] = the column sums of dgh_edge[1] below
      SRK_CHECK_HIP(hipMemsetAsync(dw_hh + 3 * H * H, 0, sizeof(float) * 3 * H * H, s));
      SRK_CHECK_HIP(hipMemsetAsync(db_hh + 3 * H, 0, sizeof(float) * 3 * H, s));
    }
  }
  if (!grouped) {
    // dW_ih_cat[6H, in] = dgi^T [6H, BT] * x [BT, in] (the forward's padded x); fp32: db_ih = the row sums of dgi^T
    GemmDesc g;
    g.M = rev_last ? 3 * H : 6 * H; g.N = ld; g.K = BT;
    set_a(g, m_dgi); g.lda = 6 * H; g.ta = true;
    set_b(g, m_x); g.ldb = ld;
    g.C = pad ? dwpad : dw_ih; g.ldc = ld; g.beta = pad ? 0.f : beta;
    if (sums) { g.rowsum = db_ih; g.rowsum_beta = beta; }
    if ((rc = srk::gemm_f32(g, s))) return rc;
    if (rev_last) {   // the reverse half from its B live rows against x[:, T-1, :]
      g.K = B;
      set_a(g, m_dgi_rev); g.lda = T * 6 * H;
      set_b(g, m_x.at((T - 1) * ld)); g.ldb = T * ld;
      g.C += 3 * H * g.ldc;
      g.rowsum = db_ih + 3 * H;
      if ((rc = srk::gemm_f32(g, s))) return rc;
    }
    if (pad && (rc = srk::launch256(srk::unpad_cols_kernel, 6 * H * in, s, dwpad, 6 * H, ld, dw_ih, in, accumulate)))
      return rc;
  }
  if (!dw_parts && !grouped) {   // (else the recurrence kernel accumulated it: dwhh_dbias_reduce_kernel above)
    // dW_hh[dir][3H, H] = sum_(b,t) dgh[b][t]^T h_prev[b][t]; h_prev of row (b,t) is y row (b,t-1)
    // (dir 0) or (b,t+1) (dir 1); the edge rows of dgh are zero so the batch seams contribute 0.
    // fp32: db_hh = row sums of dgh^T (fused) + the edge rows kept aside in dgh_edge.  Both directions run
    // as ONE batch-2 launch (dir 1 = dir 0's operands + sA / sB; option gru_dwhh_batched): a 24-tile grid
    // split 10 ways fills the CUs where two 12-tile launches ran one after the other.
    GemmDesc g;
    g.M = 3 * H; g.N = H; g.K = BT - 1;
    g.ta = true; g.lda = 3 * H; g.ldb = 2 * H;
    const Mat a0 = m_dgh.at(3 * H);   // dir 1: dgh + BT 3H
    const Mat b0 = m_y;               // dir 1: y + 3H (row 1, reverse half)
    set_a(g, a0);
    set_b(g, b0);
    g.C = dw_hh; g.ldc = H; g.beta = beta;
    g.batch = 2; g.sA = BT * 3 * H - 3 * H; g.sB = 3 * H; g.sC = 3 * H * H;
    if (sums) { g.rowsum = db_hh; g.rowsum_beta = beta; g.sRS = 3 * H; }
    // (the batched row sums exist on the ping-pong kernel only: 16-B rows, 32-bit buffer offsets)
    const bool batched = srk::g_opt_gru_dwhh_batched && (!sums || srk::gemm_f32_batched_rowsum_ok(g));
    if (top_last) {   // the forward direction alone; dW_hh[1] = 0 and db_hh[1] = the column sums of dgh_edge[1] below
      g.batch = 1;
      // mode 3: the kernel and K split of the two-direction launch, so its bits for dW_hh[0]
      g.plan_batch = (top_last == 3 && batched) ? 2 : 0;
      if (g.K > 0) {
        if ((rc = srk::gemm_f32(g, s))) return rc;
      } else if (!accumulate) {
        SRK_CHECK_HIP(hipMemsetAsync(dw_hh, 0, sizeof(float) * 3 * H * H, s));
        SRK_CHECK_HIP(hipMemsetAsync(db_hh, 0, sizeof(float) * 3 * H, s));
      }
      if (!accumulate) {
        SRK_CHECK_HIP(hipMemsetAsync(dw_hh + 3 * H * H, 0, sizeof(float) * 3 * H * H, s));
        SRK_CHECK_HIP(hipMemsetAsync(db_hh + 3 * H, 0, sizeof(float) * 3 * H, s));
      }
    } else if (g.K > 0 && batched) {
      if ((rc = srk::gemm_f32(g, s))) return rc;
    } else if (g.K > 0) {   // one launch per direction (A/B and tests)
      g.batch = 1;
      for (int dir = 0; dir < 2; ++dir) {
        set_a(g, a0.at(dir * g.sA));
        set_b(g, b0.at(dir * g.sB));
        g.C = dw_hh + dir * g.sC;
        if (sums) g.rowsum = db_hh + dir * g.sRS;
        if ((rc = srk::gemm_f32(g, s))) return rc;
      }
    } else if (!accumulate) {
      SRK_CHECK_HIP(hipMemsetAsync(dw_hh, 0, sizeof(float) * 2 * 3 * H * H, s));
      if (sums) SRK_CHECK_HIP(hipMemsetAsync(db_hh, 0, sizeof(float) * 2 * 3 * H, s));
    }
  }
  if (sums)
    for (int dir = 0; dir < 2; ++dir)
      if ((rc = srk::colsum_f32(dgh_edge + (size_t)dir * B * 3 * H, B, 3 * H, 3 * H, db_hh + dir * 3 * H, 1.f, s)))
        return rc;
  if (dx) {  // dx[BT, in] = dgi[BT, 6H] * W_ih_cat[6H, in]
    if (h16 && in <= srk::kFusedIn) {   // the fused-projection forward left W16 unwritten: round it here
      if ((rc = srk::to16(w_ih, 6 * H, in, const_cast<uint16_t*>(m_w.h), ld, s))) return rc;
    } else if (!h16 && pad) {
      if ((rc = srk::pad_cols(w_ih, 6 * H, in, wpad, s))) return rc;
    }
    GemmDesc g = gdx;
    if ((rc = dx_klive ? srk::gemm_f32_klive(g, s) : srk::gemm_f32(g, s))) return rc;
    if (rev_last) {   // rows (b, T-1) += dgi_rev_last * W_ih[1]
      g.M = B;
      set_a(g, m_dgi_rev); g.lda = T * 6 * H;
      set_b(g, m_w.at(3 * H * ld));
      g.C += (T - 1) * g.ldc; g.ldc *= T;
      g.beta = 1.f;
      if ((rc = srk::gemm_f32(g, s))) return rc;
    }
    if (pad && (rc = srk::launch256(srk::unpad_cols_kernel, BT * in, s, dxpad, BT, ld, dx, in, 0))) return rc;
  }
  return SRK_OK;
}

int srk_gru_layer_bwd_x16(const float* x, const void* x16_in, int64_t B, int64_t T, int64_t in, int64_t H,
                          const float* w_ih, const float* w_hh, const float* y, const float* ws_fwd, const float* dy,
                          float* dx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int accumulate,
                          float* ws, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_dims(B, T, in, H)) return rc;
  SRK_REQUIRE(x && w_ih && w_hh && y && ws_fwd && dy && dw_ih && dw_hh && db_ih && db_hh && ws, SRK_ERR_INVALID,
              "gru_bwd: null pointer");
  return layer_bwd(x, x16_in, B, T, in, H, w_ih, w_hh, y, ws_fwd, dy, nullptr, gru_path(B, T, in, H), 0, dx, dw_ih,
                   dw_hh, db_ih, db_hh, accumulate, ws, srk::as_stream(stream));
  SRK_API_END
}

int srk_gru_top_last_bwd(const float* x, const void* x16_in, int64_t B, int64_t T, int64_t in, int64_t H,
                         const float* w_ih, const float* w_hh, const float* y, const float* ws_fwd,
                         const float* dy_last, int mode, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                         float* db_hh, int accumulate, float* ws, void* stream) {
  SRK_API_BEGIN
  if (int rc = srk::check_dims(B, T, in, H)) return rc;
  SRK_REQUIRE(x && w_ih && w_hh && y && ws_fwd && dy_last && dw_ih && dw_hh && db_ih && db_hh && ws, SRK_ERR_INVALID,
              "gru_top_last_bwd: null pointer");
  SRK_REQUIRE(mode >= 0 && mode <= 3, SRK_ERR_INVALID, "gru_top_last_bwd: mode must be the forward's (0 .. 3)");
  // modes 1 .. 3 exist on the fp32 persistent path only; the forward chose the mode there
  const GruPath path = gru_path(B, T, in, H);
  SRK_REQUIRE(mode == 0 || path.top_last_ok, SRK_ERR_INVALID,
              "gru_top_last_bwd: mode %d needs the fp32 persistent path its forward ran on", mode);
  hipStream_t s = srk::as_stream(stream);
  // the [B][T][2H] gradient the recurrence reads: zeros and the last row (what last_step's backward builds)
  float* dy = ws + gru_ws(B, T, in, H, true).dy;
  if (int rc = srk::launch256(srk::pad_last_kernel, B * T * 2 * H / 4, s, dy_last, B, T, 2 * H, dy)) return rc;
  // mode 0 (16-bit precisions, H != 512, no persistent kernels): the full layer backward on that dy, exactly
  // what last_step(srk_gru_layer_fwd) backpropagates
  return layer_bwd(x, x16_in, B, T, in, H, w_ih, w_hh, y, ws_fwd, dy, dy_last, path, mode, dx, dw_ih, dw_hh, db_ih,
                   db_hh, accumulate, ws, s);
  SRK_API_END
}

}  // extern "C"
