// THE list of runtime options (srk_set_option / srk_get_option / srk_option_list): every option is stated here
// once.  srk_internal.h declares the variables from it, runtime.hip defines them with their defaults and builds the
// lookup table; srk_option_list prints it.
//
//   SRK_OPTION_LIST(V, H)
//     V(type, variable, "public name", accepts, default, "doc")   a plain int / unsigned variable
//     H("public name", hook, accepts, default, "doc")             stored by hand: option_set_<hook>(value) and
//                                                                 option_get_<hook>() in runtime.hip
//   accepts:  SRK_BOOL          any value, stored as value != 0
//             SRK_RANGE(lo, hi) lo <= value <= hi, stored as given
//             SRK_ONEOF(a, ...) one of the listed values
//             SRK_POINTER       any value (a device address)
//             SRK_ACTION        any value; nothing is stored and srk_get_option refuses the name
// The doc is one line.  Defaults of hooked entries are in the option's public units (what srk_get_option returns).
#pragma once

#define SRK_OPTION_LIST(V, H)                                                                                          \
  V(int, g_opt_gru_persistent, "gru_persistent", SRK_BOOL, 1,                                                          \
    "each GRU layer's recurrence as ONE persistent launch with W_hh resident in LDS (1) or one launch per time "       \
    "step (0)")                                                                                                        \
  V(int, g_opt_gemm16_kernel, "gemm16_kernel", SRK_RANGE(0, 2), 0,                                                     \
    "kernel of the 16-bit-operand GEMM (A/B measurements and tests): 0 by shape, 1 register-staged gemm_h16_kernel, "  \
    "2 LDS-DMA ping-pong gemm_g16_kernel")                                                                             \
  V(int, g_opt_conv16_sources, "conv16_sources", SRK_BOOL, 1,                                                          \
    "bf16 / fp16 convolutions gather from one pre-rounded 16-bit copy of x / dY / the weights (1) or round at "        \
    "LDS-store time (0); bit-identical results")                                                                       \
  V(int, g_opt_conv_fused_db, "conv_fused_db", SRK_BOOL, 1,                                                            \
    "conv bias gradients as column sums fused into the weight-gradient kernel (1) or the separate column-sum kernel "  \
    "over dY (0)")                                                                                                     \
  V(int, g_opt_conv_unpool_gather, "conv_unpool_gather", SRK_BOOL, 1,                                                  \
    "the pooled conv's backward gathers the pooled gradient through the argmax (1) or unpools into library scratch "   \
    "first (0)")                                                                                                       \
  V(int, g_opt_conv_tile, "conv_tile", SRK_ONEOF(128, 256), 128,                                                       \
    "conv tile shape: 128-row tiles of 4 waves, or 256-row tiles of 8 waves on tall convolutions")                     \
  V(int, g_opt_conv_ring, "conv_ring", SRK_RANGE(0, 0xf7), 0x77,                                                       \
    "LDS-DMA ring implicit-GEMM convolutions where the shape qualifies, a mask: 1 / 2 / 4 fp32 forward / data "        \
    "gradient / weight gradient, 16 / 32 / 64 the same on 16-bit operands, 128 the forward with the pooled epilogue "  \
    "and the fp32 forward at K < 3072 too (measured, r04ab / r04ab3 / r04ab6: the pooled ring forward slower in "      \
    "both precisions, the fp32 ring forward faster on the deep-K ResNet layers only)")                                 \
  V(int, g_opt_conv_unpool16, "conv_unpool16", SRK_BOOL, 1,                                                            \
    "16-bit-source modes: the pooled conv's backward writes the dense dY straight as its 16-bit copy (1) or a dense "  \
    "fp32 dY, then the 16-bit conversion and column sums (0)")                                                         \
  V(int, g_opt_conv_colsum16, "conv_colsum16", SRK_BOOL, 1,                                                            \
    "16-bit-source modes: the conv bias gradient (column sums of dY) fused into the pass that rounds dY (or unpools "  \
    "it) to its 16-bit copy (1) or a separate column-sum pass over dY (0)")                                            \
  V(int, g_opt_conv_ring_qs, "conv_ring_qs", SRK_RANGE(0, 7), 6,                                                       \
    "16-bit ring convs: whole 32-deep K-tiles per MFMA section (QS 2) by tile width, a 3-bit mask: bit 1 BN 128, "     \
    "bit 2 BN 256")                                                                                                    \
  V(int, g_opt_conv_fast16, "conv_fast16", SRK_BOOL, 1,                                                                \
    "register-staged 16-bit-source convs (fwd / dgrad): uniform-tap gathers with per-row bases and zero-filling "      \
    "buffer loads where the channels are a multiple of the K-tile (1) or the generic gathers (0)")                     \
  V(int, g_opt_conv_row16, "conv_row16", SRK_RANGE(0, 2), 1,                                                           \
    "fbanks_cnn conv2 + maxpool2 in 16-bit modes on the row-staged kernel (weights resident in LDS, image rows "       \
    "staged once per tile): 1 with 8 waves, 2 with 4 waves, 0 the implicit-GEMM kernels")                              \
  V(int, g_opt_conv_row32, "conv_row32", SRK_BOOL, 1,                                                                  \
    "fbanks_cnn conv2 (+ maxpool2) on fp32 operands on the row-staged kernels (x rows staged once per tile, the "      \
    "weights streamed one tap at a time) (1) or the implicit-GEMM kernels (0)")                                        \
  V(int, g_opt_conv_fw_gemm, "conv_fw_gemm", SRK_BOOL, 1,                                                              \
    "a full-width \"valid\" conv's forward (fbanks_cnn conv3, (1, 10) over width 10) as the plain GEMM x . Wt + bias " \
    "(1) or the implicit GEMM (0)")                                                                                    \
  V(int, g_opt_conv_row16_dgrad, "conv_row16_dgrad", SRK_RANGE(0, 2), 2,                                               \
    "the row-staged data gradient of fbanks_cnn conv2 in 16-bit modes: 2 = 5 units per wave, 1 = 3 / 3 / 2 / 2 row "   \
    "blocks per wave (418 vs 475-485 us, r05p), 0 = the implicit GEMM")                                                \
  V(int, g_opt_bn_tree, "bn_tree", SRK_RANGE(0, 2), 0,                                                                 \
    "BatchNorm training statistics: 0 = the <= 256 chunk partials combined in chunk order, the count ratios off the "  \
    "dependent chain; 1 = a fixed pairwise tree, one wave per channel (more accurate, but other bits than the "        \
    "reference's in-order arithmetic: ReLU decisions on values within roundoff of 0 move, tests/test_conv_gpu.py "     \
    "golden resnet_bgru at B = 2); 2 = in order with the divides in the chain (form 0's bitwise reference)")           \
  V(int, g_opt_mfcc_variant, "mfcc_variant", SRK_RANGE(0, 3), 3,                                                       \
    "K1 MFCC variant (bitwise-identical outputs): bit 0 = the untangle's partner exchange by DPP row_mirror instead "  \
    "of ds_bpermute, bit 1 = twiddles in registers instead of LDS")                                                    \
  V(int, g_opt_gemm_streamk, "gemm_streamk", SRK_BOOL, 1,                                                              \
    "stream-K for fp32 ping-pong GEMMs whose 256 x 256 grid covers 1/2 .. 1 round of CUs (1) or not (0)")              \
  V(int, g_opt_gemm32_kernel, "gemm32_kernel", SRK_RANGE(0, 2), 0,                                                     \
    "kernel of the fp32 GEMM: 0 by shape, 1 register-staged gemm_f32_kernel, 2 LDS-DMA ping-pong gemm_p32_kernel")     \
  H("matmul_precision", matmul_precision, SRK_RANGE(0, 2), 0,                                                          \
    "operand precision of the matrix-core kernels (GEMM, GRU recurrence): 0 fp32 (exact fp32 MFMA, the reference's "   \
    "arithmetic), 1 bf16, 2 fp16 operands (rounded to nearest-even on chip) with fp32 accumulation and fp32 "          \
    "tensors in and out")                                                                                              \
  V(int, g_opt_conv_fwd_fp32, "conv_fwd_fp32", SRK_BOOL, 0,                                                            \
    "16-bit modes: every convolution FORWARD pass on fp32 operands, the data / weight gradients on 16-bit ones (1) "   \
    "or all 16-bit (0).  resnet_bgru's training-mode BatchNorm chain amplifies the forward's operand rounding into "   \
    "4-39 % norm-wise gradient errors, while 16-bit gradients alone stay <= 0.9 % (tools/bf16_policy_resnet.py): "     \
    "the faithful 16-bit training mode of the BatchNorm models")                                                       \
  H("gru_trace_ptr", gru_trace_ptr, SRK_POINTER, 0,                                                                    \
    "diagnostics: device buffer of 8 x u64 per (workgroup, step) the persistent GRU kernels write, 0 = off")           \
  V(unsigned, g_opt_gru_spin_limit, "gru_spin_limit", SRK_RANGE(0, 0xffffffffLL), 0,                                   \
    "test hook: polls before a persistent wait gives up (0 = the default, ~2 s)")                                      \
  V(int, g_opt_gru_xcd_local, "gru_xcd_local", SRK_BOOL, 1,                                                            \
    "persistent GRU: XCD-local hand-off when the census allows (every XCD hosts one (dir, group))")                    \
  V(int, g_opt_gru_lp2, "gru_lp_32x32", SRK_BOOL, 1,                                                                   \
    "16-bit recurrence: 32 x 32 workgroups (1) or 64 rows x 16 units (0)")                                             \
  V(int, g_opt_gru_lp_wide, "gru_lp_wide", SRK_BOOL, 1,                                                                \
    "16-bit recurrence over > 256 rows: 64-row workgroups in one launch (1) or 256-row chunks (0)")                    \
  V(int, g_opt_gru_dc, "gru_fp32_dual_chain", SRK_BOOL, 1,                                                             \
    "fp32 recurrence: 8-wave workgroups running two independent row chains (1) or the 4-wave form (0)")                \
  H("gru_dc_offset_ns", gru_dc_offset_ns, SRK_RANGE(0, 1000000), 2000,                                                 \
    "fp32 two-chain kernels: delay of chain 1's start (phase offset between the chains), in ns; stored in ticks of "   \
    "10 ns, rounded down")                                                                                             \
  V(int, g_opt_gru_fast_cell, "gru_fp32_fast_cell", SRK_BOOL, 1,                                                       \
    "fp32 two-chain forward: hardware v_exp_f32 / v_rcp_f32 cell nonlinearities (1) or the exact ones (0)")            \
  V(int, g_opt_gru_dc_prio, "gru_dc_prio", SRK_RANGE(0, 2), 0,                                                         \
    "fp32 two-chain kernels: 0 equal priority, 1 / 2 chain 0 / 1 at s_setprio 1 (static)")                             \
  H("gru_dwhh_fused", gru_dwhh_fused, SRK_RANGE(0, 7), 1,                                                              \
    "16-bit backward: dW_hh accumulated in the recurrence kernel (bit 0) or by a GEMM over dgh16 / y16 (0); bit 1: "   \
    "h_prev fetched after the next exchange barrier, bit 2: recurrence waves at s_setprio 1 (timing variants, "        \
    "bitwise bit 0's results); an even value stores 0")                                                                \
  V(int, g_opt_gru_fwd_worker, "gru_fwd_worker", SRK_BOOL, 0,                                                          \
    "16-bit forward: y / gate stores and the gi fetch on extra worker waves (1) or not (0; off until measured)")       \
  V(int, g_opt_gru_dwhh_batched, "gru_dwhh_batched", SRK_BOOL, 1,                                                      \
    "16-bit GRU backward: both directions' dW_hh in one batched GEMM (1) or two (0)")                                  \
  V(int, g_opt_gru_top_last, "gru_top_last", SRK_RANGE(0, 3), 3,                                                       \
    "srk_gru_top_last_* on the fp32 persistent path: 0 = the full layer, 1 = the backward GEMMs without their "        \
    "all-zero reverse-direction parts, 2 = also the reverse direction as its one live cell, 3 = that cell and the "    \
    "forward-only launches of 2 with the full dW_ih / dx GEMMs, bit for bit the full layer's results")                 \
  V(int, g_opt_gemm_skinny, "gemm_skinny", SRK_BOOL, 1,                                                                \
    "GEMMs with a dimension <= 16 on the VALU skinny kernels (1) or the matrix-core tiles (0)")                        \
  V(int, g_opt_attn_pool_regs, "attn_pool_regs", SRK_BOOL, 1,                                                          \
    "attention pooling: clips that fit the register file are read once (1) or every shape on the two-pass kernel "     \
    "(0)")                                                                                                             \
  H("release_scratch", release_scratch, SRK_ACTION, 0,                                                                 \
    "free the library's grow-only scratch buffers (synchronizes the device; invalidates captured graphs)")
