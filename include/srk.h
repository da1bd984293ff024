/*
 * srk.h — the C ABI of libsrk.so, the MI355X (gfx950 / CDNA4) native hot path of
 * remit0/SpeechRecognitionProject: feature extraction -> acoustic model train step.
 *
 * Conventions (SURVEY.md §8b "C-ABI the build must export"):
 *  - every tensor pointer is a caller-owned DEVICE pointer (e.g. a torch tensor's data_ptr());
 *  - every call only ENQUEUES work on the caller's stream (`void* stream` = hipStream_t,
 *    nullptr = the legacy default stream) and returns 0 on success or a negative srk_status;
 *  - srk_last_error() returns a thread-local description of the last failure;
 *  - no call allocates device memory in steady state: scratch comes from the caller, sized by
 *    the matching *_workspace_bytes() query.  Constant tables are uploaded once per device
 *    by srk_init() (idempotent, thread-safe; called implicitly on first use);
 *  - layouts are row-major, innermost dimension last, fp32 unless the name says otherwise.
 *
 * Each entry point cites the reference function whose arithmetic it replaces
 * (paths relative to the reference repository).
 */
#ifndef SRK_H_
#define SRK_H_

#include <stdint.h>

#define SRK_ABI_VERSION 3

#ifdef __cplusplus
extern "C" {
#endif

enum srk_status {
  SRK_OK = 0,
  SRK_ERR_INVALID = -1,   /* bad argument (shape, null pointer, unsupported option) */
  SRK_ERR_HIP = -2,       /* a HIP runtime call failed */
  SRK_ERR_INTERNAL = -3,  /* anything else (host exception) */
  SRK_ERR_TIMEOUT = -4,   /* a persistent kernel's bounded spin-wait gave up: results are invalid */
};

/* ---------------------------------------------------------------- library / device */
int srk_version(void);                 /* ABI version, bumped on any signature change */
/* First 16 hex digits of the sha256 over the library's sources (the csrc .hip / .h / .cpp files and this
 * header, in name order) as built: profiling records (profiles/pmc_*.json) carry the stamp of the
 * library they measured, and bench.py attaches them only to a run of the same build.              */
const char* srk_source_stamp(void);
const char* srk_last_error(void);      /* thread-local, never NULL */
int srk_init(int device);              /* build + upload constant tables on `device` */
/* Opt-in kernel timing: while enabled, instrumented launches record a HIP event pair on their
 * stream; srk_prof_read sums, over every launch named `name` ("mfcc", "fbank", "spec",
 * "noise_mix", "gemm_f32", "gru_fwd_step", "gru_bwd_step", "adam", ...), the elapsed time and
 * the launches' ALGORITHMIC work (flops for matrix kernels, bytes for streaming kernels).
 * srk_prof_enable synchronizes the device and clears previous records.                     */
/* Generation of the library's grow-only scratch buffers (split-K slabs, conv / BatchNorm partials):
 * it changes whenever one is reallocated, which invalidates any HIP graph captured before.         */
int64_t srk_scratch_generation(void);
int srk_prof_enable(int on);
int srk_prof_read(const char* name, int64_t* count, double* total_ms, double* total_work);
/* Every record since srk_prof_enable grouped by (name, launch detail: kernel template + shape), one
 * "name\tdetail\tcount\ttotal_ms\ttotal_work\ttotal_bytes\n" line each, NUL-terminated into buf
 * (truncated at cap bytes); *needed = the full size.  total_bytes = the launches' ALGORITHMIC HBM
 * bytes where the launch site states them (matrix kernels: operands once + the output; 0 elsewhere).
 * bench.py names the largest single kernel with it and prices PMC traffic against the bytes. */
int srk_prof_kernels(char* buf, int64_t cap, int64_t* needed);
/* Runtime options.  Every option has a public name, a default and a rule for the values it accepts: a
 * boolean (any value, stored as value != 0), a range lo..hi, an explicit set such as 128|256, or, for
 * "release_scratch", an action that stores nothing.  srk_set_option refuses (SRK_ERR_INVALID, state
 * unchanged) an unknown name or a value outside the rule; srk_option_list is the full list with each
 * option's default, current value, rule and one-line description (csrc/options.h is its source).
 * Two an integrator meets: "matmul_precision" (default 0) = operand precision of the matrix-core
 * kernels (GEMM, GRU recurrence): 0 fp32 (exact, the reference's arithmetic), 1 bf16, 2 fp16 — operands
 * rounded to nearest-even on chip, fp32 accumulation, fp32 tensors in and out (BASELINE.json cfg2 / cfg5);
 * "conv_ring" (default 0x77) = the LDS-DMA ring implicit-GEMM convolutions where the shape qualifies
 * (bits 0-2 fp32 fwd / dgrad / wgrad, 4-6 the same in 16 bit, 7 also the pooled forward and the fp32
 * forward at K < 3072) — results equal up to fp32 summation order (A/B measurements and tests). */
int srk_set_option(const char* name, int64_t value);
/* *value = the value for which srk_set_option(name, *value) reproduces the option's current state (so
 * "gru_dc_offset_ns" in ns, "gru_dwhh_fused" as normalised).  SRK_ERR_INVALID for an unknown name, a null
 * pointer or the action "release_scratch". */
int srk_get_option(const char* name, int64_t* value);
/* One "name\tdefault\tcurrent\taccepts\tdoc\n" line per option, in the order of csrc/options.h, into buf
 * with the convention of srk_prof_kernels (NUL-terminated, truncated at cap bytes, *needed = the full
 * size).  accepts is "bool", "lo..hi", "a|b", "pointer" or "action"; an action's default and current
 * columns say "action". */
int srk_option_list(char* buf, int64_t cap, int64_t* needed);
/* Number of bounded spin-waits of the persistent kernels that gave up (synchronizes the
 * device; must stay 0 — a non-zero value means a co-residency assumption failed).  -1 on error. */
int64_t srk_spin_timeouts(void);
/* Fatal-timeout check: SRK_OK, or SRK_ERR_TIMEOUT (sticky until srk_health_reset) once any
 * persistent-kernel spin-wait has given up.  Reads a host-pinned word the kernels raise, so with
 * sync = 0 it costs no device synchronization (it sees timeouts of work the GPU has reached);
 * sync = 1 synchronizes the device first.  Option "gru_spin_limit" (test hook) shortens the wait. */
int srk_health_check(int sync);
/* Host-side audit of the persistent GRU's step-ordering words for a batch of B rows at the given
 * precision (0 fp32, 1 bf16, 2 fp16): *max_word = largest counter / flag word any workgroup of the
 * planned launches touches, *chunks = launches, *census = first word of the XCD census (must exceed
 * *max_word).  No GPU needed.                                                                     */
int srk_gru_audit_words(int64_t B, int precision, int backward, int64_t* max_word, int64_t* chunks, int64_t* census);
int srk_health_reset(void);

/* ---------------------------------------------------------------- feature extraction
 * pcm: float32 [n_clips, 16000], int16-valued (NOT scaled to +-1), exactly what
 * dataset.py:89-122 returns per item and DataLoader collates (training.py:77).        */

/* K2: log-mel filter banks, models/model_fbanks_cnn.py:15-66 (`filter_banks`).
 * out: [n_clips, 98, 120] (time x mel), dB.                                            */
int srk_fbank_fwd(const float* pcm, int64_t n_clips, float* out, void* stream);

/* K1: MFCC + delta + delta-delta, models/model_mfcc_bgru.py:11-19 (`compute_mfcc`, librosa
 * mfcc(n_mfcc=13, n_fft=640, hop=320) + np.gradient x2).
 * layout 0: out [n_clips, 39, 51] (the reference's compute_mfcc layout);
 * layout 1: out [n_clips, 51, 39] (time-major, = the transpose at model_mfcc_bgru.py:34). */
int srk_mfcc_fwd(const float* pcm, int64_t n_clips, float* out, int layout, void* stream);

/* K3: log spectrogram, models/model_spec_bgru.py:11-17 (`compute_spec`, scipy.signal.spectrogram
 * nperseg=640, noverlap=320, Tukey(0.25), PSD density, log(S + 1e-10)).
 * transposed 0: out [n_clips, 321, 49] (freq x time, model_spec_bgru.py);
 * transposed 1: out [n_clips, 49, 321] (time x freq, models/model_spec_cnn.py:14).     */
int srk_spec_fwd(const float* pcm, int64_t n_clips, float* out, int transposed, void* stream);

/* K1 / K2 / K3 on int16 PCM [n_clips, 16000] (4-byte aligned): the samples the WAV holds, widened to
 * float32 in the kernels' load stage — the same values as the float32 entry points above (the
 * reference's float32 PCM is int16-valued, dataset.py:117), at half the bytes to upload and read. */
int srk_fbank_fwd_i16(const int16_t* pcm, int64_t n_clips, float* out, void* stream);
int srk_mfcc_fwd_i16(const int16_t* pcm, int64_t n_clips, float* out, int layout, void* stream);
int srk_spec_fwd_i16(const int16_t* pcm, int64_t n_clips, float* out, int transposed, void* stream);

/* K2-VTLP: K2 with the mel filter bank warped per clip — the vocal-tract-length perturbation of the
 * reference's "top" fbank model, legacy/model_8/dataset_top.py:245-267 (one np.random.uniform(0.9, 1.1)
 * per item there).  alpha: float64 [n_clips] on the device.  With m = min(alpha, 1) the 122 mel points
 * hz[i] of model_fbanks_cnn.py:48-50 move to hz * alpha below the knee 4800 m / alpha and to
 * 8000 - s (8000 - hz), s = (8000 - 4800 m) / (8000 - 4800 (m / alpha)), above it (:252), then
 * bin = floor(513 hz' / 16000) (:254) and the triangles of :256-264; everything else is K2.
 * alpha = 1 is K2's matrix.  Domain: finite alpha in [0.8, 1.25]; a clip whose alpha is outside it (or
 * NaN) gets NaN in its whole [98, 120] output (alpha lives on the device: no host check), the other
 * clips are unaffected.  out: [n_clips, 98, 120].                                                      */
int srk_fbank_vtlp_fwd(const float* pcm, int64_t n_clips, const double* alpha, float* out, void* stream);
int srk_fbank_vtlp_fwd_i16(const int16_t* pcm, int64_t n_clips, const double* alpha, float* out, void* stream);
/* The 122 warped FFT bins of srk_fbank_vtlp_fwd for one alpha (host only, no GPU needed; the same
 * function the kernel evaluates).  bins: int32 [122] on the host.  SRK_ERR_INVALID for an alpha outside
 * [0.8, 1.25] (NaN included) or a null pointer.                                                        */
int srk_vtlp_bins(double alpha, int32_t* bins);

/* K4: uniform noise mix, dataset.py:183-193 (`add_noise_uniform`) with the random draws made
 * explicit: out[b, i] = (float) int16_trunc( (double)pcm[b, i] + gain[b] * (double)
 *                        bank[file_idx[b] * bank_len + offset[b] + i] ).
 * pcm: int16 [n_clips, 16000]; bank: int16 [n_files, bank_len]; out: float32 [n_clips, 16000].
 * The caller guarantees 0 <= offset[b] <= bank_len - 16000 and 0 <= file_idx[b] < n_files. */
int srk_noise_mix(const int16_t* pcm, const int16_t* bank, int64_t n_files, int64_t bank_len,
                  const int64_t* file_idx, const int64_t* offset, const double* gain,
                  int64_t n_clips, float* out, void* stream);

/* K4 fused into K3's load stage (model_spec_bgru on noise-augmented clips, dataset.py:183-193 then
 * models/model_spec_bgru.py:11-17): out = srk_spec_fwd of srk_noise_mix(pcm, bank, ...) — the same
 * values bit for bit — without the mixed fp32 PCM going through HBM (int16 clip + int16 noise window
 * in, the spectrogram out).  Arguments as srk_noise_mix (bank 4-byte aligned) and srk_spec_fwd. */
int srk_spec_noise_fwd(const int16_t* pcm, const int16_t* bank, int64_t n_files, int64_t bank_len,
                       const int64_t* file_idx, const int64_t* offset, const double* gain, int64_t n_clips,
                       float* out, int transposed, void* stream);

/* K10: batched training-mode augmentation, dataset.py:103-118 and its helpers :148-223, with the
 * random draws made explicit (one op per clip; the Python `Dataset.__getitem__` draws them per
 * item, srk_augment applies a whole batch in one launch).  op[b]:
 *   SRK_AUG_NONE      out = pcm
 *   SRK_AUG_SPEED     speed_tuning (:206-223): cv2 INTER_LINEAR resample to iparam[b] =
 *                     int(16000 * rate) samples, then centre cut, or random pad when shorter
 *   SRK_AUG_SHIFT     time_stretching (:195-204): shift by iparam[b] in (-16000, 16000)
 *   SRK_AUG_NOISE     add_noise_uniform (:183-193): int16(pcm + dparam[b] * noise)
 *   SRK_AUG_NOISE_SNR add_noise_snr (:163-181): dparam[b] = 10 ** (snr_dB / 10)
 *   SRK_AUG_SILENCE   generate_silence_sample (:148-161): float32(noise * dparam[b]); pcm unused;
 *                     noise_pos[b] < 0 gives the all-zero sample
 *   SRK_AUG_PITCH     pitch_shifting (:225-235): out = pcm here; srk_pitch_shift (K12) then
 *                     overwrites the clip with its shifted version (iparam[b] = n_steps)
 * noise = bank[noise_pos[b] .. + 16000) of the flat int16 noise bank (ragged files concatenated);
 * ops without noise ignore noise_pos.  The pad samples the reference draws with
 * np.random.randint(-32, 32, k) come from a counter hash of (seed, b, output position)
 * (oracle/augment.py aug_fill).  pcm: int16 [n_clips, 16000] (zero padded as dataset.py:100-102),
 * out: float32 [n_clips, 16000]; both 16-byte aligned.  op/iparam/noise_pos/dparam: device arrays
 * of n_clips entries, validated by the caller (out-of-range noise windows read as silence). */
/* ---------------------------------------------------------------- evaluation callers
 * K11: softmax ensemble, predictions.py:56-69 / models/model_analyst.py:22-53: logits float32
 * [K, B, C] (model-major) -> per clip the softmax of each model's logits; probs_cat [B, K*C] their
 * concatenation (the analyst's input, nullable), mean [B, C] = (p_1 + ... + p_K) / K (nullable),
 * pred int64 [B] = first arg-max of the mean (nullable).  1 <= K <= 8, 1 <= C <= 64.          */
int srk_softmax_ensemble(const float* logits, int64_t K, int64_t B, int64_t C, float* probs_cat, float* mean,
                         int64_t* pred, void* stream);

/* ---------------------------------------------------------------- input pipeline (host)
 * Batched WAV decode, dataset.py:98-102 (scipy.io.wavfile.read + zero pad to 16000): n files
 * (NUL-terminated paths) decoded by up to min(n_threads, 16) host threads (n_threads <= 0: all
 * hardware threads, capped at 16) into out int16 [n, 16000] (HOST memory, e.g. pinned): the first
 * min(len, 16000) samples, zero padded.  lengths[b] = the file's sample count (a count > 16000
 * is reported as is — dataset.py:104-106 then fails on that item), or a negative SRK_WAV_ERR_*
 * with out[b] all zero.  PCM16 mono RIFF/WAVE only (tag 1 or WAVE_FORMAT_EXTENSIBLE/PCM); other
 * chunks skipped.  Returns SRK_OK unless the arguments are invalid: per-file errors are data,
 * as __getitem__'s except branch (dataset.py:124-128) makes them.  Touches no GPU state.      */
enum { SRK_WAV_ERR_OPEN = -1, SRK_WAV_ERR_FORMAT = -2, SRK_WAV_ERR_UNSUPPORTED = -3 };
int srk_wav_read_batch(const char* const* paths, int64_t n, int16_t* out, int64_t* lengths, int n_threads);

enum { SRK_AUG_NONE = 0, SRK_AUG_SPEED = 1, SRK_AUG_SHIFT = 2, SRK_AUG_NOISE = 3, SRK_AUG_NOISE_SNR = 4,
       SRK_AUG_SILENCE = 5, SRK_AUG_PITCH = 6 /* srk_augment copies the clip; srk_pitch_shift shifts it */ };
int srk_augment(const int16_t* pcm, int64_t n_clips, const int16_t* bank, int64_t bank_len, const int32_t* op,
                const int64_t* iparam, const int64_t* noise_pos, const double* dparam, uint64_t seed, float* out,
                void* stream);

/* K12: batched pitch_shifting, dataset.py:225-235 — np.int16(librosa.effects.pitch_shift(
 * sample.astype(float), 16000, n_steps)) for n_steps in {-2, -1, 1, 2} (the reference's level None
 * leaves the clip as is): librosa 0.6's time_stretch (STFT 2048 / 512, phase vocoder, inverse STFT)
 * then resampy's kaiser_best resample from 16000 / rate to 16000 Hz, rate = 2^(-n_steps / 12)
 * (algorithm and dtypes: oracle/pitch.py; parity unpinned — librosa / resampy are absent).
 * For s < n_shift: out[clip_idx[s]] = the shifted pcm[clip_idx[s]] as int16-valued float32,
 * level_idx[s] in 0..3 = n_steps -2, -1, 1, 2.  pcm: int16 [n_clips, 16000]; out: float32
 * [n_clips, 16000] (rows not listed untouched); clip_idx / level_idx: device int32 [n_shift],
 * validated by the caller.  One launch for the whole batch (one workgroup per shifted clip).
 * workspace: device scratch of srk_pitch_workspace_bytes(n_shift) bytes, 16-byte aligned.     */
int64_t srk_pitch_workspace_bytes(int64_t n_shift);
int srk_pitch_shift(const int16_t* pcm, int64_t n_clips, const int32_t* clip_idx, const int32_t* level_idx,
                    int64_t n_shift, float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- dense algebra (fp32 MFMA)
 * C[M,N] = alpha * op(A) op(B) + beta * C (+ bias), row-major.  op(A) = A [M,K] (lda) or, with
 * trans_a, A stored [K,M]; op(B) = B [K,N] (ldb) or, with trans_b, B stored [N,K].
 * bias_mode: 0 none, 1 bias[N] per column, 2 bias[M] per row.  Replaces the cuBLAS/CPU GEMMs of
 * nn.Linear (model_mfcc_bgru.py:26,36; model_fbanks_cnn.py:80-81,99-100).                  */
int srk_gemm_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                 int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc,
                 const float* bias, int bias_mode, void* stream);
/* The same GEMM (alpha, beta, no bias) that also writes rowsum[m] = beta * rowsum[m] +
 * sum_k op(A)[m, k]: the weight and bias gradients of a Linear in one pass (dW = dY^T X,
 * db = sum over the batch of dY); beta = 1 accumulates both into existing .grad buffers.     */
int srk_gemm_rowsum_f32(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const float* A,
                        int64_t lda, const float* B, int64_t ldb, float beta, float* C, int64_t ldc,
                        float* rowsum, void* stream);
/* The same GEMM on 16-bit operands already in memory (bf16 or fp16 as set by matmul_precision,
 * which must not be fp32): A / B hold raw 16-bit values, leading dimensions in elements; fp32
 * accumulation, C / bias fp32.  Needs 16-B aligned rows whose lengths are multiples of 8.      */
int srk_gemm_16(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha, const uint16_t* A,
                int64_t lda, const uint16_t* B, int64_t ldb, float beta, float* C, int64_t ldc,
                const float* bias, int bias_mode, void* stream);
/* Batched form of srk_gemm_16 (no bias): for z < batch, C + z sC = alpha op(A + z sA) op(B + z sB)
 * + beta (C + z sC); strides in elements, multiples of 8 (sC of 4).  The BiGRU backward's two
 * recurrent weight gradients (nn.GRU weight_hh_l{k}{,_reverse}.grad, models/model_mfcc_bgru.py:25)
 * run as one batch-2 launch.                                                                  */
int srk_gemm_16_batched(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, float alpha,
                        const uint16_t* A, int64_t lda, int64_t sA, const uint16_t* B, int64_t ldb,
                        int64_t sB, float beta, float* C, int64_t ldc, int64_t sC, int batch, void* stream);
/* out[n] = beta * out[n] + sum_m X[m, n]  (bias gradients).                                 */
int srk_colsum_f32(const float* X, int64_t M, int64_t N, int64_t ldx, float* out, float beta, void* stream);
/* Debug: the launch plan of the GEMM these arguments describe, as text; no GPU needed.  operands16 = the
 * 16-bit-operand entry points, has_rowsum = fused row sums, prec = -1 (the matmul_precision option) or 0 / 1 / 2,
 * no_split / plan_batch = the internal fields of the same names (0 from the public entry points).  The four
 * addresses are inspected for alignment and nullness only.  buf receives two lines,
 *   "<profiler name>|<kernel and shape as srk_prof_kernels reports them>"
 *   "reduce=<none|splitk_reduce|splitk_reduce4>[+rowsum] scratch=<floats of library scratch>";
 * returns the status the GEMM itself would return for these arguments.                            */
int srk_gemm_plan_describe(int trans_a, int trans_b, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb,
                           int64_t ldc, int batch, int64_t sA, int64_t sB, int64_t sC, int bias_mode, int has_rowsum,
                           int operands16, int prec, int no_split, int plan_batch, uint64_t a_addr, uint64_t b_addr,
                           uint64_t c_addr, uint64_t bias_addr, char* buf, int64_t cap);
/* Host only, no GPU needed: the zero-block packing plan of a K dimension whose operand rows are zero but for
 * `count` live rows first, first + stride, ... (stride >= 8, all below K).  K is walked in slabs of `slab` k (a
 * positive multiple of 16, the K split of the GEMM being packed); every 8-aligned k block holding a live row is
 * kept in the slab of its original k, and every slab is padded with zero blocks to *packed_slab, the longest
 * slab's kept length rounded up to 16.  blocks receives the kept block indices (k / 8) slab by slab in k order
 * (`count` of them; blocks_cap >= count), slab_counts[s] the number kept in slab s (slabs_cap >= *n_slabs =
 * ceil(K / slab)).  The last-step top BiGRU layer packs its reverse direction's dW_ih GEMM by this plan.
 * SRK_ERR_INVALID on arguments outside those ranges.                                               */
int srk_gemm_pack_plan(int64_t K, int64_t slab, int64_t first, int64_t stride, int64_t count, int64_t* blocks,
                       int64_t blocks_cap, int64_t* slab_counts, int64_t slabs_cap, int64_t* n_slabs,
                       int64_t* packed_slab);
/* C [M,N] (ldc) = A [M,K] (lda) * B [K,N] (ldb) where columns k >= k_live of A are zero in every row but the `count`
 * live rows first, first + stride, ... (stride >= 8, all below M): the stream-K launch of srk_gemm_f32 for these
 * arguments without the K-tiles known to be zero, its cuts unmoved, then the live rows over the full K.  Bit for
 * bit what srk_gemm_f32 (alpha 1, beta 0, no bias) gives on the zero-filled A, up to the sign of a zero and for
 * finite B; columns k >= k_live of the other rows are never read.  SRK_ERR_INVALID unless the product plans as the
 * fp32 stream-K ping-pong kernel and k_live is a multiple of 16 in (0, K).                              */
int srk_gemm_f32_klive(int64_t M, int64_t N, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                       float* C, int64_t ldc, int64_t k_live, int64_t first, int64_t stride, int64_t count,
                       void* stream);
/* Host only, no GPU needed: what srk_gemm_f32_klive keeps of the stream-K plan of a packed (M, N, K) product:
 * *tiles output tiles of *ktiles 16-deep K-tiles each, cut into *wgs equal runs; kept[w] = the K-tiles workgroup w
 * still executes (kept_cap >= *wgs), live_runs[t] = the runs that execute K-tiles of tile t (runs_cap >= *tiles).
 * beta and bias_mode are those of the GEMM asked for; SRK_ERR_INVALID where srk_gemm_f32_klive would refuse.  */
int srk_gemm_klive_plan(int64_t M, int64_t N, int64_t K, int64_t k_live, int64_t first, int64_t stride, int64_t count,
                        float beta, int bias_mode, int64_t* kept, int64_t kept_cap, int64_t* live_runs,
                        int64_t runs_cap, int64_t* tiles, int64_t* ktiles, int64_t* wgs);

/* ---------------------------------------------------------------- K5: bidirectional GRU layer
 * nn.GRU(in, H, bidirectional=True, batch_first=True), one layer, PyTorch gate order [r; z; n],
 * h0 = 0 (model_mfcc_bgru.py:25,35; model_spec_bgru.py:23,33; model_resnet_bgru.py:130,135).
 * x [B, T, in]; y [B, T, 2H] (forward direction in [..., :H], reverse in [..., H:]).
 * Weights are direction-stacked: w_ih [2][3H][in] (= weight_ih_lK ; weight_ih_lK_reverse),
 * w_hh [2][3H][H], b_ih [2][3H], b_hh [2][3H].  H must be a multiple of 128.
 * ws (fwd, kept until the backward): srk_gru_workspace_floats(.., backward=0) floats;
 * ws (bwd scratch): srk_gru_workspace_floats(.., backward=1) floats.
 * Backward writes dx [B, T, in] (NULL when the input needs no gradient) and OVERWRITES
 * (accumulate = 0) or ADDS TO (accumulate = 1: autograd's .grad accumulation, done in the GEMM
 * epilogues) dw_ih, dw_hh, db_ih, db_hh (same stacked layouts).  The backward must run at the
 * matmul_precision of its forward (with bf16 / fp16 the forward workspace carries the 16-bit
 * operands of the backward's GEMMs; a layer with the fused input projection, in <= 64, leaves the
 * 16-bit W_ih slot to the backward, which fills it there only when dx is requested).          */
int64_t srk_gru_workspace_floats(int64_t B, int64_t T, int64_t in, int64_t H, int backward);
int srk_gru_layer_fwd(const float* x, int64_t B, int64_t T, int64_t in, int64_t H, const float* w_ih,
                      const float* w_hh, const float* b_ih, const float* b_hh, float* y, float* ws,
                      void* stream);
int srk_gru_layer_bwd(const float* x, int64_t B, int64_t T, int64_t in, int64_t H, const float* w_ih,
                      const float* w_hh, const float* y, const float* ws_fwd, const float* dy, float* dx,
                      float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int accumulate, float* ws,
                      void* stream);
/* The same pair taking x's ready 16-bit copy x16 ([B*T][in] bf16 / fp16 at the current precision,
 * in % 8 == 0, 16-B aligned; nullable = the plain pair) instead of rounding x: a 2-layer BiGRU's
 * second layer reads the first layer's own 16-bit h copy, which srk_gru_y16_offset locates in that
 * layer's forward workspace (in floats; -1 when the layer does not take the 16-bit path).  The
 * backward must get the forward's x16.  Bitwise the results of the plain pair (the kernels round h
 * exactly as the conversion of x would).                                                          */
int64_t srk_gru_y16_offset(int64_t B, int64_t T, int64_t in, int64_t H);
int srk_gru_layer_fwd_x16(const float* x, const void* x16, int64_t B, int64_t T, int64_t in, int64_t H,
                          const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* y,
                          float* ws, void* stream);
int srk_gru_layer_bwd_x16(const float* x, const void* x16, int64_t B, int64_t T, int64_t in, int64_t H,
                          const float* w_ih, const float* w_hh, const float* y, const float* ws_fwd, const float* dy,
                          float* dx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int accumulate,
                          float* ws, void* stream);
/* The TOP layer of a model that reads only the last step, fc(y[:, T-1, :]) (model_mfcc_bgru.py:43-44): the
 * _x16 pair with y_last [B, 2H] = y[:, T-1, :] as the output and dy_last [B, 2H] as the incoming gradient.
 * Row T-1 of the reverse direction is its FIRST step (one cell from h = 0), and in the backward its dgi is zero
 * at every t < T-1, its dgh zero everywhere and dW_hh[1] = 0.  *mode reports what the forward did and goes to
 * the backward unchanged:
 *   0  the full layer, exactly srk_gru_layer_fwd_x16 / _bwd_x16 on dy = (zeros, dy_last): every 16-bit
 *      precision, H != 512, and whenever the persistent recurrence kernels do not run;
 *   1  fp32 persistent path: the full forward; the backward GEMMs (dW_ih, dW_hh, dx) without their identically
 *      zero reverse-direction parts (option "gru_top_last" = 1);
 *   2  also the reverse direction as its one cell each way, the recurrence launches running the forward
 *      direction only, the input projection its 3H columns plus B rows of the reverse one ("gru_top_last" = 2).
 *      The reverse half of y at t < T-1 is then NOT written: y is the backward's h_prev source only.  The pruned
 *      dW_ih / dx sums run in another order than the full layer's: results differ from mode 0 by fp32 rounding.
 *   3  mode 2's forward, recurrence launches, cells and forward-only dW_hh, with the reverse dgi rows zero-filled
 *      and the full dW_ih / dx GEMMs kept: every sum runs in the full layer's order, so y_last and all gradients
 *      are bit for bit mode 0's wherever the layer's input projection runs as one unsplit GEMM (default).
 * dW_hh[1] is zero-filled (accumulate = 0) or left alone (accumulate = 1).
 * ws: srk_gru_top_last_workspace_floats(.., backward) floats each way.                                    */
int64_t srk_gru_top_last_workspace_floats(int64_t B, int64_t T, int64_t in, int64_t H, int backward);
int srk_gru_top_last_fwd(const float* x, const void* x16, int64_t B, int64_t T, int64_t in, int64_t H,
                         const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* y,
                         float* y_last, float* ws, int* mode, void* stream);
int srk_gru_top_last_bwd(const float* x, const void* x16, int64_t B, int64_t T, int64_t in, int64_t H,
                         const float* w_ih, const float* w_hh, const float* y, const float* ws_fwd,
                         const float* dy_last, int mode, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                         float* db_hh, int accumulate, float* ws, void* stream);

/* ---------------------------------------------------------------- K6: convolution / pooling
 * nn.Conv2d / nn.Conv1d (zero padding ph/pw, stride sh/sw, no groups — depthwise: srk_dwconv2d_nhwc_*; dilation: srk_conv1d_nlc_dil_*) as implicit GEMM
 * on CHANNELS-LAST activations: x [N][H][W][Ci], y [N][Ho][Wo][Co], Ho = (H + 2ph - KH)/sh + 1.
 * Weights stay in torch layout w [Co][Ci][KH][KW] (the state_dict tensor), bias [Co] (nullable).
 * ws: srk_conv2d_workspace_floats() floats (re-laid-out weights).  The 1-D convolutions of
 * model_resnet_bgru.py are H = 1, KH = 1.  Replaces model_fbanks_cnn.py:72-75,89-94.
 * Backward writes dw [Co][Ci][KH][KW] (overwrite), db (nullable) and dx (nullable).          */
int64_t srk_conv2d_workspace_floats(int64_t Ci, int64_t Co, int64_t KH, int64_t KW);
int srk_conv2d_nhwc_fwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w,
                        const float* bias, int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh,
                        int64_t sw, float* y, float* ws, void* stream);
int srk_conv2d_nhwc_bwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w, int64_t Co,
                        int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw, const float* dy,
                        float* dx, float* dw, float* db, float* ws, void* stream);
/* The same pair with the forward's 16-bit copy of x kept for the backward (bf16 / fp16 matmul
 * precision, Ci and Co multiples of 8, 16-B aligned tensors: the 16-bit operand path).  fwd16
 * rounds x into x16 (N*H*W*Ci 16-bit elements, 16-B aligned, caller storage) and sets
 * *x16_written = 1 when that path ran, else 0 (x16 untouched); bwd16 gathers from that copy instead
 * of rounding x again (x16 null: as srk_conv2d_nhwc_bwd).  The backward must run at the forward's
 * precision.  Bitwise the results of the plain pair.  *x16_written = 2 on entry declares that x16
 * already holds x's copy at this precision (srk_batchnorm_fwd16's y16): fwd16 then reads it instead
 * of rounding x.  bwd16_dy16 also takes dY's ready copy dy16 (srk_batchnorm_bwd16's dx16; nullable;
 * used wherever the 16-bit path would round dy, dy itself still required).                   */
int srk_conv2d_nhwc_fwd16(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w,
                          const float* bias, int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh,
                          int64_t sw, float* y, float* ws, void* x16, int* x16_written, void* stream);
int srk_conv2d_nhwc_bwd16(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w, int64_t Co,
                          int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw, const float* dy,
                          float* dx, float* dw, float* db, float* ws, const void* x16, void* stream);
int srk_conv2d_nhwc_bwd16_dy16(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w,
                               int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw,
                               const float* dy, const void* dy16, float* dx, float* dw, float* db, float* ws,
                               const void* x16, void* stream);
/* The same with dw_accumulate = 1: dw is the parameter's existing .grad and the weight gradient is ADDED
 * to it (autograd's accumulation of a returned gradient, fused into the layout kernel that writes it). */
int srk_conv2d_nhwc_bwd16_acc(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w,
                              int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw,
                              const float* dy, const void* dy16, float* dx, float* dw, float* db, float* ws,
                              const void* x16, int dw_accumulate, void* stream);
/* Dilated nn.Conv1d (stride 1, zero padding pad, dilation dil >= 1; model_resnet_dconv.py:98-100) on
 * CHANNELS-LAST activations: x [N][L][Ci], w [Co][Ci][K] (torch layout), bias [Co] (nullable),
 * y [N][Lo][Co] with Lo = L + 2 pad - dil (K - 1).  The same implicit GEMMs as above (H = 1, KH = 1) with
 * tap k gathered k * dil columns from tap 0, in fp32 and with bf16 / fp16 operands.
 * ws: srk_conv2d_workspace_floats(Ci, Co, 1, K) floats.  x16 / x16_written, dy16 and dw_accumulate mean
 * what they mean on srk_conv2d_nhwc_fwd16 / _bwd16_acc (all nullable / 0).  dil = 1 forwards to those entry
 * points (bitwise their results).  Backward writes dw [Co][Ci][K], db (nullable) and dx (nullable).
 * Checked on the host before any device work, SRK_ERR_INVALID with "dilation" in srk_last_error():
 * dil < 1, Lo < 1, a null x, w, y (fwd) / dy, dw (bwd) or ws.                                   */
int srk_conv1d_nlc_dil_fwd(const float* x, int64_t N, int64_t L, int64_t Ci, const float* w, const float* bias,
                           int64_t Co, int64_t K, int64_t pad, int64_t dil, float* y, float* ws,
                           void* x16, int* x16_written, void* stream);
int srk_conv1d_nlc_dil_bwd(const float* x, int64_t N, int64_t L, int64_t Ci, const float* w, int64_t Co, int64_t K,
                           int64_t pad, int64_t dil, const float* dy, const void* dy16, float* dx, float* dw,
                           float* db, float* ws, const void* x16, int dw_accumulate, void* stream);
/* Conv2d (stride 1) + bias + MaxPool2d((1, 4)) fused (model_fbanks_cnn.py:74-75,91-92: conv2 then
 * maxpool2): the implicit GEMM's epilogue pools its own output, so only the pooled activation y
 * [N][Ho][Wo/4][Co] and the uint8 window argmax [N][Ho][Wo/4][Co] (first maximum, NaN wins: the
 * maxpool rule) are written.  Needs pool_w = 4 dividing Wo.  x16 / x16_written as fwd16.  The
 * backward takes the POOLED gradient and the argmax (the dense gradient exists only in library
 * scratch) and gives what srk_conv2d_nhwc_bwd16 gives for the unpooled gradient.               */
int srk_conv2d_nhwc_fwd_pool(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w,
                             const float* bias, int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw,
                             int64_t pool_w, float* y, uint8_t* argmax, float* ws, void* x16, int* x16_written,
                             void* stream);
int srk_conv2d_nhwc_bwd_pool(const float* x, int64_t N, int64_t H, int64_t W, int64_t Ci, const float* w, int64_t Co,
                             int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t pool_w, const float* dy_pooled,
                             const uint8_t* argmax, float* dx, float* dw, float* db, float* ws, const void* x16,
                             void* stream);
/* Max pooling, window = stride = (kh, kw), floor mode, channels-last (nn.MaxPool2d((1,3)),
 * ((1,4)) and nn.MaxPool1d(98), model_fbanks_cnn.py:73,75,78).  Backward routes each gradient to
 * the first maximum of its window, as PyTorch does.                                          */
/* Fused first layer of model_fbanks_cnn (models/model_fbanks_cnn.py:72-73,89-90): Conv2d(1, 64,
 * (7,3), padding (3,1)) + bias + MaxPool2d((1,3)) in one pass.  x: [N, H, W] (one input channel);
 * y: pooled [N, H, W/3, 64] (NHWC); argmax: uint8 [N, H, W/3, 64] = position (0..2) of each window's
 * first maximum (PyTorch's rule, NaN wins).  Only that geometry is accepted (SRK_ERR_INVALID else).
 * The backward gives dW [64,1,7,3] and db [64] (db may be NULL) from the POOLED gradient dy and
 * argmax (the unpooled gradient is never formed); ws: srk_conv1_pool_workspace_floats() floats. */
int64_t srk_conv1_pool_workspace_floats(int64_t Co, int64_t KH, int64_t KW);
int srk_conv1_pool_fwd(const float* x, int64_t N, int64_t H, int64_t W, const float* w, const float* bias,
                       int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t pool, float* y,
                       uint8_t* argmax, void* stream);
/* As srk_conv1_pool_fwd, and in the 16-bit matmul modes also the pooled activation's bf16 / fp16 operand copy
 * (y16: N*H*(W/pool)*Co 16-bit elements, 8-byte aligned, or null), the one srk_conv2d_nhwc_fwd_pool accepts as
 * ready (x16_written = 2) instead of converting y again; *y16_written = 1 when it was written.  *y16_written = 3
 * on entry: the caller consumes only the copy, and y is left unwritten when the copy is written. */
int srk_conv1_pool_fwd16(const float* x, int64_t N, int64_t H, int64_t W, const float* w, const float* bias,
                         int64_t Co, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t pool, float* y,
                         uint8_t* argmax, void* y16, int* y16_written, void* stream);
int srk_conv1_pool_wgrad(const float* x, int64_t N, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                         int64_t ph, int64_t pw, int64_t pool, const float* dy, const uint8_t* argmax, float* dw,
                         float* db, float* ws, void* stream);
/* The data gradient of the same fused layer, for an input that carries a gradient (a trainable front-end such
 * as nn.PCEN before conv1): dx [N, H, W] = conv-transpose of the pooled gradient dy routed through argmax, with
 * the weights w [64,1,KH,KW]; gathered straight from dy and argmax (the unpooled gradient is never formed),
 * fixed summation order, fully written.  The two fused geometries with W % pool == 0 only (SRK_ERR_INVALID
 * else).  Profiler category "conv1_pool_dgrad".                                                          */
int srk_conv1_pool_dgrad(const float* w, int64_t N, int64_t H, int64_t W, int64_t Co, int64_t KH, int64_t KW,
                         int64_t ph, int64_t pw, int64_t pool, const float* dy, const uint8_t* argmax, float* dx,
                         void* stream);
int srk_maxpool_nhwc_fwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, int64_t kh, int64_t kw,
                         float* y, void* stream);
int srk_maxpool_nhwc_bwd(const float* x, const float* dy, int64_t N, int64_t H, int64_t W, int64_t C, int64_t kh,
                         int64_t kw, float* dx, void* stream);

/* ---------------------------------------------------------------- K9: batch norm (+ residual, ReLU)
 * nn.BatchNorm1d on channels-last x [M][C] (M = N * L), fused with an optional residual add and
 * ReLU: y = act((x - mean) * invstd * gamma + beta [+ residual]) (model_resnet_bgru.py:20-39,49).
 * training = 1: batch statistics (biased variance), running stats updated in place with
 * `momentum` (unbiased variance), as nn.BatchNorm1d; training = 0: running statistics.
 * save_mean / save_invstd [C] are written for the backward.  Backward takes the forward's y (for
 * the ReLU mask) and writes dx (nullable), dgamma, dbeta and dresidual (nullable).
 * Special values follow torch: ReLU keeps NaN (y = v <= 0 ? 0 : v, so -0.0 gives +0.0 and +inf stays);
 * gradient passes where !(y <= 0), i.e. y > 0 or NaN.  A non-finite x in training mode makes its
 * channel's statistics, running statistics and outputs non-finite, as nn.BatchNorm1d's.          */
int srk_batchnorm_fwd(const float* x, int64_t M, int64_t C, const float* gamma, const float* beta, float eps,
                      float momentum, int training, float* running_mean, float* running_var, const float* residual,
                      int relu, float* y, float* save_mean, float* save_invstd, void* stream);
int srk_batchnorm_bwd(const float* x, const float* y, const float* dy, int64_t M, int64_t C, const float* gamma,
                      const float* save_mean, const float* save_invstd, int training, int relu, float* dx,
                      float* dgamma, float* dbeta, float* dresidual, void* stream);
/* The same pair emitting the 16-bit operand copy of their output for the convolution that consumes it
 * (model_resnet_bgru.py: every conv reads a BatchNorm output, and every BatchNorm's dx is a conv's dY).
 * fwd16 writes y16 = y rounded to the bf16 / fp16 matmul precision (M*C 16-bit elements, 16-B aligned,
 * caller storage) beside y; bwd16 writes dx16 = dx rounded likewise; *_written = 1 when the copy was
 * written, else 0 (fp32 precision, null or misaligned pointer; dx16 also needs dx).  The rounding is
 * the convolutions' own (round to nearest even), so srk_conv2d_nhwc_fwd16 (x16_written = 2 on entry)
 * and srk_conv2d_nhwc_bwd16_dy16 use the copies bitwise as if they had made them.               */
int srk_batchnorm_fwd16(const float* x, int64_t M, int64_t C, const float* gamma, const float* beta, float eps,
                        float momentum, int training, float* running_mean, float* running_var, const float* residual,
                        int relu, float* y, void* y16, int* y16_written, float* save_mean, float* save_invstd,
                        void* stream);
int srk_batchnorm_bwd16(const float* x, const float* y, const float* dy, int64_t M, int64_t C, const float* gamma,
                        const float* save_mean, const float* save_invstd, int training, int relu, float* dx,
                        void* dx16, int* dx16_written, float* dgamma, float* dbeta, float* dresidual, void* stream);
/* The same, and dgamma_acc / dbeta_acc (nullable: the parameters' existing .grad) += dgamma / dbeta
 * (autograd's accumulation fused into the kernel that forms the sums; dgamma / dbeta stay outputs). */
int srk_batchnorm_bwd16_acc(const float* x, const float* y, const float* dy, int64_t M, int64_t C,
                            const float* gamma, const float* save_mean, const float* save_invstd, int training,
                            int relu, float* dx, void* dx16, int* dx16_written, float* dgamma, float* dbeta,
                            float* dresidual, float* dgamma_acc, float* dbeta_acc, void* stream);
/* The ReLU as bits: with relu set, fwd16_mask also writes relu_mask (M*C/4 bytes; byte i holds bit e = !(y[4i+e] <= 0):
 * y > 0 or NaN, nullable), and bwd16_mask takes that mask in place of y (y may then be null) — the backward's two reads of the
 * ReLU pattern are 1/16 of y's bytes.  Otherwise as fwd16 / bwd16_acc, whose results they equal bit for bit. */
int srk_batchnorm_fwd16_mask(const float* x, int64_t M, int64_t C, const float* gamma, const float* beta, float eps,
                             float momentum, int training, float* running_mean, float* running_var,
                             const float* residual, int relu, float* y, void* y16, int* y16_written,
                             uint8_t* relu_mask, float* save_mean, float* save_invstd, void* stream);
int srk_batchnorm_bwd16_mask(const float* x, const float* y, const uint8_t* relu_mask, const float* dy, int64_t M,
                             int64_t C, const float* gamma, const float* save_mean, const float* save_invstd,
                             int training, int relu, float* dx, void* dx16, int* dx16_written, float* dgamma,
                             float* dbeta, float* dresidual, float* dgamma_acc, float* dbeta_acc, void* stream);
/* SyncBatchNorm pieces (torch.nn.SyncBatchNorm semantics: training statistics over the global
 * batch of all data-parallel ranks; model_resnet_bgru.py's BatchNorm1d layers under DP).  Forward:
 * srk_batchnorm_stats (this rank's count, mean, M2 per channel -> stats [3][C]), the caller gathers
 * every rank's triple ([world][3][C], rank order), srk_batchnorm_combine (Chan's combination in rank
 * order: identical on every rank; running stats with the global unbiased variance; total_count [1]
 * = the global row count, nullable), then
 * srk_batchnorm_apply.  Backward: srk_batchnorm_bwd_reduce (this rank's sums [2][C] = sum g,
 * sum g * xhat, g = dy * act'(y): also its dbeta / dgamma contributions), the caller sums them over
 * ranks, srk_batchnorm_bwd_dx with the combine's total_count (device).  The C-ABI replaces the fused
 * srk_batchnorm_fwd / _bwd statistics step only; layouts as srk_batchnorm_fwd.                    */
int srk_batchnorm_stats(const float* x, int64_t M, int64_t C, float* stats, void* stream);
int srk_batchnorm_combine(const float* stats_all, int world, int64_t C, float eps, float momentum,
                          float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                          float* total_count, void* stream);
int srk_batchnorm_apply(const float* x, int64_t M, int64_t C, const float* save_mean, const float* save_invstd,
                        const float* gamma, const float* beta, const float* residual, int relu, float* y,
                        void* stream);
int srk_batchnorm_bwd_reduce(const float* x, const float* y, const float* dy, int64_t M, int64_t C,
                             const float* save_mean, const float* save_invstd, int relu, float* sums, void* stream);
int srk_batchnorm_bwd_dx(const float* x, const float* y, const float* dy, int64_t M, int64_t C,
                         const float* total_count, const float* gamma, const float* save_mean,
                         const float* save_invstd, const float* sums, int relu, float* dx, float* dresidual,
                         void* stream);

/* ---------------------------------------------------------------- K7/K8: step ops
 * Cross-entropy, mean over the batch (nn.CrossEntropyLoss, training.py:73,87):
 * loss[0] = mean_b(logsumexp(logits_b) - logits_b[label_b]); dlogits (nullable) =
 * (softmax - onehot) / B.  ws: B + 1 floats.  An out-of-range label makes the loss NaN.  It is
 * srk_cross_entropy_mix's kernel without a mix and without smoothing, under its own error texts. */
int srk_cross_entropy(const float* logits, const int64_t* labels, int64_t B, int64_t C, float* loss,
                      float* dlogits, float* ws, void* stream);
/* torch.optim.Adam step (no weight decay / amsgrad) over n contiguous floats (training.py:74,91);
 * step is the 1-based step count after increment; grad is multiplied by grad_scale first.  The
 * four Adam entries run one update (srk_adamw_step says what it computes); this one takes lr and
 * the step count from the host.                                                              */
int srk_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, int64_t step, float grad_scale, void* stream);
/* The same step with its per-step values on the device, so a captured HIP graph can replay it:
 * state is a 4-int64 (32-B) device buffer — int64 step, then floats bc1, sqrt(bc2), lr, 0.  The
 * caller writes lr (float, byte offset 16); the call advances the step and derives the bias
 * corrections on the device (double precision, as srk_adam_step's host side).  It is
 * srk_adamw_step without a scaler and with decay, clipping and the EMA off; n == 0 returns before
 * any launch.                                                                                     */
int srk_adam_step_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                        float beta2, float eps, int64_t* state, float grad_scale, void* stream);
/* Loss scaling for 16-bit training (torch.cuda.amp.GradScaler semantics, on the device so a
 * captured step replays it).  scaler: 8 x 32-bit device words {float scale, float 1/scale, float
 * growth, float backoff, int found_inf, int good_steps, int growth_interval, int overflows};
 * growth_interval 0 = static scale.  The caller multiplies the loss by scale (word 0) before
 * backward.  No reference counterpart: the reference trains fp32 only (training.py:85-91).       */
int srk_grad_scaler_init(int32_t* scaler, float init_scale, float growth_factor, float backoff_factor,
                         int growth_interval, void* stream);
/* The step on loss-scaled gradients (srk_adamw_step with a scaler and decay, clipping and the EMA
 * off; with n == 0 the step count and the scaler still advance): one pass flags any non-finite
 * gradient element;
 * if one is found the step is SKIPPED (parameters, moments and the step count unchanged), the
 * overflow counter (word 7) advances and a dynamic scale backs off; otherwise the gradients are
 * multiplied by grad_scale / scale inside the update and a dynamic scale grows after
 * growth_interval clean steps.                                                                    */
int srk_adam_step_scaled(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                         float beta2, float eps, int64_t* state, float grad_scale, int32_t* scaler, void* stream);
/* Floats of workspace srk_adamw_step needs while clipping is on: one partial sum per workgroup of the gradient-norm
 * pass, whose grid depends on n alone (min(ceil(n / 1024), 1024), at least 1).  0 for n < 0.             */
int64_t srk_adamw_workspace_floats(int64_t n);
/* The Adam step with every per-step value on the device: a loss scaler (nullable), decoupled weight decay,
 * global-norm gradient clipping and an exponential moving average of the weights, all optional:
 *   norm    (clipping on, or a scaler) one read of grad: total_norm = sqrt(sum (grad[i] * s)^2), s = grad_scale
 *           [/ scale], summed in a fixed order (same n and bits in, same bits out; no atomics on floats), and the
 *           scaler's found_inf raised on a non-finite element in the same read (a scaler without clipping: that
 *           check alone);
 *   prep    coef = min(1, max_norm / (total_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_); clip_state, 16 B
 *           on the device {float total_norm, float coef, int32 clipped_steps, int32 0}, is written; clipped_steps
 *           advances on a step that is not skipped and has coef < 1; the step count advances as in the others;
 *   update  one pass: a skipped step (scaler overflow) writes nothing; else gg = grad * s * coef; where
 *           decay_mask marks the element's 64-float chunk (one byte per chunk, ceil(n / 64) bytes; NULL = every
 *           chunk) param *= 1 - lr * weight_decay (torch.optim.AdamW, lr from state); then torch.optim.Adam's
 *           update, m = b1 m + (1 - b1) gg, v = b2 v + (1 - b2) gg^2, param -= (lr / bc1) m / (sqrt(v) / sqrt(bc2)
 *           + eps), every rounding fixed by the kernel's source (not by the compiler's contraction); then
 *           ema = ema_decay * ema + (1 - ema_decay) * param where ema (n floats) is given.
 * max_norm <= 0 or +inf: clipping off (clip_state and ws are not touched and may be NULL); weight_decay == 0: no
 * decay; ema NULL: no average.  srk_adam_step_state and srk_adam_step_scaled are this call with all three off
 * (the same launches, the same bits).  ws: srk_adamw_workspace_floats(n) floats, fully written before they are read.
 * Checked on the host before any device work, SRK_ERR_INVALID with "adamw" and the argument's name in
 * srk_last_error(): n < 0; state NULL; param / grad / exp_avg / exp_avg_sq NULL with n > 0; param, grad, exp_avg,
 * exp_avg_sq, ema off 16 bytes, state off 8, scaler / clip_state / ws off 4; weight_decay negative or not finite;
 * max_norm NaN; clip_state or ws NULL while clipping is on; ema given with ema_decay outside [0, 1) or aliasing
 * another buffer.                                                                                          */
int srk_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float beta1,
                   float beta2, float eps, int64_t* state, float grad_scale, int32_t* scaler, float weight_decay,
                   const uint8_t* decay_mask, float max_norm, int32_t* clip_state, float* ema, float ema_decay,
                   float* ws, void* stream);
/* nn.Dropout(p) training forward: keep[i] = Bernoulli(1-p) from a counter-based hash of
 * (seed, i) (not torch's RNG stream), y = keep ? x / (1-p) : 0.                              */
int srk_dropout_fwd(const float* x, int64_t n, float p, uint64_t seed, float* y, uint8_t* keep, void* stream);
/* srk_dropout_fwd with its seed on the device: state = uint64[2] {base, counter}; the mask hashes
 * base + counter * odd constant, then the call advances state[1] (graph-replayable; nn.Dropout,
 * model_fbanks_cnn.py:79,98).                                                                    */
int srk_dropout_fwd_state(const float* x, int64_t n, float p, uint64_t* state, float* y, uint8_t* keep,
                          void* stream);
/* n float64 draws from U[lo, hi) with the seed on the device (graph-replayable, as srk_dropout_fwd_state;
 * the VTLP warp factors, legacy/model_8/dataset_top.py:251): state = uint64[2] {base, counter},
 * seed = base + 0xD1B54A32D192ED03 * counter; out[i] = lo + (hi - lo) * u_i (two roundings) with
 * u_i = (z >> 11) * 2^-53, z = the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (i + 1); then the
 * call advances state[1].  out: float64 [n] on the device.                                      */
int srk_uniform_f64_state(uint64_t* state, double lo, double hi, int64_t n, double* out, void* stream);
/* y = keep ? x * scale : 0 (dropout with an explicit keep-mask; also its backward).          */
int srk_dropout_apply(const float* x, const uint8_t* keep, int64_t n, float scale, float* y, void* stream);

/* ---------------------------------------------------------------- attention pooling over time
 * A query scores every step of a sequence, a softmax over time weights them, the weighted sum is the
 * context (nn.AttentionPool over a BiGRU's output; no reference counterpart):
 *   s[b,t] = scale * <q[b,:], y[b,t,:]>, alpha[b,:] = softmax_t(s[b,:]) (max-subtracted),
 *   ctx[b,:] = sum_t alpha[b,t] * y[b,t,:].
 * y [B][T][D] contiguous, q / ctx / dctx / dq [B][D], alpha [B][T]; fp32 at every matmul precision.
 * Backward, g = dctx: a_t = <g, y_t>, m = sum_t alpha_t a_t, ds_t = alpha_t (a_t - m),
 *   dq = scale * sum_t ds_t y_t, dy_t = alpha_t g + scale * ds_t q   (dy fully written, not accumulated;
 *   alpha is an output only: no gradient flows into it).
 * One workgroup per clip, one launch per call; every reduction has a fixed order and there are no
 * floating-point atomics, so equal inputs give equal bits (eagerly and from a replayed graph).
 * T <= 64 and D <= 1024 with D % 4 == 0 and 16-byte aligned tensors keep the clip in registers (y is read
 * once); other shapes take two passes over y, the second one out of the caches, with scalar accesses when
 * D % 4 != 0 (srk_set_option "attn_pool_regs", default 1; 0 = always two passes: A/B measurements and tests).
 * Checked on the host before any device work, SRK_ERR_INVALID with "attn_pool" in srk_last_error():
 * B < 1, T outside 1..1024, D outside 1..4096, a scale that is not finite, any null tensor.
 * Profiler category "attn_pool" (one record per launch, with its algorithmic bytes).            */
int srk_attn_pool_fwd(const float* y, const float* q, int64_t B, int64_t T, int64_t D, float scale, float* ctx,
                      float* alpha, void* stream);
int srk_attn_pool_bwd(const float* y, const float* q, const float* alpha, const float* dctx, int64_t B, int64_t T,
                      int64_t D, float scale, float* dy, float* dq, void* stream);

/* ---------------------------------------------------------------- per-channel energy normalisation
 * Trainable PCEN (Wang et al., ICASSP 2017; nn.PCEN over K2's [B][98][120] dB output; no reference
 * counterpart): each band is divided by a smoothed version of its own recent energy and root-compressed,
 * every constant learned per band.  Per clip b, frame t, channel c, raw parameters p [4][C]:
 *   alpha = exp(p[0][c]), delta = exp(p[1][c]), r = exp(p[2][c]), s = sigmoid(p[3][c]),
 *   E[t] = exp(log_scale * x[t]) (log_scale != 0; ln(10)/20 for dB input) or x[t] (log_scale == 0),
 *   M[0] = E[0], M[t] = (1 - s) M[t-1] + s E[t],
 *   u = eps + M[t], g = E[t] u^-alpha, v = g + delta, y[t] = v^r - delta^r.
 * x / y / m / dy / dx [B][T][C] contiguous, p / dp [4][C]; fp32 at every matmul precision.
 * Backward, dy given: dv = dy r v^(r-1); d_r = sum dy (v^r ln v - delta^r ln delta);
 *   d_delta = sum (dv - dy r delta^(r-1)); d_alpha = sum dv g (-ln u); du = -alpha dv g / u;
 *   reverse scan G[T] = 0, G[t] = du[t] + (1 - s) G[t+1]; dE[t] = dv u^-alpha + s G[t] (t >= 1),
 *   dE[0] = dv u^-alpha + G[0]; d_s = sum_{t >= 1} G[t] (E[t] - M[t-1]); dx = dE E log_scale (or dE);
 *   dp = [d_alpha alpha, d_delta delta, d_r r, d_s s (1 - s)], the sums over b and t: the gradient with
 *   respect to the RAW parameters, written, not accumulated.
 * One thread per (clip, channel) column.  The forward is one launch (m_out == NULL: M is not written, for
 * evaluation); the backward is the reverse scan (dx == NULL: not written) plus one small launch that sums
 * the columns' parameter sums in ws (srk_pcen_workspace_floats floats) over the clips and applies the chain
 * rule.  Every sum has a fixed order and there are no floating-point atomics, so equal inputs give equal
 * bits (eagerly and from a replayed graph).
 * Checked on the host before any device work, SRK_ERR_INVALID with "pcen" in srk_last_error():
 * B < 1, T outside 1..1024, C outside 1..1024, B T C >= 2^31, eps not finite or <= 0, log_scale not
 * finite, any required pointer null.
 * Profiler category "pcen" (one record per launch, with its algorithmic bytes).                     */
int64_t srk_pcen_workspace_floats(int64_t B, int64_t T, int64_t C);
int srk_pcen_fwd(const float* x, const float* p, int64_t B, int64_t T, int64_t C, float log_scale, float eps,
                 float* y, float* m_out /* [B][T][C] or NULL */, void* stream);
int srk_pcen_bwd(const float* x, const float* p, const float* m, const float* dy, int64_t B, int64_t T, int64_t C,
                 float log_scale, float eps, float* dx /* or NULL */, float* dp /* [4][C], written not accumulated */,
                 float* ws, void* stream);

/* ---------------------------------------------------------------- depthwise convolution / global average pool
 * The two primitives of a depthwise-separable CNN block that K6 lacks (nn.DepthwiseConv2d, nn.GlobalAvgPool2d; the
 * fbanks_dscnn plugin; no reference counterpart).  All tensors fp32, channels-last, contiguous; fp32 arithmetic at
 * every matmul precision (there is no GEMM in a depthwise conv).  Lanes run along C: 16-byte loads / stores of 4
 * channels when C % 4 == 0 and the pointers are 16-byte aligned, a scalar path otherwise (csrc/dwconv.hip).
 *
 * Depthwise nn.Conv2d (groups = C, channel multiplier 1, zero padding, no dilation):
 * x [N][H][W][C], w [C][1][KH][KW] (the torch state_dict tensor), bias [C] nullable,
 * y [N][Ho][Wo][C], Ho = (H + 2ph - KH)/sh + 1, Wo likewise:
 *   y[n][ho][wo][c] = bias[c] + sum_{kh,kw} w[c][kh][kw] x[n][ho sh - ph + kh][wo sw - pw + kw][c].
 * Backward: dx (NULL: not computed) in the gather form — every element sums the taps whose output position
 * exists, written once in full, no zero fill, no atomics; dw[c][kh][kw] = sum_{n,ho,wo} dy x and
 * db[c] = sum dy (NULL: not written) as per-thread register partials, a per-workgroup LDS sum, per-workgroup
 * slabs in ws (srk_dwconv2d_workspace_floats floats) and a second launch that sums the slabs in a fixed order;
 * with dw_accumulate != 0 that launch ADDS into dw (a FlatParams-owned .grad, the convention of
 * srk_conv2d_nhwc_bwd16_acc), otherwise it writes it; db is always written.  Equal inputs give equal bits.
 * Domain: 1 <= KH, KW <= 7; sh, sw in {1, 2}; 0 <= ph < KH, 0 <= pw < KW; Ho, Wo >= 1; N, H, W, C >= 1; every
 * tensor below 2^31 elements.  Anything else, a null required pointer or a null ws is refused on the host before
 * any device work: SRK_ERR_INVALID with "dwconv" in srk_last_error() (srk_dwconv2d_workspace_floats returns 0).
 *
 * Global average pool: x [N][HW][C] -> y [N][C] = the mean over the HW positions of each clip (summed in a fixed
 * order, divided by HW); dx = dy / HW broadcast.  N, HW, C >= 1, N HW C < 2^31, else SRK_ERR_INVALID with
 * "avgpool" in srk_last_error().
 * Every launch is on the given stream, with no host synchronisation and no allocation.
 * Profiler categories "dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad" (both launches) and "avgpool".       */
int64_t srk_dwconv2d_workspace_floats(int64_t N, int64_t H, int64_t W, int64_t C, int64_t KH, int64_t KW,
                                      int64_t ph, int64_t pw, int64_t sh, int64_t sw);
int srk_dwconv2d_nhwc_fwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, const float* w,
                          const float* bias, int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw,
                          float* y, void* stream);
int srk_dwconv2d_nhwc_bwd(const float* x, int64_t N, int64_t H, int64_t W, int64_t C, const float* w,
                          int64_t KH, int64_t KW, int64_t ph, int64_t pw, int64_t sh, int64_t sw, const float* dy,
                          float* dx /* or NULL */, float* dw, float* db /* or NULL */, float* ws,
                          int dw_accumulate, void* stream);
int srk_avgpool_nhwc_fwd(const float* x, int64_t N, int64_t HW, int64_t C, float* y, void* stream);
int srk_avgpool_nhwc_bwd(const float* dy, int64_t N, int64_t HW, int64_t C, float* dx, void* stream);

/* ---------------------------------------------------------------- transformer encoder pieces
 * The three layers of a transformer encoder that are not a GEMM (nn.MultiheadSelfAttention, nn.LayerNorm, nn.GELU;
 * the fbanks_kwt plugin; no reference counterpart).  All tensors fp32 and contiguous, fp32 arithmetic at every matmul
 * precision.  Every sum has a fixed order and there are no floating-point atomics, so equal inputs give equal bits
 * (eagerly and from a replayed graph).  Every launch is on the given stream, with no host synchronisation and no
 * allocation.  Arguments are checked on the host before any device work: SRK_ERR_INVALID with the family's name
 * ("mhsa", "layernorm", "gelu") in srk_last_error() for a null required pointer, a size outside the domain or a
 * tensor of 2^31 elements or more.  A tensor whose base is not 16-byte aligned (or, LayerNorm, a D that is not a
 * multiple of 4) takes scalar accesses instead of float4 ones.  Profiler categories "mhsa", "layernorm", "gelu": one
 * record per call with its algorithmic bytes.
 *
 * Multi-head self-attention core (csrc/mhsa.hip), per clip b and head h:
 *   S = scale Q K^T,  P = softmax over each row of S (row maximum subtracted),  O = P V.
 * qkv [B][T][3 D], D = H dh, is the packed projection as a Linear writes it, torch's in_proj order: columns [0, D)
 * q, [D, 2D) k, [2D, 3D) v, head h owning columns h dh .. (h + 1) dh - 1 of each third.  o [B][T][D] has the heads
 * side by side.  The forward also writes lse [B][H][T], each row's log-sum-exp of S: all the backward keeps (P is
 * recomputed as exp(S - lse); o is not read: rowsum(dO o O) = sum_j P_ij dP_ij).  The backward writes
 * dqkv [B][T][3 D] in the packed layout: dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dO o O)),
 * dQ = scale dS K, dK = scale dS^T Q.  Domain: B, H >= 1, 1 <= T <= 128, dh % 4 == 0, 4 <= dh <= 64, a finite scale,
 * B T 3 D < 2^31.  No workspace.                                                                       */
int srk_mhsa_fwd(const float* qkv, int64_t B, int64_t H, int64_t T, int64_t dh, float scale, float* o, float* lse,
                 void* stream);
int srk_mhsa_bwd(const float* qkv, const float* lse, const float* d_o, int64_t B, int64_t H, int64_t T, int64_t dh,
                 float scale, float* dqkv, void* stream);
/* LayerNorm over the last dimension of [M][D] (csrc/layernorm.hip):  s = x + res (res NULL: s = x),
 *   y = (s - mean) rstd gamma + beta,  rstd = 1 / sqrt(var + eps), var the biased variance, computed as the mean of
 * the centred squares after the mean.  mean and rstd [M] are saved for the backward, which recomputes s from x and
 * res and writes ds [M][D] (the gradient of x and of res alike) and dgamma, dbeta [D]:
 *   out = acc_beta * out + sum  (acc_beta 0: written without being read), the sum formed from per-workgroup partials
 * in ws (srk_layernorm_workspace_floats floats, every word written before it is read) added in a fixed order (runs of
 * consecutive partials in index order, then the runs in index order).
 * Domain: M >= 1, 1 <= D <= 1024, M D < 2^31, eps finite and >= 0 (srk_layernorm_workspace_floats returns 0
 * outside it).                                                                                          */
int64_t srk_layernorm_workspace_floats(int64_t M, int64_t D);
int srk_layernorm_fwd(const float* x, const float* res /* or NULL */, const float* gamma, const float* beta,
                      int64_t M, int64_t D, float eps, float* y, float* mean, float* rstd, void* stream);
int srk_layernorm_bwd(const float* x, const float* res /* or NULL */, const float* gamma, const float* mean,
                      const float* rstd, const float* dy, int64_t M, int64_t D, float* ds, float* dgamma,
                      float* dbeta, float acc_beta, float* ws, void* stream);
/* GELU, erf form (csrc/gelu.hip; torch's default): y = x Phi(x), dx = dy (Phi(x) + x phi(x)), the backward reading
 * x.  NaN propagates; every finite x gives finite y and dx.  1 <= n < 2^31.                            */
int srk_gelu_fwd(const float* x, int64_t n, float* y, void* stream);
int srk_gelu_bwd(const float* x, const float* dy, int64_t n, float* dx, void* stream);

/* ---------------------------------------------------------------- SpecAugment on a feature map
 * Time warp, frequency masks and time masks (Park et al., Interspeech 2019) on a batch of feature clips, the
 * random draws made explicit and drawn on the device (features.spec_augment / specaug_draw; no reference
 * counterpart).  All tensors fp32 and contiguous; a clip is [T][F] with time_major = 1 (what every plugin feeds its
 * network) or [F][T] with time_major = 0 (the layout of K1 layout 0 and K3 transposed 0).
 *
 * params: int32 [B][P] on the device, P = 2 + 2 NF + 2 NT, 0 <= NF, NT <= 4; clip b holds
 *   {c, w, f0_0, fw_0, .., f0_{NF-1}, fw_{NF-1}, t0_0, tw_0, .., t0_{NT-1}, tw_{NT-1}}.
 *
 * srk_specaug_apply computes per clip, in this order (y may be x: in place):
 *  1. the fill value: fill_value (fill_mode 0), or the mean of the clip's T F input elements (fill_mode 1; fp32,
 *     summed in a fixed order that does not depend on the layout, no floating-point atomics);
 *  2. the time warp that moves frame c to frame w: output frame t reads source position s(t), an exact rational,
 *       s = t c / w (t <= w),   s = c + (t - w)(T - 1 - c) / (T - 1 - w) (t > w);
 *     with i = floor(s) and a = frac(s) = (float)(num % den) / (float)den: a == 0 copies x[i] bit for bit and reads
 *     nothing else, otherwise x[i] + a (x[i+1] - x[i]) in fp32 (three roundings, no contraction).  c == w is the
 *     identity: every frame a bit-exact copy;
 *  3. the masks: an element whose feature index lies in any [f0_j, f0_j + fw_j) or whose frame lies in any
 *     [t0_j, t0_j + tw_j) becomes the fill value.  Width 0 masks nothing; masks may overlap.
 * Valid parameters: c == w with both in [0, T-1], or both c and w in [1, T-2]; f0, fw >= 0 and f0 + fw <= F;
 * t0, tw >= 0 and t0 + tw <= T.  The parameters live on the device (no host check): the kernel validates a clip's
 * row before it reads anything through it, and a clip with an invalid row gets NaN in its whole output (K2-VTLP's
 * convention); the other clips are unaffected and no out-of-range address is formed.
 * One launch, one workgroup per clip, the clip staged in LDS: one HBM read and one write per element, both along
 * the contiguous axis in either layout, 16-byte accesses when T F % 4 == 0 and x, y are 16-byte aligned (a scalar
 * path otherwise).  Domain: T F <= SRK_SPECAUG_MAX_ELEMS.
 * Checked on the host before any device work, SRK_ERR_INVALID with "specaug" in srk_last_error(): T F above the
 * constant, B < 1, T or F < 1, NF or NT outside 0..4, a fill_mode other than 0 or 1, a fill_value that is not
 * finite, a null pointer.  Profiler category "specaug" (one record per launch, with its algorithmic bytes).
 *
 * srk_specaug_draw draws the parameters of B clips on the device (one launch, graph-replayable) from the state and
 * hash of srk_uniform_f64_state: state = uint64[2] {base, counter}, seed = base + 0xD1B54A32D192ED03 * counter,
 * z_i = the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (i + 1), r_i(n) = ((z_i >> 32) * n) >> 32, an exact
 * integer in [0, n).  Clip b uses i = b P + k, k in this order:
 *   k = 0: c = W + 1 + r(T - 2W - 2);   k = 1: w = c - W + r(2W + 1)   (W == 0: c = w = 0);
 *   k = 2 + 2j: fw_j = r(f_max + 1);    k = 3 + 2j: f0_j = r(F - fw_j + 1);
 *   k = 2 + 2NF + 2j: tw_j = r(t_max + 1);   k = 3 + 2NF + 2j: t0_j = r(T - tw_j + 1)
 * (a width is drawn before its start and stored after it); then the call advances state[1] by one.  Every drawn row
 * is valid for srk_specaug_apply.  The host refuses, as above: W < 0, W > 0 with T < 2W + 3, f_max outside [0, F],
 * t_max outside [0, T], B, T or F < 1 (or T, F above 2^30), NF or NT outside 0..4, a null pointer.               */
#define SRK_SPECAUG_MAX_ELEMS 15840   /* 98 x 120, 49 x 321, 51 x 39 and 98 x 40 fit; the staged clip is <= 62 KB */
int srk_specaug_apply(const float* x, int64_t B, int64_t T, int64_t F, int time_major, const int32_t* params,
                      int NF, int NT, int fill_mode, float fill_value, float* y, void* stream);
int srk_specaug_draw(uint64_t* state, int64_t B, int64_t T, int64_t F, int W, int NF, int f_max, int NT, int t_max,
                     int32_t* params_out, void* stream);

/* ---------------------------------------------------------------- mixup and label smoothing
 * Mixup (Zhang et al., ICLR 2018) on the PCM a training step receives, and the soft-target cross-entropy that goes
 * with it (features.mixup_draw / mixup, nn.CrossEntropyLoss(label_smoothing)(.., mix=); no reference counterpart).
 * Clip b is mixed with clip partner[b] at weight lam[b]; both arrays are ordinary device arrays (int32 [B],
 * float [B]) that the draw fills and the apply and the loss read.
 *
 * srk_mixup_draw draws them on the device (one launch, graph-replayable) from the state and hash of
 * srk_uniform_f64_state: state = uint64[2] {base, counter}, seed = base + 0xD1B54A32D192ED03 * counter,
 * z_i = the splitmix64 finaliser of seed + 0x9E3779B97F4A7C15 * (i + 1), u_i = (z_i >> 11) * 2^-53.
 *  - lam[b] ~ Beta(alpha, alpha) by Joehnk's method, at most SRK_MIXUP_TRIALS trials: trial k takes
 *    U = u_{(32 b + k) 2} and V = u_{(32 b + k) 2 + 1}, X = pow(U, 1 / alpha), Y = pow(V, 1 / alpha), S = X + Y
 *    (all double; at alpha == 1, X = U and Y = V exactly); the first k with 0 < S <= 1 is accepted: l = X / S, then
 *    l = max(l, 1 - l) (a clip dominates its own mix), lam[b] = (float)l.  No trial accepted: lam[b] = 1.
 *  - one rotation for the batch: r = 1 + (((z_j >> 32) * (B - 1)) >> 32) with j = 64 B, partner[b] = (b + r) % B:
 *    a bijection without a fixed point.  B == 1: partner[0] = 0 and lam[0] = 1.
 * Then the call advances state[1] by one.  Acceptance is 1/2 per trial at alpha = 1 and higher below it, and pow
 * cannot underflow to a denormal down to alpha = 0.1: the domain is 0.1 <= alpha <= 1.
 * The host refuses, SRK_ERR_INVALID with "mixup" in srk_last_error(): B < 1, B > 2^24, alpha outside [0.1, 1] or not
 * finite, a null pointer.  Profiler category "mixup_draw".
 *
 * srk_mixup_apply: x, out fp32 [B][n] contiguous, out of place,
 *   out[b][i] = fl(lam_b * x[b][i]) + fl(w_b * x[partner_b][i]),   w_b = fl(1 - lam_b)
 * (fp32, four roundings, no contraction).  Any values are accepted (self, duplicates, lam anywhere in [0, 1]); they
 * live on the device (no host check): the kernel validates a row before it reads through it, and a row whose
 * partner is outside [0, B) or whose lam is not in [0, 1] (NaN included) gets NaN in its whole output row; no
 * out-of-range address is formed and the other rows are unaffected.  One launch, two reads and one write per
 * element (12 B n bytes), 16-byte accesses when n % 4 == 0 and x, out are 16-byte aligned (a scalar path
 * otherwise).  The host refuses, "mixup" in srk_last_error(): out overlapping x, B < 1, n < 1 (or above 2^31 - 1, or
 * more than 2^31 - 1 workgroups), a null pointer.  Profiler category "mixup" (one record per launch, 12 B n bytes).
 *
 * srk_cross_entropy_mix is srk_cross_entropy on the soft target of a mixed and / or smoothed batch.  partner and lam
 * are both NULL (label smoothing alone: lam_b = 1) or both given; with q_b = labels[partner_b] and eps = smoothing,
 *   t[b][c] = (1 - eps) (lam_b [c == y_b] + (1 - lam_b) [c == q_b]) + eps / C
 * (torch's label_smoothing on the mixed target), loss[0] = mean_b(logsumexp(z_b) - sum_c t[b][c] z[b][c]), dlogits
 * (nullable) = (softmax - t) / B.  ws: B + 1 floats; one row kernel and one deterministic mean serve both entries
 * (srk_cross_entropy passes no mix and no smoothing), so with partner == lam == NULL and smoothing == 0 loss and
 * dlogits are srk_cross_entropy's bits.  An
 * out-of-range label (a row's own or its partner's), a partner outside [0, B) or a lam not in [0, 1] makes that
 * row's loss, and so the loss, NaN.  The host refuses, "cross_entropy" in srk_last_error(): smoothing outside
 * [0, 1) or not finite, a shape outside srk_cross_entropy's domain (or B >= 2^31), exactly one of partner / lam
 * NULL, a null pointer.                                                                                          */
#define SRK_MIXUP_TRIALS 32
int srk_mixup_draw(uint64_t* state, int64_t B, double alpha, int32_t* partner, float* lam, void* stream);
int srk_mixup_apply(const float* x, int64_t B, int64_t n, const int32_t* partner, const float* lam, float* out,
                    void* stream);
int srk_cross_entropy_mix(const float* logits, const int64_t* labels, const int32_t* partner, const float* lam,
                          int64_t B, int64_t C, float smoothing, float* loss, float* dlogits, float* ws,
                          void* stream);

/* ---------------------------------------------------------------- diagnostics (tests only)
 * Directed checks of two instruction patterns (csrc/diag.hip; tests/test_diag_gpu.py):
 * srk_diag_acc_store: the row-staged data gradient's epilogue (raw buffer stores of 32x32 MFMA
 *   accumulators, its descriptor, offsets and drop value) into dx [rows][40][64] fp32 (rows % 8 == 0):
 *   tile g's first 32 pixels get 1 + 64 p + c + 2048 g; variant 0 = the product form, 1 = the round-5
 *   source form (a bit cast of a vector-component lvalue, miscompiled to component 0).
 * srk_diag_tr16_read: ds_read_b64_tr_b16 B fragments of a [32 k][cols] 16-bit matrix m staged as the
 *   64-column (cols = 64) or the 128-column TR image: out[(fragment * 64 + lane) * 4 + d], fragments
 *   (r0 = 0, 32, ...) x (kk = 0, 16). */
int srk_diag_acc_store(float* dx, int64_t rows, int variant, void* stream);
int srk_diag_tr16_read(const uint16_t* m, int64_t cols, uint32_t* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SRK_H_ */
