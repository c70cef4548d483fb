/*
 * fsn_hip.h - C ABI of libfsn_hip.so, the MI355X (gfx950) implementation of the FullSubNet
 * enhancement path.  Every entry point replaces one call site of the reference (cited as
 * path:line relative to the Audio-WestlakeU/FullSubNet checkout); INTEGRATION.md shows the
 * ctypes binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - all pointers are DEVICE pointers to contiguous fp32 arrays owned by the caller (PyTorch's
 *     caching allocator in practice); the library never allocates device memory;
 *   - `stream` is a hipStream_t passed as void*; work is enqueued and the call returns at once.  The
 *     device the stream belongs to is made current for the duration of the call (and restored), so one
 *     process may drive several GPUs.  The only state the library keeps is one small record per
 *     (device, stream) - an auxiliary stream with fork / join events for the left-over sub-band tiles and
 *     the profiler's events - so calls on DIFFERENT streams (from one or several host threads) are
 *     independent; calls that share a stream must be issued one at a time, like any stream-ordered API;
 *   - return value 0 = OK, < 0 = error; fsn_last_error() gives the thread-local message;
 *   - tensor shapes use the reference's names: B batch, L samples, F = n_fft/2+1 bins,
 *     T = 1 + L/hop frames, la = look_ahead.
 */
#ifndef FSN_HIP_H
#define FSN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSN_OK 0
#define FSN_ERR_ARG (-1)       /* bad shape / null pointer / unsupported configuration */
#define FSN_ERR_WORKSPACE (-2) /* workspace too small                                  */
#define FSN_ERR_LAUNCH (-3)    /* hipLaunch / hipMemsetAsync failed                    */
#define FSN_ERR_TIMEOUT (-4)   /* a persistent kernel ran out of time (see "residency contract" below) */

#define FSN_NORM_OFFLINE_LAPLACE 0    /* audio_zen/model/base_model.py:204-218 */
#define FSN_NORM_CUMULATIVE_LAPLACE 1 /* audio_zen/model/base_model.py:221-251 */
#define FSN_NORM_OFFLINE_GAUSSIAN 2   /* audio_zen/model/base_model.py:295-310 (fsn_norm only) */
#define FSN_NORM_CUMULATIVE_LAYER 3   /* audio_zen/model/base_model.py:312-354 (fsn_norm only) */
#define FSN_NORM_FORGETTING 4         /* audio_zen/model/base_model.py:103-151 (fsn_norm only) */

/* Arithmetic of the three large sub-band kernels.  F32 (the default, what every parity claim and bench.py's
 * `value` refer to): v_mfma_f32_16x16x4_f32, bit-equal to an fmaf chain.  F16X3: opt-in experiment - fp32
 * operands split into two fp16 halves, three 16-bit MFMAs per product block, fp32 accumulation. */
#define FSN_ARITH_F32 0
#define FSN_ARITH_F16X3 1
/* Training entries only (fsn_lstm2_forward_train / fsn_lstm2_backward): the arithmetic of torch.autocast, which the
 * reference trains under (fullsubnet/trainer.py:56, train.toml:5 use_amp = true) - both operands of every LSTM
 * product are rounded to fp16 / bf16 at the matrix core's input, accumulation and everything stored stay fp32. */
#define FSN_ARITH_F16 2
#define FSN_ARITH_BF16 3
/* Flag for the `arith` argument of fsn_lstm2_forward_train / fsn_lstm2_backward(_phase) / their workspace queries, OR-ed to
 * FSN_ARITH_F16 / _BF16 (the SAME value must reach the forward and the backward call of a step): the activated gates the
 * backward pass re-reads are saved in the arithmetic's 16-bit type instead of fp32 - what the vendor LSTM the reference
 * trains on keeps in its reserve space under autocast (fullsubnet/trainer.py:56) - inside the same save buffers; the cell
 * sequence, the hidden sequences and every gradient stay fp32.  Takes effect where the 16-bit arithmetic's own kernels run
 * BOTH directions (lstm_group16_kernels.hip; field 12 of fsn_debug_lstm2_plan16); ignored elsewhere, where the saves and
 * every result are those of the call without the flag.  Half the save traffic of the two persistent launches. */
#define FSN_ARITH_SAVES16 0x100

const char* fsn_last_error(void);
/* The ABI revision this header describes.  fsn_version() returns the revision the LIBRARY was built with: a caller
 * compares the two once after loading (fullsubnet_amd/_lib.py raises on a mismatch) - argument lists changed between
 * revisions (116: + fsn_lstm_layer_plan_rows; 115: + fsn_train_rows_pieces; 114: + fsn_lstm2_train_is_persistent; 113: + fsn_gru2_forward; 112: + FSN_ARITH_SAVES16; 111: + the composed families' glue entries; 110: fsn_train_dims.norm, fsn_train_den_elems; 100 -> 101 of round 4: fsn_clip_adam_step's found_inf). */
#define FSN_ABI_VERSION 118
int fsn_version(void);

/* ---- STFT / iSTFT : audio_zen/acoustics/feature.py ------------------------------------- */

/* feature.py:9-50  stft(y, n_fft, hop, win) -> (mag, phase, real, imag); phase is never used on
 * the path (inferencer.py:132 discards it) and is not produced.
 * y [B, L];  window [n_fft] (torch.hann_window(n_fft), feature.py:38);  real/imag/mag [B, F, T],
 * any of the three may be NULL.  win_length == n_fft; n_fft = 512 / hop = 256 (every FullSubNet TOML)
 * runs on the radix-8 kernels, any other even n_fft in [16, 4096] / hop in [1, n_fft] (e.g. 512 / 128
 * and 960 / 480 of improved_fullsubnet/model.py:550-557) on a direct fp64 DFT.  Either way the
 * result is the correctly rounded transform of the fp32 windowed frame. */
int fsn_stft(const float* y, int B, int L, int n_fft, int hop, int win_length, const float* window,
             float* real, float* imag, float* mag, void* stream);

/* feature.py:53-91  istft((real, imag), n_fft, hop, win, length, input_type="real_imag").
 * real/imag [B, F, T] -> y [B, length].  workspace >= fsn_istft_workspace_bytes(B, T, n_fft).
 * Contract: the overlap-added squared window must be non-zero at every sample written (p = n_fft/2 + j < n_fft +
 * hop (T - 1)); the entry divides by it unchecked, like ATen's kernel after torch.istft's own check.  With a window whose
 * first tap is zero (the periodic Hann) hop == n_fft breaks it - sample p = n_fft t is covered by tap 0 of frame t alone
 * and comes out as 0/0 = NaN - and fullsubnet_amd's istft raises there as torch.istft does; every hop < n_fft is fine.
 * fsn_stft at hop == n_fft is supported.  Samples at and past n_fft/2 + hop (T - 1) are written as zeros. */
size_t fsn_istft_workspace_bytes(int B, int T, int n_fft);
int fsn_istft(const float* real, const float* imag, int B, int T, int n_fft, int hop, int win_length,
              const float* window, int length, float* y, void* workspace, size_t workspace_bytes,
              void* stream);

/* fsn_stft on a RAGGED batch: row b of y [B][L_max] holds lengths[b] samples (lengths: device memory, [B]; values are
 * clamped to [n_fft/2 + 1, L_max]); the rest of the row is never read.  real/imag/mag [B, F, T_max], T_max = 1 + L_max / hop
 * (any of the three may be NULL): row b is the STFT of y[b][0 .. lengths[b]) alone - reflected at its own end - in its
 * first T_b = 1 + lengths[b] / hop frames, zeros after them.  n_fft = win_length = 512 / hop = 256 only; any other shape
 * is an error (fsn_last_error). */
int fsn_stft_ragged(const float* y, const int* lengths, int B, int L_max, int n_fft, int hop, int win_length,
                    const float* window, float* real, float* imag, float* mag, void* stream);

/* fsn_stft_ragged at every shape fsn_stft takes (improved_fullsubnet/model.py:550-557 runs 512 / 128 and 960 / 480; feature.py:9-50):
 * same arguments and result - row b is the STFT of y[b][0 .. lengths[b]) alone, reflected at its own end, in its first
 * T_b = 1 + lengths[b] / hop frames; frames past T_b are exact zeros and cost a store, not a transform; samples past
 * lengths[b] are never read (values are clamped to [n_fft/2 + 1, L_max]).  512 / 256 runs on the radix-8 kernels' lengths path
 * (fsn_stft_ragged), any other shape on the ragged forms of the direct-DFT kernels - two-level where n_fft splits, the plain
 * direct form where it is twice a prime - with fsn_stft's own arithmetic: a row equals fsn_stft of that row alone bit for bit. */
int fsn_stft_ragged_generic(const float* y, const int* lengths, int B, int L_max, int n_fft, int hop, int win_length,
                            const float* window, float* real, float* imag, float* mag, void* stream);

/* fsn_istft on a RAGGED batch (feature.py:53-91; improved_fullsubnet/model.py:582-589): real/imag [B, F, T] -> y [B, length],
 * lengths (device, [B]).  Row b is the iSTFT of its own first T_b = 1 + lengths[b] / hop frames at its own length - the same
 * envelope and trim arithmetic as fsn_istft - and zeros from lengths[b] on; frames t >= T_b of real / imag are never read.
 * length is the longest row and T = 1 + length / hop.  Equal lengths give fsn_istft's bits.  Every shape fsn_istft takes;
 * workspace >= fsn_istft_ragged_workspace_bytes(B, T, n_fft) (0: unsupported). */
size_t fsn_istft_ragged_workspace_bytes(int B, int T, int n_fft);
int fsn_istft_ragged(const float* real, const float* imag, const int* lengths, int B, int T, int n_fft, int hop, int win_length,
                     const float* window, int length, float* y, void* workspace, size_t workspace_bytes, void* stream);

/* inferencer.py:134-141 as one call on a model's COMPRESSED cIRM: decompress_cIRM (K = 10, limit = 9.9), the complex
 * mask on the noisy spectrum and the iSTFT, with the fp32 products of the reference's tensor algebra.
 * crm [B, 2, F, T] as a model's forward returns it (read in place); real/imag [B, F, T] as fsn_stft writes them;
 * y [B, length].  lengths (device, [B], may be NULL = a rectangular batch): row b is the iSTFT of its own
 * T_b = 1 + lengths[b] / hop frames at its own length (as fsn_enhance_ragged), zeros from lengths[b] on; frames t >= T_b
 * of crm / real / imag are never read; then length must be the longest row (T = 1 + length / hop).
 * n_fft = win_length = 512 / hop = 256 only.  workspace >= fsn_mask_istft_workspace_bytes(B, T, n_fft) (0: unsupported). */
size_t fsn_mask_istft_workspace_bytes(int B, int T, int n_fft);
int fsn_mask_istft(const float* crm, const float* real, const float* imag, const int* lengths, int B, int F, int T, int n_fft,
                   int hop, int win_length, const float* window, int length, float* y, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---- cIRM mask algebra : audio_zen/acoustics/mask.py ----------------------------------- */

/* The three entries below clamp with comparisons, not with mask.py's products of the value and a 0 / 1 condition: NaN stays
 * NaN, and an infinite input takes the clamp's value where the tensor expression gives inf * 0 = NaN (decompress: +-inf as
 * +-9.9f; compress: -inf as -100, +inf gives exactly 10).  Beyond the clamps the result is bit for bit the one at the clamp.
 * mask.py:47-64  decompress_cIRM(mask, K=10, limit=9.9), elementwise over n floats. */
int fsn_decompress_cirm(const float* mask, float* out, size_t n, void* stream);
/* mask.py:32-44  compress_cIRM(mask, K=10, C=0.1). */
int fsn_compress_cirm(const float* mask, float* out, size_t n, void* stream);
/* mask.py:7-29  build_complex_ideal_ratio_mask: four [n] planes -> out [n, 2] (compressed). */
int fsn_build_cirm(const float* noisy_real, const float* noisy_imag, const float* clean_real,
                   const float* clean_imag, float* out, size_t n, void* stream);

/* ---- feature norms : audio_zen/model/base_model.py --------------------------------------- */

/* norm_wrapper (base_model.py:356-372): any of the five norms on x [B, C, F, T] -> y (same shape; y may alias x), as
 * the composed models call them between their SequenceModel blocks.  sample_length: forgetting_norm's argument
 * (192 in the reference's signature; ignored by the others).  eps <= 0: the reference's constant for that norm
 * (1e-5 / fp32 epsilon / 1e-5 / fp32 epsilon / 1e-10); improved_fullsubnet/model.py:124-216 uses fp32 epsilon in its
 * offline norms and passes it.  Statistics are summed exactly (fp64) and then follow the reference's fp32 tensor
 * arithmetic operation by operation. */
#define FSN_NORM_MAX_FRAMES 6144 /* T of one fsn_norm call (a row's per-frame statistics sit in LDS) */
size_t fsn_norm_workspace_bytes(int norm_type, int B, int C, int F, int T);
int fsn_norm(const float* x, float* y, int norm_type, int B, int C, int F, int T, int sample_length, float eps,
             void* workspace, size_t workspace_bytes, void* stream);

/* ---- FullSubNet model : recipes/dns_interspeech_2020/fullsubnet/model.py --------------- */

typedef struct fsn_fullsubnet_cfg {
    int num_freqs;        /* model.py:12  (257)                                   */
    int look_ahead;       /* model.py:13  (2)                                     */
    int sb_num_neighbors; /* model.py:16  (15); fb_num_neighbors must be 0        */
    int fb_hidden;        /* model.py:19  (512), multiple of 64                   */
    int sb_hidden;        /* model.py:20  384 (the persistent kernel's size)      */
    int norm_type;        /* model.py:21  FSN_NORM_*                              */
    int arith;            /* FSN_ARITH_* (0 = fp32 MFMA)                          */
} fsn_fullsubnet_cfg;

/* The 20 tensors of Model.state_dict() in the reference's layout (nn.LSTM: weight_ih [4H, I],
 * weight_hh [4H, H], gate rows i,f,g,o; nn.Linear: weight [O, I]).  SURVEY §8a rows A5 / A9. */
typedef struct fsn_fullsubnet_params {
    const float *fb_w_ih_l0, *fb_w_hh_l0, *fb_b_ih_l0, *fb_b_hh_l0;
    const float *fb_w_ih_l1, *fb_w_hh_l1, *fb_b_ih_l1, *fb_b_hh_l1;
    const float *fb_fc_w, *fb_fc_b;
    const float *sb_w_ih_l0, *sb_w_hh_l0, *sb_b_ih_l0, *sb_b_hh_l0;
    const float *sb_w_ih_l1, *sb_w_hh_l1, *sb_b_ih_l1, *sb_b_hh_l1;
    const float *sb_fc_w, *sb_fc_b;
} fsn_fullsubnet_params;

/* Re-tile the weights into MFMA B-fragment order (done once per checkpoint load, the analogue of
 * nn.LSTM.flatten_parameters(), sequence_model.py:114). */
size_t fsn_fullsubnet_packed_bytes(const fsn_fullsubnet_cfg* cfg);
int fsn_fullsubnet_pack(const fsn_fullsubnet_cfg* cfg, const fsn_fullsubnet_params* params,
                        void* packed, size_t packed_bytes, void* stream);

/* model.py:72-136  Model.forward(noisy_mag [B,1,F,T]) -> compressed cIRM [B,2,F,T]
 * (inference semantics: every sample keeps all F bins, i.e. num_groups_in_drop_band = 1, see
 * SURVEY quirk Q1). */
size_t fsn_fullsubnet_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int T);
int fsn_fullsubnet_forward(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* noisy_mag,
                           int B, int T, float* crm_out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* model.py:85-95 alone: look-ahead pad, norm, full-band model.  fb_output [B, F, T + look_ahead] is the tensor
 * `fb_output` of model.py:95 (stage-level parity checks; the input a batch-sharded full-band stage would
 * all-gather).  workspace >= fsn_fullsubnet_workspace_bytes(cfg, B, T). */
int fsn_fullsubnet_fullband(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* noisy_mag, int B,
                            int T, float* fb_output, void* workspace, size_t workspace_bytes, void* stream);

/* The same model on a contiguous slice [row_begin, row_end) of the B*F flattened (b, f) rows that
 * model.py:121-128 hands to the sub-band LSTM as independent sequences - the multi-GPU partition of the path
 * (one rank per slice, then one all-gather of the slices).  noisy_mag is the WHOLE batch [B,1,F,T]; only the
 * utterances the slice touches are read: their full-band model (model.py:95) and norm statistics (model.py:92,111)
 * are computed whole, the sub-band model only on the slice.  crm_rows [row_end - row_begin][2][T] receives
 * the compressed cIRM of row n = b*F + f at crm_rows[n - row_begin] (= crm[b, :, f, :] of the full result).
 * A slice aligned to utterances does exactly the work of fsn_fullsubnet_forward on those utterances. */
size_t fsn_fullsubnet_rows_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int T, long row_begin,
                                           long row_end);
int fsn_fullsubnet_forward_rows(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* noisy_mag,
                                int B, int T, long row_begin, long row_end, float* crm_rows,
                                void* workspace, size_t workspace_bytes, void* stream);

/* recipes/dns_interspeech_2020/inferencer.py:130-145  Inferencer.full_band_crm_mask:
 * noisy [B, L] -> enhanced [B, L] (stft -> model -> decompress -> complex mask -> istft), all
 * intermediates kept in the frame-major device layout.  crm_out (optional, may be NULL) receives
 * the compressed mask [B, 2, F, T] for parity checks. */
size_t fsn_enhance_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int L, int n_fft, int hop);
int fsn_enhance(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* window,
                const float* noisy, int B, int L, int n_fft, int hop, float* enhanced, float* crm_out,
                void* workspace, size_t workspace_bytes, void* stream);

/* fsn_enhance on a RAGGED batch: row b of noisy [B][L_max] holds an utterance of lengths[b] samples (lengths: device
 * memory, [B]; values are clamped to [n_fft/2 + 1, L_max]).  Row b of the result is, within fp32 rounding, fsn_enhance
 * of noisy[b][0 .. lengths[b]) alone: the STFT reflects at the row's own end, the offline norm averages over the row's
 * own T_b + look_ahead frames (T_b = 1 + lengths[b] / hop) and the iSTFT uses only its T_b frames.  Beyond each row's
 * end:
 *   - noisy[b][lengths[b] ..] is never read (it may hold anything);
 *   - enhanced[b][lengths[b] ..] is written as zeros;
 *   - crm_out (optional) [B][2][F][T_max], T_max = 1 + L_max / hop: frames t >= T_b of row b are zeros.
 * The models run every row to T_max (the padded steps are the price of one call).  Same arguments, checks, 512 / 256
 * transform and workspace (fsn_enhance_workspace_bytes(cfg, B, L_max, n_fft, hop)) as fsn_enhance; with every length
 * equal to L_max the result is bit-identical to fsn_enhance's. */
int fsn_enhance_ragged(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* window,
                       const float* noisy, const int* lengths, int B, int L_max, int n_fft, int hop,
                       float* enhanced, float* crm_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming: the model on k more frames with carried state --------------------------------- */

/* Frame-by-frame / chunked form of fsn_fullsubnet_forward for real-time use (not in the reference, which only
 * has the whole-utterance loop of inferencer.py:130-145): `state` carries (h, c) of the four LSTM layers and the
 * running sums of the two cumulative Laplace norms (base_model.py:221-251; norm_type must be
 * FSN_NORM_CUMULATIVE_LAPLACE) from call to call - zero-fill it for a new stream.  mag [B, 1, F, k] are the
 * next k input frames of the model (the caller appends the look_ahead zero frames of model.py:85 at the end of
 * the stream), steps_done the number of frames passed in before this call, crm_out [B, 2, F, k] the model
 * output of exactly these steps (step s is the compressed mask of frame s - look_ahead).  Feeding a stream in
 * any chunking gives the offline result. */
size_t fsn_fullsubnet_stream_state_bytes(const fsn_fullsubnet_cfg* cfg, int B);
size_t fsn_fullsubnet_stream_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int k);
int fsn_fullsubnet_stream_step(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                               int steps_done, const float* mag, int B, int k, float* crm_out, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- recordings of any length: the model in segments, state carried, both norms ------------- */

/* fsn_fullsubnet_forward stops at 100 000 frames and its workspace grows with the recording at hidden-state width.  These
 * entries run the same model on k (1 .. 4096) frames at a time: only planes of F floats per frame (magnitude, full-band
 * output, mask) live for the whole recording, in the caller's memory; everything of hidden-size width is inside `workspace`
 * (fsn_fullsubnet_segment_workspace_bytes(cfg, B, k), shared by the passes) and dies with the segment.  fp32 arithmetic only.
 *
 * `state` (fsn_fullsubnet_segment_state_bytes(cfg, B), caller-owned): (h, c) of the four LSTM layers, the running sums of
 * the cumulative norm, and the fp64 accumulators of the offline norm - per-bin magnitude sums [B][FP] and the sum of the
 * full-band output [B].  All zeros is a fresh recording.  Both size queries answer without a device and return 0
 * (fsn_last_error) for B outside 1 .. 4096, k outside 1 .. 4096 or a bad cfg; both norm types are accepted.
 *
 * offline_laplace_norm (base_model.py:204-218) divides by ONE mean per utterance, so a recording takes three passes over
 * its segments, each pass in frame order over the T_max + look_ahead model steps (the caller appends the look_ahead zero
 * frames of model.py:85), each step exactly once:
 *   1. fsn_fullsubnet_segment_stats on every segment: adds the segment's per-bin sums of mag [B, 1, F, k] to the state
 *      (fp64, fixed order inside a segment).
 *   2. fsn_fullsubnet_segment_fullband on every segment: the full-band divisor from the finished sums, both full-band
 *      layers and the output layer on k more frames from the carried (h, c) -> fb_out [B, F, k] (model.py:95); the sum of
 *      fb_out over the frames frames_done + t < total_frames[b] of each row is added to the state.
 *   3. fsn_fullsubnet_segment_subband on every segment: the sub-band divisor (model.py:110-111, the multiplicity-weighted
 *      per-bin sums plus the full-band sum), both sub-band layers and the output layer from the carried (h, c) ->
 *      crm_out [B, 2, F, k]; step s is the compressed mask of frame s - look_ahead, as in fsn_fullsubnet_stream_step.
 * frames_done: model steps passed to THIS pass before the call.  total_frames (device memory, [B]): row b's own
 * T_b + look_ahead.  In a ragged batch every row runs to the longest row's end; a row's mag must be zero from its frame T_b
 * on (fsn_stft_ragged writes it so), and only the divisors and the fb_out sum depend on total_frames.  The divisors are
 * exactly-summed fp64 values, then the reference's fp32 operations (float(sum / count) + 1e-5f), as in the one-call path;
 * the results agree with fsn_fullsubnet_forward within fp32 rounding, not bit for bit (different recurrent kernels), and
 * two segmentations of one recording agree within fp32 rounding of the recurrences (the sums differ in fp64 only).
 * fsn_fullsubnet_segment_divisors writes the two divisors the passes use to den_fb / den_sb (device memory, [B] each); call
 * it after pass 2 for den_sb.
 *
 * cumulative_laplace_norm: the norm is causal, passes 2 and 3 continue its running sums exactly as
 * fsn_fullsubnet_stream_step does (the state begins with that entry's layout), pass 1 does nothing, total_frames may be
 * NULL and fsn_fullsubnet_segment_divisors is refused.  One driver serves both norms. */
size_t fsn_fullsubnet_segment_state_bytes(const fsn_fullsubnet_cfg* cfg, int B);
size_t fsn_fullsubnet_segment_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int k);
int fsn_fullsubnet_segment_stats(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, const float* mag, int B,
                                 int k, void* stream);
int fsn_fullsubnet_segment_fullband(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                    int frames_done, const int* total_frames, const float* mag, int B, int k,
                                    float* fb_out, void* workspace, size_t workspace_bytes, void* stream);
int fsn_fullsubnet_segment_subband(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                   int frames_done, const int* total_frames, const float* mag, const float* fb_out, int B,
                                   int k, float* crm_out, void* workspace, size_t workspace_bytes, void* stream);
int fsn_fullsubnet_segment_divisors(const fsn_fullsubnet_cfg* cfg, const void* state, size_t state_bytes,
                                    const int* total_frames, int B, float* den_fb, float* den_sb, void* stream);

/* ---- streaming pool: sessions that open, advance and close on their own --------------------- */

/* fsn_fullsubnet_stream_step for streams that are NOT in lockstep.  `state` is a pool of `capacity` slots (1 .. 4096),
 * fsn_fullsubnet_stream_pool_state_bytes(cfg, capacity) bytes = capacity equal records, slot s at byte
 * s * (state_bytes / capacity).  A record holds (h, c) of the four LSTM layers, the two running fp64 norm sums, the slot's
 * own step count (on the device: the kernels read and advance it) and the transform state of the two entries below.  All
 * zeros is a fresh pool; fsn_fullsubnet_stream_pool_reset returns the n listed slots to that state (stream-ordered).
 *
 * fsn_fullsubnet_stream_pool_step advances the n listed slots (`slots`: device memory, n DISTINCT ids) by k model steps,
 * each from its own step count: row i of mag [n, 1, F, k] and crm_out [n, 2, F, k] belongs to slots[i], and is what
 * fsn_fullsubnet_stream_step gives a batch of one with the same history.  Slots that are not listed are not written.  A
 * row whose id is outside [0, capacity) is skipped (its crm_out row is finite, no state is touched); listing an id twice
 * is the caller's error.  Both size queries return 0 (fsn_last_error) for a non-causal norm or a size out of range. */
size_t fsn_fullsubnet_stream_pool_state_bytes(const fsn_fullsubnet_cfg* cfg, int capacity);
size_t fsn_fullsubnet_stream_pool_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int n, int k);
int fsn_fullsubnet_stream_pool_reset(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                     const int* slots, int n, void* stream);
int fsn_fullsubnet_stream_pool_step(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                    int capacity, const int* slots, int n, const float* mag, int k, float* crm_out,
                                    void* workspace, size_t workspace_bytes, void* stream);

/* The transform around that step, one frame at a time for the listed slots of the same pool (n_fft = 512, hop = 256 only;
 * cfg->num_freqs = 257).  All int arrays are device memory, [n].
 *
 * fsn_stream_pool_analysis: frame = the slot's last hop ++ hops[i] (hops [n][hop]) -> window -> real FFT.  The spectrum
 * goes to the slot's ring of look_ahead + 1 frames at frame_no[i] (the session's frame index, >= 0), its magnitude to
 * mag [n, 1, F, 1]; hops[i] becomes the slot's last hop.  The caller makes the two edges of torch.stft(center=True) by what
 * it passes: for frame 0 (frame_no[i] == 0) the left half is the reflection y[hop], y[hop - 1] .. y[1], read backwards from
 * prime[i] = y[1 .. hop] (prime [n][hop]; rows of sessions not at frame 0 are not read).  CONTRACT: prime may be NULL only
 * when no listed session is at frame 0.  frame_no lives on the device, so the entry cannot check this: a frame 0 with
 * prime == NULL takes the slot's carried hop like any other frame - zeros on a fresh slot, i.e. a zero-padded left edge
 * instead of torch.stft's reflection - and no error is raised.  The session's last frame gets a hop that continues
 * past the end L by reflection (sample j >= L is y[2 (L - 1) - j]).
 *
 * fsn_stream_pool_synthesis: column j of crm [n, 2, F, k] is the compressed mask of output frame m = first_frame[i] + j of
 * slots[i] (m < 0: a model step of the first look_ahead frames, no output).  Frame m's spectrum is taken from the ring
 * (so m must be one of the last look_ahead + 1 analysed frames), decompress_cIRM and the complex mask applied, then
 * irfft, window and overlap-add with the slot's carried half frame as torch.istft does: frame m >= 1 gives the hop samples
 * [(m - 1) hop, m hop) at out[i][j hop ..]; frame 0 gives none.  tail_samples[i] >= 0 marks the session's last frame:
 * the samples [(T - 1) hop, L), tail_samples[i] = L - (T - 1) hop of them, follow at out[i][k hop ..] (pass -1
 * otherwise).  out [n][(k + 1) hop] is written completely (zeros where there is no sample);
 * workspace >= n k n_fft floats. */
int fsn_stream_pool_analysis(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, int capacity,
                             const int* slots, int n, const float* hops, const float* prime, const int* frame_no,
                             int n_fft, int hop, const float* window, float* mag, void* stream);
int fsn_stream_pool_synthesis(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, int capacity,
                              const int* slots, int n, const float* crm, int k, const int* first_frame,
                              const int* tail_samples, int n_fft, int hop, const float* window, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- training step: one nn.LSTM layer with back-propagation through time ----------------- */

/* audio_zen/model/module/sequence_model.py:52-58 (nn.LSTM, one layer, batch_first, h0 = c0 = 0) as
 * used under autograd by fullsubnet/trainer.py:56-63.  Time-major rows: x [T][N][ldx] (columns
 * I..ldx-1 zero, ldx >= round_up(I,16)), hseq [T][N][H]; w_ih [4H][I], w_hh [4H][H], b_* [4H] in the
 * reference's layout.  N % 16 == 0, H % 64 == 0 (a smaller hidden size is run zero-padded: units
 * with all-zero weights and biases stay at h = c = 0, exactly).  `save` keeps the activated gates and
 * the cell sequence for the backward pass; save == NULL is inference mode (SequenceModel.forward under
 * no_grad, sequence_model.py:106-125): nothing but hseq is kept and, for H = 384, the rows run on the
 * persistent recurrent kernels of the sub-band model - with a narrow input (I <= 32) or as the layer above an
 * equally wide one (I = H = ldx) on the forms that build their input projection themselves, in whole rounds of
 * 2 - 4 row tiles per workgroup (several rounds beyond four tiles per CU); row tiles left over advance step by step
 * beside the launch from their own small projection (round 6). */
size_t fsn_lstm_layer_save_bytes(int T, int N, int H);
size_t fsn_lstm_layer_fwd_workspace_bytes(int T, int N, int I, int H);
int fsn_lstm_layer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                           const float* b_hh, int T, int N, int I, int H, float* hseq, void* save,
                           size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* Two stacked layers of equal width H (nn.LSTM(num_layers = 2), sequence_model.py:52-58) forward with saved
 * activations: the result of two fsn_lstm_layer_forward calls (hseq0 / save0 and hseq1 / save1 in that entry's
 * layouts, each save buffer >= fsn_lstm_layer_save_bytes(T, N, H)), ready for two fsn_lstm_layer_backward calls.
 * The full-band shape (H = 512, N <= 64) runs as ONE persistent launch for both layers and all steps
 * (fb_chain_kernel) instead of 2 T launches; other shapes run layer by layer.
 * arith: FSN_ARITH_F32, or FSN_ARITH_F16 / FSN_ARITH_BF16 = the autocast arithmetic the reference trains under
 * (trainer.py:56): on the sub-band shape (the group kernels, 99 % of the step's products) both operands of every
 * product are rounded to 16 bits at the matrix core's input, accumulation and everything stored stay fp32; shapes
 * that run on other kernels compute in fp32 (wider than asked for).  Same rule for fsn_lstm2_backward, which then
 * expects dh1 scaled by the caller's loss scale (GradScaler) like any autocast backward. */
size_t fsn_lstm2_train_workspace_bytes(int T, int N, int I, int H, int arith);
/* 1 when BOTH directions of this shape run as persistent launches (forward: the group kernel - H = 384, 17 - 32 input
 * columns, 96+ row tiles in whole 64-row clusters up to 8 left-over tiles - or the chain; backward likewise): the shapes on
 * which the 16-bit arithmetic has kernels of its own.  Callers with more rows than one launch holds split them into such
 * pieces (the rows of a stack are independent sequences: sequence_model.py:52-58; fullsubnet_amd.train.lstm2_train_chunks). */
int fsn_lstm2_train_is_persistent(int T, int N, int I, int H);
int fsn_lstm2_forward_train(const float* x, long ldx, const float* w_ih0, const float* w_hh0, const float* b_ih0,
                            const float* b_hh0, const float* w_ih1, const float* w_hh1, const float* b_ih1,
                            const float* b_hh1, int T, int N, int I, int H, float* hseq0, float* hseq1, void* save0,
                            void* save1, size_t save_bytes, void* workspace, size_t workspace_bytes, int arith,
                            void* stream);
/* Two stacked LSTM layers in inference mode, advanced as a wavefront (layer 1 at step t next to layer 0 at
 * step t + 1): T + 1 dependent launches instead of 2 T.  Either nn.LSTM(num_layers = 2) of one SequenceModel
 * (H1 == H0, sequence_model.py:52-58) or two consecutive single-layer blocks of different widths (the
 * encoder / decoder pairs of fast_fullsubnet/model.py:35-96; layer 1 takes the H0 outputs of layer 0).  For
 * blocks with few rows (the latency-bound regime); hseq1 [T][N][H1] is the hidden sequence of the second layer. */
size_t fsn_lstm2_fwd_workspace_bytes(int T, int N, int I, int H0, int H1);
/* 1 when fsn_lstm2_forward runs this call (T steps, N rows of ldx floats) as ONE persistent launch (equal widths of
 * 384 / 512 with up to 64 rows and 4095 steps: the chain kernel; 384 twice, up to 32 input columns in rows of exactly
 * 16 or 32 floats, 1536 - 2559 or 3584 - 4096 rows in whole 64-row clusters, hidden sequence below 2 GB: the group
 * kernel) - then it is also the better choice above the few-row regime it was made for.  Anything else runs on the
 * generic path of fsn_lstm2_forward (never an error). */
int fsn_lstm2_forward_is_persistent(int T, int N, int I, long ldx, int H0, int H1);
int fsn_lstm2_forward(const float* x, long ldx, const float* w_ih0, const float* w_hh0, const float* b_ih0,
                      const float* b_hh0, const float* w_ih1, const float* w_hh1, const float* b_ih1,
                      const float* b_hh1, int T, int N, int I, int H0, int H1, float* hseq1, void* workspace,
                      size_t workspace_bytes, void* stream);

/* improved_fullsubnet/model.py:402-440 (SubbandModel.forward up to the sequence model) for one band section
 * [lower, upper) of the F-bin inputs noisy / fb_out [B][F][T]: unit u sees the noisy bins lower + u c - n .. (c =
 * sb_center, n = sb_neighbor; model.py:315-400 `_freq_unfold`, reflected at both ends of the spectrum) and the same
 * window of the full-band output (fb_center, fb_neighbor), concatenated and divided by (the mean of the WHOLE section's
 * unfolded input of that utterance + eps): offline_laplace_norm, model.py:124-150 (eps = torch.finfo(float32).eps
 * there).  The result is written for units [unit_lo, unit_hi) in the layout the LSTM entries take: out [T][Np][ldo],
 * row b (unit_hi - unit_lo) + (u - unit_lo), columns beyond the window and rows beyond B (unit_hi - unit_lo) zero
 * (Np <= 65535 rows, ldo <= 240 columns).
 * The unfolded tensor is never formed (three launches instead of nine per section). */
size_t fsn_improved_section_input_workspace_bytes(int B, int F);
int fsn_improved_section_input(const float* noisy, const float* fb_out, int B, int F, int T, int lower, int upper,
                               int sb_center, int sb_neighbor, int fb_center, int fb_neighbor, int unit_lo, int unit_hi,
                               float eps, float* out, int Np, int ldo, void* workspace, size_t workspace_bytes,
                               void* stream);

/* fsn_improved_section_input on a RAGGED batch: frames (device, [B]) holds utterance b's frame count T_b in [1, T].  The
 * section's statistic (model.py:124-150 on the unfolded input of model.py:402-440) comes from the frames t < T_b only - past a
 * row's end the full-band output is an LSTM's response to zero input, not zero - with the count units x columns x T_b; the
 * gathered output is zero for t >= T_b, and neither input is read there.  Same tile limits and workspace as the rectangular
 * entry; frames[b] = T for every b gives its bits. */
int fsn_improved_section_input_ragged(const float* noisy, const float* fb_out, const int* frames, int B, int F, int T, int lower,
                                      int upper, int sb_center, int sb_neighbor, int fb_center, int fb_neighbor, int unit_lo,
                                      int unit_hi, float eps, float* out, int Np, int ldo, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* The tensor glue AROUND the models of the composed families (round 5; section_kernels.hip), all bit-identical to the tensor
 * algebra it replaces:
 * fsn_improved_front      improved_fullsubnet/model.py:565-566: mag [B][F][T] -> out [B][F - 1][T] = mag ** fdrc without the
 *                         last bin, contiguous; sqrt_mode 1: fdrc = 0.5 (sqrtf, what torch.pow computes for that exponent),
 *                         0: fdrc = 1.
 * fsn_bft_to_rows         x [B][F][T] -> h [T][Np][Ip], zero beyond (B, F): the layout every LSTM / Linear entry takes
 *                         (audio_zen/model/module/sequence_model.py:106-125 permutes to [B, T, F] for nn.LSTM).
 * fsn_rows_to_bft         o [T][Np][ld] -> y [B][O][T]: the way back (sequence_model.py:123).
 * fsn_improved_mask_apply model.py:438-449 (the sections' outputs re-ordered and concatenated along the bins), :575 F.pad of
 *                         the last bin and :576-577 (mask x noisy real / imaginary part, no complex product) in one pass:
 *                         section i's output o [T][Np][ld] (as fsn_linear_forward writes it: row b units + u, column
 *                         comp center + cc) -> er / ei [B][F][T] at bin lower + u center + cc; bins no section covers: 0. */
typedef struct fsn_mask_section {
    const void* o; /* [T][Np][ld] */
    int Np, ld, lower, units, center;
} fsn_mask_section;
int fsn_improved_front(const float* mag, int B, int F, int T, int sqrt_mode, float* out, void* stream);
int fsn_bft_to_rows(const float* x, int B, int F, int T, float* h, int Np, int Ip, void* stream);
int fsn_rows_to_bft(const float* o, int T, int Np, int ld, int B, int O, float* y, void* stream);
int fsn_improved_mask_apply(int n, const fsn_mask_section* sections, const float* real, const float* imag, int B, int F, int T,
                            float* er, float* ei, void* stream);
/* fsn_improved_front and the offline Laplace norm of the full-band input (improved_fullsubnet/model.py:565-567, norm :124-150)
 * on a RAGGED batch, as ONE fused entry: out [B][F - 1][T] = mag ** fdrc without the last bin for t < frames[b] and zero from
 * there on (mag is not read past a row's end); normed = out / (mean over the (F - 1) x frames[b] entries of the row + eps), zero
 * past the end as well.  frames: device, [B], values in [1, T].  The sums are fp64, rounded once, then the reference's fp32
 * division, as fsn_norm does: frames[b] = T for every b gives the bits of fsn_improved_front followed by fsn_norm.
 * workspace >= fsn_improved_front_norm_ragged_workspace_bytes(B, F, T). */
size_t fsn_improved_front_norm_ragged_workspace_bytes(int B, int F, int T);
int fsn_improved_front_norm_ragged(const float* mag, const int* frames, int B, int F, int T, int sqrt_mode, float eps, float* out,
                                   float* normed, void* workspace, size_t workspace_bytes, void* stream);

/* Two stacked GRU layers of equal width (nn.GRU(num_layers = 2) of a SequenceModel, sequence_model.py:59-66; weights in nn.GRU's
 * layout: w_ih [3H][I], w_hh [3H][H], biases [3H], gate rows r, z, n) with few rows - the full-band model of a GRU FullSubNet -
 * as ONE persistent launch (the chain kernel with the GRU written as a four-gate cell) instead of 2 T per-step launches.
 * fsn_gru2_forward_supported: 1 for H = 384 / 512, N <= 64 rows (a multiple of 16), T <= 4095 on a device that holds the
 * chain's grid; anything else: fsn_gru_layer_forward layer by layer.  x [T][N][ldx] time-major, hseq1 [T][N][H]. */
int fsn_gru2_forward_supported(int T, int N, int H);
size_t fsn_gru2_fwd_workspace_bytes(int T, int N, int I, int H);
int fsn_gru2_forward(const float* x, long ldx, const float* w_ih0, const float* w_hh0, const float* b_ih0, const float* b_hh0,
                     const float* w_ih1, const float* w_hh1, const float* b_ih1, const float* b_hh1, int T, int N, int I, int H,
                     float* hseq1, void* workspace, size_t workspace_bytes, void* stream);

/* Up to eight INDEPENDENT two-layer stacks over the same T frames: the band sections of
 * improved_fullsubnet/model.py:402-449, whose SequenceModels have B x {20, 25, 6, 4} rows and input widths 62 .. 180 at
 * 48 kHz.  Per stack the arguments of fsn_lstm2_forward.  When every stack has H0 = H1 = 384, T >= 4 and together they fill
 * most of the chip (fsn_lstm2_multi_is_persistent: 3/4 .. 1 x CUs / 8 clusters of 64 rows) they run as ONE persistent
 * launch of the group kernel with one weight set per stack; otherwise one stack after the other as fsn_lstm2_forward
 * would (callers with small stacks do better to put them on one stream each).  Results equal fsn_lstm2_forward's per
 * stack within fp32 rounding (the kernels differ in their order of accumulation). */
typedef struct fsn_lstm2_stack {
    const float* x; /* [T][N][ldx], columns I .. ldx-1 zero */
    long ldx;
    const float *w_ih0, *w_hh0, *b_ih0, *b_hh0, *w_ih1, *w_hh1, *b_ih1, *b_hh1;
    int N, I, H0, H1;
    float* hseq1; /* [T][N][H1] out */
} fsn_lstm2_stack;
int fsn_lstm2_multi_is_persistent(int n, const fsn_lstm2_stack* stacks, int T);
size_t fsn_lstm2_multi_workspace_bytes(int n, const fsn_lstm2_stack* stacks, int T);
int fsn_lstm2_forward_multi(int n, const fsn_lstm2_stack* stacks, int T, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Streaming inference (chunked / frame-by-frame processing with carried state - the real-time use the
 * model is designed for; the reference has no such entry point, nn.LSTM's (h_0, c_0) argument is the
 * analogue).  fsn_lstm_layer_pack re-tiles one layer's weights once; fsn_lstm_layer_forward_state then runs
 * T more steps starting from h_state / c_state [N][H], both updated in place, with two launches plus one per
 * step.  workspace >= fsn_lstm_layer_state_workspace_bytes(T, N, H). */
size_t fsn_lstm_layer_packed_bytes(int I, int H);
int fsn_lstm_layer_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int I, int H,
                        void* packed, size_t packed_bytes, void* stream);
size_t fsn_lstm_layer_state_workspace_bytes(int T, int N, int H);
int fsn_lstm_layer_forward_state(const float* x, long ldx, const void* packed, int T, int N, int I, int H,
                                 float* hseq, float* h_state, float* c_state, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* dh [T][N][H] = dLoss/dhseq.  Outputs: dx [T][N][lddx] (may be NULL), dw_ih [4H][I], dw_hh [4H][H],
 * db [4H] (= d b_ih = d b_hh). */
size_t fsn_lstm_layer_bwd_workspace_bytes(int T, int N, int I, int H);
int fsn_lstm_layer_backward(const float* dh, const float* x, long ldx, const float* w_ih, const float* w_hh, int T,
                            int N, int I, int H, const float* hseq, const void* save, float* dx, long lddx,
                            float* dw_ih, float* dw_hh, float* db, void* workspace, size_t workspace_bytes,
                            void* stream);

/* The LAST layer of an inference stack together with the nn.Linear(H, O) that follows it (sequence_model.py:106-125:
 * self.fc_output_layer(self.sequence_model(x)); Fast FullSubNet's bottleneck, fast_fullsubnet/model.py:66-74: 16 384 rows x
 * 384 units -> one value per step).  Where the persistent kernel that forms the projection itself takes the layer
 * (fsn_lstm_layer_fc_supported: H = I = ldx = 384, O = 1 or 2, whole rounds of 2 - 4 row tiles per CU) its fused two-row
 * output layer does the nn.Linear too: the [T][N][H] hidden sequence is neither written nor read back.  out0 / out1:
 * PRE-activation outputs 0 / 1, time-major [T][ldo] (out1 may be NULL when O == 1); the caller applies the block's
 * activation.  Any other shape: FSN_ERR_ARG (fsn_lstm_layer_forward + fsn_linear_forward take it). */
/* Row padding hint for a caller that owns the padding of a stand-alone inference layer's rows: the row count (a multiple of 16,
 * >= N) to allocate so that the persistent kernels take every row with no left-over tiles, where that is the faster plan (e.g. 448
 * row tiles: 224 workgroups x 2 tiles instead of 256 x 1 + 192 tiles step by step); N rounded up to 16 otherwise.  Rows beyond N
 * must be zero-filled inputs (their outputs are not meaningful). */
int fsn_lstm_layer_plan_rows(int N, int H);
int fsn_lstm_layer_fc_supported(int T, int N, int I, long ldx, int H, int O);
size_t fsn_lstm_layer_fc_workspace_bytes(int T, int N, int I, int H);
int fsn_lstm_layer_forward_fc(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                              const float* b_hh, int T, int N, int I, int H, const float* fc_w, const float* fc_b, int O,
                              float* out0, float* out1, long ldo, void* workspace, size_t workspace_bytes, void* stream);

/* Backward of two stacked layers (the counterpart of fsn_lstm2_forward_train): dh1 [T][N][H] = dLoss/dhseq1;
 * outputs as two fsn_lstm_layer_backward calls would give them (dx may be NULL).  The sub-band shape (H = 384, 96+
 * row tiles) runs its back-propagation through time - both layers, all steps, the layer-to-layer dX - as ONE
 * persistent launch (lstm2_group_bptt_kernel) followed by the weight-gradient GEMMs. */
size_t fsn_lstm2_bwd_workspace_bytes(int T, int N, int I, int H, int arith);
int fsn_lstm2_backward(const float* dh1, const float* x, long ldx, const float* w_ih0, const float* w_hh0,
                       const float* w_ih1, const float* w_hh1, int T, int N, int I, int H, const float* hseq0,
                       const float* hseq1, const void* save0, const void* save1, float* dx, long lddx, float* dw_ih0,
                       float* dw_hh0, float* db0, float* dw_ih1, float* dw_hh1, float* db1, void* workspace,
                       size_t workspace_bytes, int arith, void* stream);

/* The same in parts, for callers that have other work waiting on dx (fullsubnet/trainer.py:56-69: the full-band model's
 * backward only needs the sub-band model's input gradient).  `phase` is a sum of 1 = back-propagation through time (the
 * gate gradients stay in the workspace), 4 = dx from them, 2 = the weight- and bias-gradient products from them; 7 =
 * fsn_lstm2_backward; 8 = only what the products need besides the gate gradients (16-bit copies of the hidden sequences:
 * independent of part 1, so it can run on another stream WHILE part 1 runs), 16 (with 2) = a part-8 call has done that.  Parts 2 and 4 take the same arguments and the same workspace as part 1, which nothing else may touch
 * in between; either may be issued on ANOTHER stream, ordered behind part 1 by the caller (an event), so that the products
 * run beside whatever follows dx. */
int fsn_lstm2_backward_phase(const float* dh1, const float* x, long ldx, const float* w_ih0, const float* w_hh0,
                             const float* w_ih1, const float* w_hh1, int T, int N, int I, int H, const float* hseq0,
                             const float* hseq1, const void* save0, const void* save1, float* dx, long lddx, float* dw_ih0,
                             float* dw_hh0, float* db0, float* dw_ih1, float* dw_hh1, float* db1, void* workspace,
                             size_t workspace_bytes, int arith, int phase, void* stream);

/* nn.GRU branch of SequenceModel (sequence_model.py:59-66), one layer, unidirectional, h0 = 0; same
 * conventions as the LSTM layer above with 3H gate rows (r, z, n).  save == NULL: inference.  The two
 * bias gradients differ in the n block (b_hn sits inside r * (W_hn h + b_hn)), hence two outputs.
 * Inference with MANY rows (ABI 117; the sub-band model of a GRU FullSubNet, fullsubnet/model.py:121-128 with
 * sequence_model = "GRU"): H = 384, N >= 18 rows per CU and either I <= 32 (a narrow row-major input) or I = H = ldx (the
 * layer above an equally wide one) run on the LSTM's persistent many-row kernels with the GRU written as a four-gate cell
 * (3/4 of the LSTM's matrix work: the two zero blocks are skipped) - fsn_gru_layer_is_persistent says whether; left-over
 * row tiles advance step by step beside the launch.  Results equal the step form's within fp32 rounding. */
int fsn_gru_layer_is_persistent(int T, int N, int I, long ldx, int H);
size_t fsn_gru_layer_save_bytes(int T, int N, int H);
size_t fsn_gru_layer_fwd_workspace_bytes(int T, int N, int I, int H);
int fsn_gru_layer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                          const float* b_hh, int T, int N, int I, int H, float* hseq, void* save, size_t save_bytes,
                          void* workspace, size_t workspace_bytes, void* stream);
/* Streaming form: T more steps from the carried state h_state [N][H] (zero-filled for a new stream), updated in
 * place - nn.GRU(x, h_0) is the analogue; workspace >= fsn_gru_layer_fwd_workspace_bytes(T, N, I, H).  Chunked calls
 * give the offline result bit for bit (the same step kernels in the same order) wherever the offline call runs step by
 * step (fsn_gru_layer_is_persistent == 0), within fp32 rounding otherwise. */
int fsn_gru_layer_forward_state(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                const float* b_hh, int T, int N, int I, int H, float* hseq, float* h_state,
                                void* workspace, size_t workspace_bytes, void* stream);
size_t fsn_gru_layer_bwd_workspace_bytes(int T, int N, int I, int H);
int fsn_gru_layer_backward(const float* dh, const float* x, long ldx, const float* w_ih, const float* w_hh, int T,
                           int N, int I, int H, const float* hseq, const void* save, float* dx, long lddx,
                           float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace,
                           size_t workspace_bytes, void* stream);

/* nn.Linear (sequence_model.py:82-84) of the training step.  x [R][ldx] with ldx = round_up(I,16) and
 * zero padding, w [O][I], b [O] -> y [R][O] (ReLU fused when relu != 0).  Backward: dy [R][lddy]
 * (lddy = round_up(O,16), zero padded) -> dx [R][lddx] (may be NULL), dw [O][I], db [O]. */
size_t fsn_linear_workspace_bytes(int R, int I, int O);
int fsn_linear_forward(const float* x, long ldx, const float* w, const float* b, int R, int I, int O, int relu,
                       float* y, void* workspace, size_t workspace_bytes, void* stream);
int fsn_linear_backward(const float* dy, long lddy, const float* x, long ldx, const float* w, int R, int I, int O,
                        float* dx, long lddx, float* dw, float* db, void* workspace, size_t workspace_bytes,
                        void* stream);

/* ---- training step: loss, gradient clipping and the optimizer ------------------------------- */

/* audio_zen/loss.py:4 (torch.nn.MSELoss(), reduction "mean") as used at fullsubnet/trainer.py:62:
 * loss[0] = mean((input - target)^2); grad_input (may be NULL) = 2 (input - target) / n, i.e. the
 * gradient for an upstream gradient of 1.  Deterministic two-pass reduction (fp64 partials). */
size_t fsn_mse_loss_workspace_bytes(size_t n);
int fsn_mse_loss(const float* input, const float* target, size_t n, float* loss, float* grad_input,
                 void* workspace, size_t workspace_bytes, void* stream);


/* ---- glue of the TRAINING graph (fullsubnet/model.py:72-136 under autograd, fullsubnet/trainer.py:41-71) ----------------
 * Everything between the transforms, the LSTM / Linear entries above and the loss, as kernels (train_glue_kernels.hip):
 * no tensor-algebra kernel of the host framework is left in a training step.  Dimensions: B utterances, F bins, T frames,
 * look_ahead (model.py:13), nb = sb_num_neighbors (model.py:16), groups = num_groups_in_drop_band (model.py:22; band
 * dropping applies when B > 1 and groups > 1, audio_zen/acoustics/feature.py:309-345).  Row order of the sub-band
 * tensors = drop_band's: group i holds samples i, i + g, ... at bins i, i + g, ... (< F - F % g), groups concatenated
 * along the batch axis: row r = b_out Fs + fs.  Time-major tensors: [Tp = T + look_ahead][rows padded][columns padded].
 *
 * fsn_train_rows            Fs (bins per band-dropped sample) and R = B Fs (sub-band rows).
 * norm = FSN_NORM_OFFLINE_LAPLACE (train.toml:82) or FSN_NORM_CUMULATIVE_LAPLACE (train_cumulativeLaplaceNorm.toml:82).
 * fsn_train_fb_input        mag [B][F][T] -> x_tm [Tp][Bp][Fp] = pad(mag) / (mean_b + 1e-5) (model.py:85-95: look-ahead pad,
 *                           base_model.py:204-218 offline Laplace norm over [1, F, Tp]; cumulative: / (running mean over the
 *                           frames so far + EPSILON, base_model.py:221-251)), zeros beyond (B, F): the input of
 *                           fsn_lstm2_forward_train (ldx = Fp); mag_tm [Tp][Bp][Fp] = the padded magnitude itself, for
 *                           fsn_train_sb_input.  Leaves the per-bin sums in `workspace` (same buffer for the whole step).
 * fsn_train_sb_input        freq_unfold(mag, nb) ++ fb_out, / (mean + 1e-5), rows of drop_band (model.py:98-125;
 *                           base_model.py:14-46) -> sb_in [Tp][Rp][32] (columns 2 nb + 2 .. 31 and rows beyond R zero);
 *                           fb_out_tm [Tp][Bp][ld_fb] = the full-band output layer's result (fsn_linear_forward, ReLU);
 *                           den [fsn_train_den_elems] = the divisors (kept for the backward): [B], one per utterance
 *                           (offline; the mean of the unfolded tensor is taken from per-bin sums and window multiplicities) or
 *                           [Tp][Rp], one per unit and frame (cumulative: base_model.py:230-251 sees the units as samples and
 *                           a unit's 2 nb + 2 rows as its frequencies; Rp <= rows rounded up to 64).  The unfolded tensor is
 *                           never formed.  CALL ORDER: the offline norm reads the per-bin sums over the frames (rowsum
 *                           [B][F], fp64, the first region of `workspace`, written by tr_rowsum_kernel) that
 *                           fsn_train_fb_input of the same dims and the same mag left there - call fsn_train_fb_input
 *                           first, on the same workspace.  That region is what must survive: no entry of this group
 *                           writes it but fsn_train_fb_input (the backward overwrites the per-frame partials and the
 *                           mean gradients, which fsn_train_sb_input forms anew), so the backward of one step may run
 *                           before the next fsn_train_sb_input of the same mag; a call with other dims or another mag
 *                           in between may not.  Rows >= B and columns >= F of fb_out_tm are never read.
 * fsn_train_sb_input_backward  dx [Tp][Rp][32] (d loss / d sb_in, from fsn_lstm2_backward) -> d_fb [Tp Bp][ld_dfb]: the
 *                           gradient of the full-band output layer's PRE-activation (through the ReLU: fb_out > 0), directly
 *                           (column 2 nb + 1 of the kept rows) and through the mean (cumulative: through the running means of
 *                           this and all later frames of the same unit) - the padded dy fsn_linear_backward takes.  Columns
 *                           2 nb + 2 .. 31 of dx are never read (the dX product does not write them).
 * fsn_train_mask_out        y [Tp][Rp][2] (fsn_linear_forward of the sub-band output layer) -> mask [B][2][Fs][T], the
 *                           look-ahead frames dropped (model.py:129-135).   fsn_train_mask_grad: its adjoint, d_mask ->
 *                           dy [Tp][Rp][ld] (zeros in the look-ahead frames and the padding).
 * fsn_train_cirm_target     compressed cIRM of (noisy, clean) spectra [B][F][T] (mask.py:7-44), band-dropped like the
 *                           prediction, in its layout [B][2][Fs][T] (trainer.py:51-53).  Any row count B Fs (more than
 *                           65535 rows stride over the grid).
 * fsn_scale_by_scalar       y = x * (*scale), scale a device scalar (the incoming gradient of the loss). */
typedef struct fsn_train_dims {
    int B, F, T, look_ahead, nb, groups;
    int norm; /* FSN_NORM_OFFLINE_LAPLACE / FSN_NORM_CUMULATIVE_LAPLACE (model.py:21 norm_type) */
} fsn_train_dims;
int fsn_train_rows(const fsn_train_dims* dims, int* Fs, int* R);
size_t fsn_train_glue_workspace_bytes(const fsn_train_dims* dims);
size_t fsn_train_den_elems(const fsn_train_dims* dims, int Rp);
int fsn_train_fb_input(const fsn_train_dims* dims, const float* mag, float* x_tm, float* mag_tm, int Bp, int Fp,
                       void* workspace, size_t workspace_bytes, void* stream);
int fsn_train_sb_input(const fsn_train_dims* dims, const float* mag_tm, const float* fb_out_tm, long ld_fb, int Bp, int Fp,
                       float* sb_in, int Rp, float* den, void* workspace, size_t workspace_bytes, void* stream);
int fsn_train_sb_input_backward(const fsn_train_dims* dims, const float* dx, const float* sb_in, int Rp, const float* den,
                                const float* fb_out_tm, long ld_fb, int Bp, float* d_fb, long ld_dfb, void* workspace,
                                size_t workspace_bytes, void* stream);
int fsn_train_mask_out(const fsn_train_dims* dims, const float* y, int Rp, float* mask, void* stream);
int fsn_train_mask_grad(const fsn_train_dims* dims, const float* d_mask, float* dy, int Rp, int ld, void* stream);
/* Time-major rows src [T][N][W] -> dst [n][T][rows][W] (to_pieces = 1; rows beyond N zero) or back (to_pieces = 0: src the
 * pieces, dst the rows; rows beyond N dropped): a batch with more sub-band rows than one persistent training launch holds
 * - the shipped TOMLs train 32 / 48 utterances per process, train.toml:52 - runs as n equal pieces of whole clusters
 * (fullsubnet/model.py:121-128: the rows are independent sequences).  W even, n rows >= N, T <= 65535. */
int fsn_train_rows_pieces(const float* src, float* dst, int T, long N, int W, int rows, int n, int to_pieces, void* stream);
int fsn_train_cirm_target(const fsn_train_dims* dims, const float* noisy_real, const float* noisy_imag,
                          const float* clean_real, const float* clean_imag, float* target, void* stream);
int fsn_scale_by_scalar(const float* x, const float* scale, float* y, size_t n, void* stream);

/* Fast FullSubNet's tensor glue between its LSTM / Linear blocks (fast_fullsubnet/model.py:108-140 real_time_down /
 * up-sampling, :143-202 forward), every tensor TIME-MAJOR [frames][rows][columns] - the layout the LSTM entries take and
 * fsn_linear_forward writes - so that no transposing copy sits between two blocks (fast_glue_kernels.hip):
 * fsn_fast_spec_rows        mag [B][F][T0] (model.py:151 functional.pad(..., [0, look_ahead]) included) -> rows
 *                           [T0 + look_ahead][Bp][Fp] of the mel product (model.py:157), zero beyond (T0, B, F).
 * fsn_fast_norm_rows        offline_laplace_norm (base_model.py:204-218) of x [T][Bp][C]: out = x / (mean over the
 *                           utterance's T x C values + 1e-5), rows beyond B zero (model.py:160, the encoder's input).
 *                           workspace: B floats rounded up to 256 bytes, which every fsn_fast_glue_workspace_bytes(T >= 2,
 *                           B, ...) covers (the query itself answers 0 for T = 1, a length this entry takes); rows >= B of x
 *                           are not read.
 * fsn_fast_bottleneck_input model.py:163-178: unit windows of mel (mel_neighbors) and of the encoder output (enc_neighbors),
 *                           reflected at the band edges (base_model.py:14-46), concatenated, down-sampled in time (frame 0
 *                           kept, then means over blocks of `shrink` frames, a shorter last block over what it has),
 *                           divided by (the utterance's mean of that tensor + 1e-5): out [Ts][Np][Wp], row b num_mels + m,
 *                           zero padding; Ts = fsn_fast_low_rate_frames(T, shrink).  The unfolded tensor is never formed.
 * fsn_fast_decoder_input    model.py:131-140 + :188-190: out [T][Bp][2 num_mels] = encoder output | bottleneck output held
 *                           for `shrink` frames (frame t takes low-rate frame t / shrink; slow[ts ld_slow_frame + row ld_slow_row];
 *                           relu != 0: `slow` is the bottleneck output layer's PRE-activation, fsn_lstm_layer_forward_fc).
 * fsn_fast_mask_out         model.py:200-202: o [T][Bp][ld >= 2F] -> mask [B][2][F][T - look_ahead] (first frames dropped). */
int fsn_fast_low_rate_frames(int T, int shrink);
size_t fsn_fast_glue_workspace_bytes(int T, int B, int num_mels, int shrink);
int fsn_fast_spec_rows(const float* mag, int B, int F, int T0, int look_ahead, float* rows, int Bp, int Fp, void* stream);
int fsn_fast_norm_rows(const float* x, int T, int B, int Bp, int C, float* out, void* workspace, size_t workspace_bytes,
                       void* stream);
int fsn_fast_bottleneck_input(const float* mel, const float* enc, long ld_enc, int T, int B, int Bp, int num_mels,
                              int mel_neighbors, int enc_neighbors, int shrink, float* out, int Np, int Wp, void* workspace,
                              size_t workspace_bytes, void* stream);
int fsn_fast_decoder_input(const float* enc, long ld_enc, const float* slow, long ld_slow_frame, long ld_slow_row, int relu, int T,
                           int B, int Bp, int num_mels, int shrink, float* out, void* stream);
int fsn_fast_mask_out(const float* o, long ld, int T, int B, int Bp, int F, int look_ahead, float* mask, void* stream);

/* The same four glue steps on a RAGGED batch (Model.forward(mix_mag, frames=...)): frames (device, [B], not NULL) holds
 * utterance b's STFT frame count T_b before the look-ahead (clamped to [1, T0], T0 = T - look_ahead); row b then behaves as
 * a batch of one utterance of T_b frames - its own look_ahead zero frames, its own norms and down-sampling blocks.  The LSTM
 * blocks between them are causal and run every row to T: a row's first T_b + look_ahead steps never see the padded ones.
 * fsn_fast_spec_rows_ragged        mag frames t >= T_b are never read; their rows are written as zeros.
 * fsn_fast_norm_rows_ragged        the mean covers the row's own (T_b + look_ahead) x C values.
 * fsn_fast_bottleneck_input_ragged row b has Ts_b = fsn_fast_low_rate_frames(T_b + look_ahead, shrink) low-rate frames: the
 *                                  last down-sampling block ends at T_b + look_ahead (averaged on its own, short or whole),
 *                                  the mean divides by num_mels W Ts_b, and units of frames ts >= Ts_b are zeros.
 * fsn_fast_mask_out_ragged         mask frames t >= T_b of row b are zeros.
 * (fsn_fast_decoder_input needs no lengths: frame t < T_b + look_ahead takes low-rate frame t / shrink < Ts_b.)
 * Arguments, checks and workspace (fsn_fast_glue_workspace_bytes) as the plain entries, which are these with frames = NULL;
 * every frames[b] = T0 gives their result bit for bit. */
int fsn_fast_spec_rows_ragged(const float* mag, const int* frames, int B, int F, int T0, int look_ahead, float* rows, int Bp, int Fp,
                              void* stream);
int fsn_fast_norm_rows_ragged(const float* x, const int* frames, int look_ahead, int T, int B, int Bp, int C, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int fsn_fast_bottleneck_input_ragged(const float* mel, const float* enc, long ld_enc, const int* frames, int look_ahead, int T, int B,
                                     int Bp, int num_mels, int mel_neighbors, int enc_neighbors, int shrink, float* out, int Np,
                                     int Wp, void* workspace, size_t workspace_bytes, void* stream);
int fsn_fast_mask_out_ragged(const float* o, long ld, const int* frames, int T, int B, int Bp, int F, int look_ahead, float* mask,
                             void* stream);

/* fullsubnet/trainer.py:65-69: torch.nn.utils.clip_grad_norm_(parameters, max_norm) followed by
 * torch.optim.Adam.step() (train.py:55-59: lr, betas, eps 1e-8, no weight decay / amsgrad), fused into
 * two multi-tensor launches.  The arrays are HOST arrays of n_tensors device pointers / element
 * counts.  grads are scaled in place by min(1, max_norm / (total_norm + 1e-6)) exactly like
 * clip_grad_norm_ (max_norm <= 0 disables clipping); total_norm_out (device, may be NULL) receives
 * the unclipped 2-norm.  `step` is the 1-based count of this call (bias corrections).
 * A non-finite gradient norm SKIPS the update (parameters, moments and gradients untouched), as GradScaler.step()
 * does in the reference (trainer.py:69), with no host synchronisation: skipped_steps (device, two words, may be
 * NULL; zero it once) counts the skipped updates in word 0 (word 1 is scratch), and a skipped update does not
 * advance Adam's step count - the kernel uses step - skipped for the bias corrections.
 * grad_scale (device scalar, may be NULL = 1): the loss scale the gradients carry (GradScaler, trainer.py:63-69):
 * they are divided by it first (GradScaler.unscale_), so total_norm_out, the clipping and the update see unscaled
 * gradients; an overflowed (inf / NaN) gradient makes the norm non-finite and the update is skipped as above.
 * found_inf (device scalar, may be NULL): GradScaler's inf flag over ALL of the optimizer's parameter groups; non-zero
 * skips this call's update too, so that the groups of one optimizer skip together like scaler.step does. */
#define FSN_ADAM_MAX_TENSORS 32
typedef struct fsn_adam_cfg {
    float lr, beta1, beta2, eps;
    float max_norm;
    int step;
} fsn_adam_cfg;
size_t fsn_clip_adam_workspace_bytes(int n_tensors, const size_t* numel);
int fsn_clip_adam_step(int n_tensors, float* const* params, float* const* grads, float* const* exp_avg,
                       float* const* exp_avg_sq, const size_t* numel, const fsn_adam_cfg* cfg,
                       float* total_norm_out, const float* grad_scale, const float* found_inf,
                       unsigned* skipped_steps, void* workspace, size_t workspace_bytes, void* stream);

/* ---- residency contract of the persistent kernels ----------------------------------------------------------
 * Four kernels - the full-band chain (forward, BPTT) and the sub-band group kernel (forward, BPTT) - run a whole
 * recurrence as ONE launch whose workgroups hand results to each other step by step; they make progress only while
 * their whole grid is resident.  What the library guarantees by itself: such a launch is only chosen when the grid
 * fits an idle device (from the compiled kernel's occupancy on THAT device; other shapes take the per-step paths),
 * and the library's own persistent launches from different streams (one process) only run side by side when the
 * whole set is provably placeable in any dispatch order (every launch reports grid and occupancy; a launch waits for
 * earlier ones, oldest first, until sum_j grid_j / (occ_j CUs) stays below the fill level at which some CU state
 * could refuse a workgroup of any kernel of the set - e.g. two 192-workgroup chain launches share the chip, two
 * 448-workgroup group launches take turns).  What it
 * cannot control is bounded instead: a FOREIGN kernel holding CUs (an RCCL collective beside DDP's backward, work
 * of another stream) merely delays the workgroups that found no room until it ends - the resident ones wait for
 * them, by the device's wall clock, up to fsn_set_persistent_timeout_ms (default 20 s).  A wait that runs out means
 * the foreign kernel was itself waiting for this one (two processes sharing a GPU each holding part of it, graph
 * replays of two persistent launches on two streams): the launch then finishes with NaN outputs, never garbage and
 * never a hang, the stream's sticky status is raised, and every later persistent launch on that stream returns
 * FSN_ERR_TIMEOUT until fsn_stream_status_clear.  Callers that cannot rule that situation out switch the
 * persistent kernels off (FSN_PERSISTENT_NEVER: the per-step paths, same results, slower for few rows). */
#define FSN_PERSISTENT_AUTO 0
#define FSN_PERSISTENT_NEVER 1
int fsn_set_persistent_mode(int mode);       /* process-wide */
int fsn_set_persistent_timeout_ms(int ms);   /* process-wide, [1, 3600000] */
/* The sticky status of `stream`: *status_out = status word of the first launch that ran out of time (0 = none),
 * *events_out = number of outputs poisoned since the last clear; either may be NULL.  synchronize != 0 waits for the
 * stream first (the record is written by the device when the launch ends).  Returns FSN_ERR_TIMEOUT when raised. */
int fsn_stream_status(void* stream, int synchronize, unsigned* status_out, unsigned* events_out);
int fsn_stream_status_clear(void* stream);
/* What a RAISED record does to later persistent launches on `stream`.  FSN_TIMEOUT_REFUSE (default): they return
 * FSN_ERR_TIMEOUT until the record is cleared - an inference caller must never consume NaN silently.
 * FSN_TIMEOUT_DEFER: they are launched regardless - for a training step in flight (fullsubnet/trainer.py:41-71:
 * forward, loss, backward are ~10 entry points behind autograd, and under DistributedDataParallel,
 * audio_zen/trainer/base_trainer.py:32, a rank that raised in the middle of backward would leave its peers waiting in
 * the gradient all-reduce): the poisoned outputs are NaN, NaN propagates into every gradient, the fused optimizer
 * skips the update on the device (fsn_clip_adam_step), and the caller reads fsn_stream_status once per step. */
#define FSN_TIMEOUT_REFUSE 0
#define FSN_TIMEOUT_DEFER 1
int fsn_stream_timeout_policy(void* stream, int policy);

/* Per-stage kernel timing of the last fsn_enhance / fsn_fullsubnet_forward call made ON `stream` with
 * profiling enabled for THAT stream (hipEvents on it, kept per (device, stream); forces a sync of them when read).
 * Stage ids are listed by fsn_profile_stage_name(); used by bench.py for the roofline line.  */
int fsn_profile_enable(void* stream, int on);
/* Test hook: a launch of a persistent kernel that ran out of time raises a status word and a follow-up kernel turns
 * its output into NaN instead of leaving garbage.  This entry runs that follow-up kernel on caller data:
 * out[0..n) = NaN iff *status (a device word) != 0, and the stream's sticky status is raised like a real event. */
int fsn_debug_poison_if(const void* status, float* out, size_t n, void* stream);
/* Test hook: a foreign kernel - `workgroups` x 256 threads, lds_bytes of LDS each, ~200 registers per lane when
 * heavy != 0 - that holds its CUs for `ms` milliseconds on `stream`.  sink: one device float (never written). */
int fsn_debug_hog(int workgroups, int lds_bytes, int heavy, float ms, float* sink, void* stream);
/* Test hook: persistent launches admitted so far (process-wide), stream waits inserted between them, and launches
 * that did not report their footprint (must stay 0).  Any pointer may be NULL. */
int fsn_debug_persist_stats(unsigned* launches, unsigned* waits, unsigned* unreported);
/* Test / measurement hook: the two-layer training entries (fsn_lstm2_forward_train / fsn_lstm2_backward) under
 * FSN_ARITH_F16 / _BF16 run the 16-bit arithmetic's own persistent kernels (lstm_group16_kernels.hip) where they
 * apply; on = 0 keeps the fp32-era group kernels under that arithmetic (A/B measurements), on = 2 only the round-3 form
 * of the weight-gradient products (operands converted on the fly), on = 3 layer 0's input-side products (dx, dW_ih0) from
 * fp32 gate gradients as in round 5 (the BPTT launch then stores them), on = 1 restores the default. */
int fsn_debug_g16_kernels(int on);
/* 0: the 16-bit-operand weight-gradient products on 192 x 192 tiles also where the 192 x 384 eight-wave form applies (both
 * give bit-identical partial products; the split count differs).  A/B measurements and tests. */
int fsn_debug_tn16h_wide(int on);
/* Test hook that needs no device: the plan of the two-layer training entries under `arith` (FSN_ARITH_F32 / _F16 / _BF16
 * [| FSN_ARITH_SAVES16]) for x rows of ldx columns, decided from the shape alone (and the two switches above).
 * out[0..n) of: 0 the forward runs in the 16-bit arithmetic at all, 1 the backward does, 2 the forward on the 16-bit
 * arithmetic's own kernel, 3 the BPTT on it, 4 the three large weight-gradient products from 16-bit operands in memory
 * (tn16h), 5 their form at K = (T - 1) N (0 none, 1 192 x 192 tiles, 2 192 x 384), 6 dx and dW_ih0 from the 16-bit gate
 * gradients too (in16), 7 the products read the 16-bit h_t of the save slots (h16_saved), 8 rows beside the backward
 * launch (step by step, fp32), 9 its clusters, 10 rows beside the forward launch, 11 its clusters, 12 FSN_ARITH_SAVES16
 * in force (asked for, and both directions on the 16-bit arithmetic's own kernels: otherwise the gates are saved and read in
 * fp32 whatever the flag).  Returns the number of fields written (at most 13), -1 on bad arguments. */
int fsn_debug_lstm2_plan16(int T, int N, int I, long ldx, int H, int arith, int* out, int n);
/* Test hooks: the 16-bit training arithmetic's conversion and weight-gradient / dx products on caller data, each the
 * internal launcher unchanged behind shape, pointer and size checks (the launcher's own refusals - no plan for the shape,
 * alignment, arithmetic - come back as FSN_ERR_ARG with nothing written).  arith: FSN_ARITH_F16 / _BF16 (gemm_tn: _F32 too).
 * to16: dst[0..n) = src rounded to nearest even, n % 4 == 0.
 * gemm_tn16h / gemm_tn16n / gemm_tn: C [M][ldc >= Nc] = A^T B over K rows, A [K][lda], B [K][ldb] 16-bit (gemm_tn: fp32,
 *   rounded on load under a 16-bit arith); tn16n reads 32 columns of B (those beyond Nc zero).  Workspace:
 *   fsn_debug_gemm_tn_workspace_bytes(M, Nc, K).  fsn_debug_tn16_plan: *form = 0 when the 16-bit-operand product has no
 *   plan at this shape (narrow != 0: tn16n, form 0 / 1; else tn16h, 1 = 192 x 192 tiles, 2 = 192 x 384), *splits its K splits.
 * gemm_dx16: dx [rows][lddx] columns 0 .. I - 1 = dg16 [rows][ld16] (16-bit) x w [G][I] (fp32, rounded here); wfrag:
 *   scratch of G x 32 16-bit words. */
size_t fsn_debug_gemm_tn_workspace_bytes(int M, int Nc, long K);
int fsn_debug_tn16_plan(int narrow, int M, int Nc, long K, int* splits, int* form);
int fsn_debug_to16(const float* src, void* dst, size_t n, int arith, void* stream);
int fsn_debug_gemm_tn16h(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                         void* workspace, size_t workspace_bytes, int arith, void* stream);
int fsn_debug_gemm_tn16n(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                         void* workspace, size_t workspace_bytes, int arith, void* stream);
int fsn_debug_gemm_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int Nc, long K,
                      void* workspace, size_t workspace_bytes, int arith, void* stream);
int fsn_debug_gemm_dx16(const void* dg16, long ld16, const float* w, void* wfrag, size_t wfrag_bytes, float* dx, long lddx,
                        long rows, int G, int I, int arith, void* stream);
/* Test hooks that need no device.  fsn_debug_persist_set_fits: 1 when the gate would let n persistent launches with the
 * given chip fractions (grid / (occ x CUs)) and occupancies run side by side, 0 when the newest has to wait.
 * fsn_debug_tn_plan: the K splits a weight-gradient product [M x Nc], K rows, would take (*splits) and the bound the
 * scratch of every caller is sized by (*bound >= *splits must hold for every shape). */
int fsn_debug_persist_set_fits(int n, const double* fracs, const int* occs);
int fsn_debug_tn_plan(int M, int Nc, long K, int arith, int* splits, long* bound);
/* Test hook: fsn_enhance / fsn_fullsubnet_forward run a batch of B utterances as one or several calls of the model core
 * (whole rounds of the persistent kernels, a remainder split by a cost model of the plans - the model has no
 * cross-utterance term); sizes[0..n) = their utterance counts, largest first, n returned (max_sizes >= 80), -1 on bad
 * arguments. */
int fsn_debug_core_chunks(const fsn_fullsubnet_cfg* cfg, int B, int* sizes, int max_sizes);
/* Diagnostic: how the sub-band model of a B-utterance, T-frame call is spread over the device (of its first chunk when the
 * batch runs as several).  plan[0..8) = sub-band rows, 16-row tiles, row tiles per workgroup of the persistent pair, its
 * workgroups (0: the rows run on the group kernel / step launches), left-over tiles beside it, clusters of the group
 * kernel (0: none), full-band model on the chain kernel (0 / 1), chunks of the batch; with n >= 9 also plan[8] = the rows
 * the persistent pair processes summed over ALL chunks (whole rounds and a remainder have different plans).  bench.py
 * prints it per rank and counts the roofline's FLOPs on the rows the persistent launches actually process. */
int fsn_debug_core_plan(const fsn_fullsubnet_cfg* cfg, int B, int T, int* plan, int n);
/* Test hook: the plan of ONE call of the model core, formed by the code the entries themselves use.  row_end < 0: the B
 * utterances whole as a single call (what one chunk of fsn_fullsubnet_forward runs; no chunking is applied here);
 * otherwise the row slice [row_begin, row_end) exactly as fsn_fullsubnet_forward_rows forms it.  plan[0..15) (n >= 15):
 * 0 sub-band rows N, 1 16-row tiles (padding tiles of whole rounds included), 2 padded rows, 3 row tiles per workgroup of
 * the persistent pair, 4 its workgroups, 5 left-over tiles, 6 clusters of the group kernel, 7 tiles beside the group
 * launch, 8 / 9 tiles on the one-workgroup-per-CU step kernel / on the small step kernel of the persistent and step
 * regimes (0 in the other regimes), 10 full-band model on the chain kernel, 11 its padded rows, 12 output layer fused into
 * layer 1's persistent kernel, 13 layer 1 on lstm_rec_x, 14 16-column chunks of the sub-band input.  -1 on bad arguments. */
int fsn_debug_core_call_plan(const fsn_fullsubnet_cfg* cfg, int B, int T, long row_begin, long row_end, int* plan, int n);
/* Test hook: which launchers the last call of this library ON THE CALLING THREAD went through - one 32-bit mask per
 * thread, cleared when an entry that enqueues work is entered.  Bits, from 0: lstm_rec, lstm_rec_in, lstm_rec_x,
 * lstm_step, lstm_step_cu, lstm_wavefront2, lstm2_group, fb_chain, then the model core's sub-band GEMM sites: layer-0
 * projection of rows that run step by step, layer-1 projection, output layer as a GEMM. */
unsigned fsn_debug_core_last_launches(void);
/* Test hooks that need no device: where the arrays of the opaque state blobs lie, formed by the code the entries carve
 * them with (tests/test_gpu_stream_sweep.py writes and reads states through them).
 * fsn_debug_stream_state_layout: the blob of fsn_fullsubnet_stream_step at batch B, which is also the head of the blob of
 * the fsn_fullsubnet_segment_* entries (either norm).  out[0..13) (n >= 13): byte offsets of 0 - 3 the full-band model's
 * h0, h1, c0, c1 [padded rows][fb_hidden] floats, 4 - 7 the sub-band model's [padded rows][sb_hidden], 8 fb_sum [B]
 * doubles, 9 sb_sum [B num_freqs] doubles; 10 / 11 the padded row counts of the full-band / sub-band arrays; 12 the size
 * fsn_fullsubnet_stream_state_bytes returns.
 * fsn_debug_stream_pool_layout: one record of the streaming pool.  out[0..21) (n >= 21): byte offsets into the record of
 * 0 - 3 the full-band h0, h1, c0, c1 [fb_hidden], 4 - 7 the sub-band ones [num_freqs][sb_hidden], 8 fb_sum (double), 9 sb_sum
 * [num_freqs] doubles, 10 steps (int), 11 in_tail, 12 ola_tail, 13 ring_re, 14 ring_im; 15 the bytes of a record; 16 - 20
 * num_freqs, its padded width, fb_hidden, sb_hidden, ring frames.  Both: -1 on bad arguments. */
int fsn_debug_stream_state_layout(const fsn_fullsubnet_cfg* cfg, int B, long* out, int n);
int fsn_debug_stream_pool_layout(const fsn_fullsubnet_cfg* cfg, long* out, int n);
/* ---- training pairs mixed on the device : recipes/dns_interspeech_2020/dataset_train.py ---------------------------
 * The arithmetic of Dataset.snr_mix (dataset_train.py:137-195, with norm_amplitude / tailor_dB_FS / is_clipped of
 * audio_zen/acoustics/feature.py:99-114) as deterministic functions of host-drawn descriptors: every random draw stays
 * with the caller (fullsubnet_amd/mix.py).  The source audio lives in three device slabs - clean speech, noise, room
 * impulse responses - of fp32 samples (slab_format FSN_SLAB_F32) or 16-bit PCM read as v / 32768 (FSN_SLAB_I16, what a
 * 16-bit wav loads as); offsets and lengths count samples.  `items`, `segs`, `h_off` and `h_len` are DEVICE pointers;
 * the calls copy nothing, never synchronise and can be captured in a graph.  1 <= L <= FSN_MIX_MAX_L.
 *
 * Convolution: y[b, n] = sum_k h_b[k] x[b, n - k] for 0 <= n < L, i.e. fftconvolve(x_b, h_b)[:L]; taps from L on cannot
 * reach those outputs and are never read; h_len[b] <= 0 copies the row.  y must not alias x.  It is an FFT convolution
 * of circular length N = 2^k >= L + min(h, L) - 1 in fp64 (DESIGN "mixing on the device").  The host cannot see h_len, so
 * N follows from the WORKSPACE: the largest transform workspace_bytes pays for, at most the one of max_h_len = L; the
 * size query is what states the longest response.  A row whose response is longer than that transform carries
 * (workspace sized for a smaller max_h_len) is written as NaN - never a silently aliased result.
 *
 * fsn_mix_pairs, per row: the clean row is clean_slab[clean_off, clean_off + clean_len) zero-padded to L
 * (feature.py:subsample); the noise row is silence except where a segment copies noise_slab[src_off, src_off + len) to
 * [dst_off, dst_off + len) (the files and 0.2 s silences of _select_noise_y after its crop); then
 *   1. the clean row is convolved with the response (rir_len > 0);
 *   2. c / (max|c| + eps) levelled to target_dbfs, the same for the noise;
 *   3. noise gain clean_rms / 10^(snr / 20) / (noise_rms + eps), noisy = clean + gain * noise;
 *   4. noisy levelled to noisy_target_dbfs, clean scaled by the same factor;
 *   5. if any |noisy| > 0.999, both divided by max|noisy| / (0.99 - eps).
 * Sums and scalars are fp64; noisy / clean [B][L] are rounded to fp32 once.  Rows do not depend on one another: a
 * descriptor gives the same bits in any row of any batch.  Descriptor fields the host cannot see are clamped on the
 * device so that nothing is WRITTEN outside the outputs and the workspace (clean_len to [0, L], segments to the row);
 * the offsets into the slabs are the caller's responsibility.
 * Refused without a launch (size queries return 0, fsn_last_error has the reason): L outside the range, B < 1, negative
 * lengths, a NULL or misaligned (256 bytes) or short workspace. */
#define FSN_SLAB_F32 0
#define FSN_SLAB_I16 1
#define FSN_MIX_MAX_L 131072
typedef struct fsn_mix_seg {
    long src_off; /* first sample in the noise slab */
    int dst_off;  /* first sample of the row it lands on */
    int len;
} fsn_mix_seg;
typedef struct fsn_mix_item {
    long clean_off;
    int clean_len;            /* <= L */
    int seg_begin, seg_count; /* this row's slice of the segment table */
    long rir_off;
    int rir_len;              /* 0: no reverb */
    float snr_db, target_dbfs, noisy_target_dbfs;
} fsn_mix_item;
size_t fsn_conv_rows_workspace_bytes(int B, int L, int max_h_len);
int fsn_conv_rows(const float* x, int B, int L, const void* h_slab, int slab_format, const long* h_off, const int* h_len,
                  float* y, void* workspace, size_t workspace_bytes, void* stream);
size_t fsn_mix_workspace_bytes(int B, int L, int max_rir_len);
int fsn_mix_pairs(const void* clean_slab, const void* noise_slab, const void* rir_slab, int slab_format,
                  const fsn_mix_item* items, const fsn_mix_seg* segs, int n_segs, int B, int L, float eps, float* noisy,
                  float* clean, void* workspace, size_t workspace_bytes, void* stream);

/* ---- dereverberation targets : audio_zen/acoustics/rvb.py (reverberation_time_shortening) ---------------------------
 * The training target of "Speech Dereverberation With a Reverberation Time Shortening Target" (Zhou, Zhu, Li 2022): the
 * clean row convolved with a response whose tail, from after_max samples behind its peak on, decays faster.  Added
 * without a new FSN_ABI_VERSION (additive; a binding looks the three symbols up by name).  Every pointer is a DEVICE
 * pointer, the descriptor tables included; the calls copy nothing, never synchronise and can be captured in a graph.
 *
 * fsn_rir_shorten, per row b: the response h_b = h_slab[h_off[b], h_off[b] + h_len[b]) in either slab format, exactly
 * as fsn_conv_rows takes it, and a descriptor targets[b]:
 *   mode 0            out = h                                                    (the response, copied)
 *   mode 1 shortened  idx = the FIRST index of max |h_b| over the WHOLE response (np.argmax(np.abs(rir))),
 *                     N1 = idx + after_max, win[n] = 1 for n < N1 and 10^(-q (n - N1)) from N1 on, formed in fp64 and
 *                     rounded to fp32; out[n] = fp32(h[n]) * win[n] as ONE fp32 product - the reference's arithmetic, a
 *                     float32 window times a float32 response
 *   mode 2 early      win[n] = 0 from N1 on: the direct path and what arrives within after_max samples of it
 * The host forms q = 3 / (target_T60 sr) - 3 / (original_T60 sr) and after_max = floor(time_after_max sr); q is a double
 * because its rounding error in fp32 would grow into win through exponents of 100 and more.  One workgroup per response:
 * the arg-max is a fixed-order reduction over (value, lowest index) pairs, the window and the product follow in the same
 * launch.  out [B][ld] (zeros behind h_len[b]); win [B][ld] (NULL: not wanted; zeros behind h_len[b]); idx [B] (NULL: not
 * wanted; 0 for an empty response).  max_h_len states the longest response of the table: the host cannot see h_len, and
 * a longer row is cut at ld - nothing is written outside [B][ld].  The descriptors are in device memory too: a mode
 * outside 0 - 2 cannot be refused by the host and turns its row (out, win) into NaN; the packers of fullsubnet_amd/mix.py
 * refuse it before anything is uploaded.
 * Refused without a launch (fsn_last_error has the reason): a NULL h_slab, h_off, h_len, targets or out, B < 1,
 * max_h_len < 0, ld < max_h_len, an unknown slab_format.
 *
 * fsn_mix_pairs_target: fsn_mix_pairs plus a third output.  noisy and clean are EXACTLY what fsn_mix_pairs writes for
 * the same items - every level scalar of steps 2 - 5 still comes from the reverberant row - and clean may be NULL.
 * target = conv(clean row, shortened response)[:L] times the scalar chain the clean row gets (1 / (max|c| + eps), the
 * target_dbfs factor, the mixture's level factor, the clip divisor), rounded to fp32 once: the shortened counterpart of
 * `clean` at the same gain, time-aligned with the mixture, and noisy - clean is untouched.  Rows with rir_len == 0 or
 * mode 0 get target == clean bit for bit.  The second convolution runs on the plan of the first with the shortened taps
 * (fp32, in the workspace); silence and all-zero responses give exact zeros, a response the workspace's transform cannot
 * carry gives NaN in all three outputs, and a descriptor gives the same bits in any row of any batch. */
typedef struct fsn_mix_target {
    double q;      /* decay added per sample, in decades: win = 10^(-q (n - N1)) */
    int after_max; /* samples behind the peak that stay untouched */
    int mode;      /* 0: the response as it is, 1: shortened, 2: early */
} fsn_mix_target;
int fsn_rir_shorten(const void* h_slab, int slab_format, const long* h_off, const int* h_len, int B, int max_h_len,
                    const fsn_mix_target* targets, float* out, int ld, float* win, int* idx, void* stream);
size_t fsn_mix_target_workspace_bytes(int B, int L, int max_rir_len);
int fsn_mix_pairs_target(const void* clean_slab, const void* noise_slab, const void* rir_slab, int slab_format,
                         const fsn_mix_item* items, const fsn_mix_seg* segs, int n_segs, int B, int L, float eps,
                         const fsn_mix_target* targets, float* noisy, float* clean, float* target, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- validation metrics on the device : audio_zen/metrics.py (STOI, SI_SDR) ------------------------------------------
 * Row b of clean / reference and of estimate [B][L_max] (fp32) holds lengths[b] samples (device pointer; a value is
 * clamped into [0, L_max]; NULL: every row holds L_max); nothing past a row's length is read.  All arithmetic is fp64,
 * every sum runs in a fixed order and no row's result depends on the rows around it: a pair gives the same bits alone
 * and in any batch.  The calls copy nothing, never synchronise, can be captured in a graph and use no library state
 * beyond the per-stream record of every entry.  Added without a new FSN_ABI_VERSION (additive; a binding looks the
 * three symbols up by name).
 *
 * fsn_stoi: the short-time objective intelligibility of Taal, Hendriks, Heusdens and Jensen (2011), not extended, as
 * DESIGN "metrics on the device" pins it constant by constant: polyphase resampling to 10 kHz (sr = 10000: none,
 * 16000: 5 / 8, 48000: 5 / 24, Kaiser-windowed sinc formed on the device), removal of the 256-sample frames (hop 128)
 * of the CLEAN row more than 40 dB below its loudest, 512-point spectra, 15 one-third-octave bands from 150 Hz,
 * clipped and normalised correlations over every 30 consecutive frames.  d [B] (device, fp64):
 *   - a row that is left with fewer than 30 spectral frames: 1e-5 exactly;
 *   - an all-zero clean row or an all-zero estimate row (of 30 frames or more): 0, never NaN (the "+ eps" terms).
 * fsn_si_sdr: out_db[b] = 10 log10(|a r|^2 / |e - a r|^2), a = <r, e> / <r, r>, the residual summed in a second
 * pass (the expanded form cancels at high SDR).  An all-zero or empty reference row gives NaN, estimate == a r gives +inf,
 * as the formula does.
 * Refused with FSN_ERR_ARG, a message and no launch (the size query returns 0): an sr other than the three, B < 1,
 * L_max < 1, a NULL pointer, a NULL, misaligned (256 bytes) or short workspace. */
size_t fsn_stoi_workspace_bytes(int B, int L_max, int sr);
int fsn_stoi(const float* clean, const float* estimate, const int* lengths, int B, int L_max, int sr, double* d,
             void* workspace, size_t workspace_bytes, void* stream);
int fsn_si_sdr(const float* reference, const float* estimate, const int* lengths, int B, int L_max, double* out_db,
               void* stream);

/* ---- sample-rate conversion on the device : what the reference gets from librosa.load(path, sr=sr) ------------------
 * A rational-ratio polyphase FIR resampler, scipy.signal.resample_poly's construction with three design parameters
 * (DESIGN "resampling on the device" pins it).  For a row x of n fp32 samples, sr_in -> sr_out and (zeros, beta, rolloff):
 *   u = sr_out / g, d = sr_in / g, g = gcd;  P = max(u, d), H = zeros P, fc = rolloff / P;
 *   g[t] = kaiser(2H + 1, beta)[t] fc sinc(fc t) for t = -H .. H,  h = u g / sum(g)               (fp64)
 *   n_out = ceil(n u / d),  y[k] = fp32(sum_m h[k d + H - m u] x[m]) over the m in [0, n) whose tap exists  (fp64 sums)
 * Nothing outside the row is read: no reflection, no carried state.  u == d == 1 copies the row bit for bit.
 * (zeros, beta, rolloff) = (10, 5.0, 1.0) is resample_poly(x, u, d) with its default window; (32, 12.0, 0.92) is a
 * steeper anti-alias filter (-43 dB at the new Nyquist rate, below -120 dB past 9 / 8 of it, for 3 : 1).
 *
 * Row b of x [B][L_max] holds lengths[b] samples (device pointer; a value is clamped into [0, L_max]; NULL: every row
 * holds L_max); nothing past a row's length is read.  y [B][L_out_max]: row b receives its n_out samples and zeros from
 * there to L_out_max; out_lengths (device, [B], may be NULL) receives n_out.  The taps are formed on the device by the
 * call itself (workspace), so a call copies nothing, never synchronises and can be captured in a graph; the order of an
 * output's sum depends on (u, d, design, k) alone, so a row has the same bits alone and in any batch; an all-zero row
 * gives exact zeros.  Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name).
 *
 * fsn_resample_out_length: ceil(n u / d) on the host, no device call; -1 for rates < 1 or n < 0.
 * fsn_resample_taps: h in natural order, h[t + H], as fp64 into device memory of h_count >= 2H + 1 doubles.
 * fsn_debug_resample_plan (test hook): out[0 .. n) = u, d, H, taps, taps per phase, row stride of the polyphase table,
 * outputs per workgroup, the longest row one workgroup covers, input samples a workgroup stages, table in LDS (0 / 1).
 * Refused with FSN_ERR_ARG, a message and no launch (the size query returns 0): a rate < 1, zeros < 1, beta outside
 * [0, FSN_RESAMPLE_MAX_BETA], rolloff outside (0, 1], max(u, d) > FSN_RESAMPLE_MAX_P, 2H + 1 > FSN_RESAMPLE_MAX_TAPS, a ratio and filter whose
 * smallest workgroup tile (8 u outputs) lies over more than 24576 input samples, B outside [1, 65535], L_max < 1,
 * L_out_max smaller than ceil(L_max u / d), y == x, a NULL pointer, a NULL, misaligned (256 bytes) or short workspace. */
#define FSN_RESAMPLE_MAX_P 4096
#define FSN_RESAMPLE_MAX_TAPS 262145
#define FSN_RESAMPLE_MAX_BETA 256
long fsn_resample_out_length(long n, int sr_in, int sr_out);
size_t fsn_resample_workspace_bytes(int sr_in, int sr_out, int zeros, double beta, double rolloff);
int fsn_resample_taps(int sr_in, int sr_out, int zeros, double beta, double rolloff, double* h, size_t h_count,
                      void* stream);
int fsn_resample(const float* x, const int* lengths, int B, int L_max, int sr_in, int sr_out, int zeros, double beta,
                 double rolloff, float* y, int L_out_max, int* out_lengths, void* workspace, size_t workspace_bytes,
                 void* stream);
int fsn_debug_resample_plan(int sr_in, int sr_out, int zeros, int* out, int n);

/* ---- sample-rate conversion of streams : sessions that receive their input chunk by chunk ---------------------------
 * The same filter and the same sums as fsn_resample (notation above; J = ceil((2H + 1) / u) taps per phase), for up to
 * `capacity` sessions that each carry their last J - 1 input samples in a slot of one device blob.  Output k of a session
 * has newest input q(k) = floor((k d + H) / u) and is fp32(sum_{j < J} poly[(k d + H) mod u][j] x[q - j]), an fp64 fma
 * chain in that order with x[m] = 0 for m < 0 - so whatever the chunking, a session's outputs are bit for bit those of
 * fsn_resample on its whole input (DESIGN "resampling streams").
 *   before the end of input, after n_in samples the outputs k < ready(n_in) may be emitted: ready = 0 while
 *     n_in u <= H, else floor((n_in u - H - 1) / d) + 1 - those whose newest input has arrived;
 *   at the end (`final`, n samples in all) the rest up to ceil(n u / d), with x[m] = 0 for m >= n;
 *   u == d == 1 passes chunks through bit for bit with no delay (ready(n_in) = n_in).
 * The delay this adds is H / u input samples: 30 samples at 48 kHz in (0.625 ms) for 48 -> 16 kHz and 10 samples at
 * 16 kHz in (0.625 ms) for 16 -> 48 kHz with zeros = 10; 2 ms each way with zeros = 32.
 *
 * All counts live with the caller (fsn_resample_stream_ready is host arithmetic, no device call; -1 for a refused
 * request).  The blob: a header (the taps [2H + 1] and the polyphase table [u][Js], formed on the device by
 * fsn_resample_stream_init) and `capacity` slots of two history buffers [J - 1] each; all zeros is a fresh slot, and
 * init clears every slot.  fsn_resample_stream_push is ONE launch for the n listed sessions: row i of x [n][C_max] holds
 * item i's chunk, row i of y [n][O_max] receives its `count` outputs k0 .. k0 + count - 1 and zeros from there to O_max.
 * `items` is a device table the caller writes (n entries).  An item reads buffer `parity` of its slot and, when its chunk
 * is not empty and it is not final, writes the session's new history into the other one: the caller flips a session's
 * parity after exactly those pushes (a final push leaves the slot stale: reset it before it is used again).  Chunks of 0
 * and 1 samples are legal, and chunks longer than the history.  What an item says is clamped on the device (a slot
 * outside [0, capacity) or a position outside [0, 2^40) writes zeros only; n_chunk into [0, C_max]; count into [0, O_max]); slots must be distinct.  Slots
 * that are not listed are not written.  The calls never synchronise and copy nothing; a session has the same bits alone
 * and beside any others; an all-zero input gives exact zeros.  fsn_resample_stream_reset zeroes the listed slots (device
 * list of n ids).  Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name).
 * Refused with FSN_ERR_ARG, a message and no launch (the size query returns 0): what fsn_resample refuses of rates and
 * design, a filter of more than 16383 taps per phase, capacity outside [1, 65535], n < 1 or n > capacity, a state blob
 * that is NULL, not 256-byte aligned or not of exactly fsn_resample_stream_state_bytes, a NULL pointer, C_max or O_max
 * outside [1, 2^30]. */
typedef struct fsn_resample_stream_item {
    long long slot;      /* [0, capacity) */
    long long n_chunk;   /* samples in row i of x */
    long long final;     /* 0 / 1: the session's input ends with this chunk */
    long long parity;    /* 0 / 1: the history buffer that holds the samples before this chunk */
    long long n_before;  /* samples the session received before this chunk */
    long long k0;        /* first output to write = outputs emitted so far */
    long long count;     /* outputs to write */
    long long reserved;  /* 0 */
} fsn_resample_stream_item;
long fsn_resample_stream_ready(long n_in, int final, int sr_in, int sr_out, int zeros);
size_t fsn_resample_stream_state_bytes(int sr_in, int sr_out, int zeros, int capacity);
int fsn_resample_stream_init(void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros, double beta,
                             double rolloff, void* stream);
int fsn_resample_stream_push(void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros,
                             const fsn_resample_stream_item* items, int n, const float* x, int C_max, float* y, int O_max,
                             void* stream);
int fsn_resample_stream_reset(void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros,
                              const int* slots, int n, void* stream);

/* ---- bidirectional nn.LSTM / nn.GRU layer (bidirectional = True of sequence_model.py:52-66) ------------------------------
 * One layer, both directions: step launch s advances the forward direction at frame s and the reverse one at frame
 * T - 1 - s, so a layer is T dependent launches (birnn_step_kernels.hip); the input projection of both directions is one
 * GEMM.  Conventions of fsn_lstm_layer_forward / _backward (time-major rows, N % 16 == 0, H % 64 == 0 - smaller sizes run
 * zero-padded -, h0 = c0 = 0, save == NULL: inference, dx may be NULL) with these specifics:
 *   weights in torch's layout with a leading direction axis: w_ih [2][gH][I], w_hh [2][gH][H], b_ih / b_hh [2][gH] (g = 4
 *     gates i, f, g, o / 3 gates r, z, n); direction 0 is forward, direction 1 torch's `*_reverse`; gradients likewise;
 *   hseq [T][N][ldh], ldh >= 2 H and a multiple of 4: the forward direction's h_t in columns [0, H), the reverse one's in
 *     [H, 2 H) - torch's output layout; dh [T][N][lddh] likewise; columns 2 H .. ldh - 1 of hseq and I .. lddx - 1 of dx are
 *     never written;
 *   save: fsn_*_bilayer_save_bytes, workspaces exactly the queries' sizes or more;
 *   a direction's results do not depend on its slot: (w_r, w_f) on the frame-reversed input gives the two halves swapped
 *     and frame-reversed, bit for bit, weight gradients included.
 * Bad arguments (N % 16, H % 64, T < 1, ldh < 2 H, a NULL pointer): FSN_ERR_ARG with fsn_last_error text and no launch;
 * the size queries return 0.  There is no `_state` form: the reverse direction starts from the LAST frame, so a
 * bidirectional layer cannot be streamed chunk by chunk.  fsn_debug_bilayer_last_step_launches (test hook): the recurrent
 * step launches the calling thread's last bilayer call issued (T).  Additive entries (no new FSN_ABI_VERSION). */
size_t fsn_lstm_bilayer_save_bytes(int T, int N, int H);
size_t fsn_lstm_bilayer_fwd_workspace_bytes(int T, int N, int I, int H);
int fsn_lstm_bilayer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                             const float* b_hh, int T, int N, int I, int H, float* hseq, long ldh, void* save,
                             size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t fsn_lstm_bilayer_bwd_workspace_bytes(int T, int N, int I, int H);
int fsn_lstm_bilayer_backward(const float* dh, long lddh, const float* x, long ldx, const float* w_ih, const float* w_hh,
                              int T, int N, int I, int H, const float* hseq, long ldh, const void* save, float* dx,
                              long lddx, float* dw_ih, float* dw_hh, float* db, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t fsn_gru_bilayer_save_bytes(int T, int N, int H);
size_t fsn_gru_bilayer_fwd_workspace_bytes(int T, int N, int I, int H);
int fsn_gru_bilayer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                            const float* b_hh, int T, int N, int I, int H, float* hseq, long ldh, void* save,
                            size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream);
size_t fsn_gru_bilayer_bwd_workspace_bytes(int T, int N, int I, int H);
int fsn_gru_bilayer_backward(const float* dh, long lddh, const float* x, long ldx, const float* w_ih, const float* w_hh,
                             int T, int N, int I, int H, const float* hseq, long ldh, const void* save, float* dx,
                             long lddx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace,
                             size_t workspace_bytes, void* stream);
unsigned fsn_debug_bilayer_last_step_launches(void);

/* ---- Fast FullSubNet, streaming: the model on k more frames with carried state ---------------------------------------
 * fsn_fullsubnet_stream_step's contract for recipes/dns_interspeech_2020/fast_fullsubnet/model.py:143-202 under the
 * cumulative norm (DESIGN "Fast FullSubNet as a stream" derives why every stage is causal).  mag [B, 1, F, k] are the next
 * k input frames of the model (the caller appends the look_ahead zero frames of model.py:161 at the end of the stream),
 * steps_done the number of frames passed in before this call, crm_out [B, 2, F, k] the model output of exactly these steps
 * (step t is the compressed mask of frame t - look_ahead; the caller does the matching, so look_ahead is no field of the
 * configuration).  `state` (fsn_fast_stream_state_bytes, zero-filled for a new stream) carries (h, c) of encoder.0,
 * encoder.1, decoder_lstm.0, decoder_lstm.1 (B rows padded to 16) and of the bottleneck's layers (B num_mels rows), the
 * fp64 running sums of the mel norm [B] and of the unit norm [B num_mels], the fp32 partial sum of the open down-sampling
 * block [B][num_mels][W] (W = 2 mel_neighbors + 1 + 2 enc_neighbors + 1; added in frame order, divided by `shrink` once
 * the block is whole, zero while no block is open) and the last bottleneck output [B][num_mels] held for up-sampling.  Any
 * chunking of the same frames gives the same masks and the same final state bit for bit; a call in which no low-rate
 * frame completes (no t in [steps_done, steps_done + k) with t % shrink == 0) does not run the bottleneck.
 * Configuration: F = 257 and num_mels = 64 (the block widths are literals in the reference), shrink >= 1, neighbours
 * 0 .. 7, bn_hidden 128, 256, 384 or 512 with bn_layers 1 or 2, LSTM cells, norm = FSN_NORM_CUMULATIVE_LAPLACE.
 * Anything else: FSN_ERR_ARG with fsn_last_error text; the size queries (which need no device) return 0, as they do for B
 * or k outside 1 .. 4096.
 * Weights: fsn_fast_stream_pack copies them once into MFMA-fragment order (fsn_fast_stream_packed_bytes).  The tensors of
 * fsn_fast_params are nn.LSTM / nn.Linear tensors with every hidden size padded to a multiple of 64 (encoder.1: 257 ->
 * 320 units, zero weights and biases in the padding) and the input widths that follow from it: mel_w [64][F] (the
 * filterbank transposed); enc0 I 64, H 384; enc1 I 384, H 320, enc1_fc_w [64][320]; bn layer 0 I W, H bn_hidden, layer 1
 * (bn_layers = 2, else NULL) I = H = bn_hidden, bn_fc_w [1][bn_hidden]; dec0 I 128, H 512; dec1 I 512, H 512, dec1_fc_w
 * [2 F][512].  A layer is w_ih [4H][I], w_hh [4H][H], b_ih [4H], b_hh [4H].
 * fsn_debug_fast_stream_state_layout (test hook, no device): out[0..21) (n >= 21): byte offsets of 0 / 1 encoder.0's h, c
 * [rows][384], 2 / 3 encoder.1's [rows][320], 4 / 5 decoder_lstm.0's [rows][512], 6 / 7 decoder_lstm.1's [rows][512], 8 / 9
 * the bottleneck's layer 0 h, c [B num_mels][bn_hidden], 10 / 11 its layer 1 (-1 with one layer), 12 the mel norm's sums
 * [B] doubles, 13 the unit norm's sums [B num_mels] doubles, 14 the open block's partial sum [B][num_mels][W] floats, 15
 * the held bottleneck output [B][num_mels] floats; 16 the padded row count of 0 - 7, 17 the bottleneck's row count, 18
 * encoder.1's padded hidden size, 19 W, 20 the size fsn_fast_stream_state_bytes returns.  -1 on bad arguments.
 * Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name). */
typedef struct fsn_fast_cfg {
    int F;              /* STFT bins, 257 */
    int num_mels;       /* 64 */
    int shrink;         /* shrink_size >= 1 */
    int mel_neighbors;  /* noisy_input_num_neighbors */
    int enc_neighbors;  /* encoder_output_num_neighbors */
    int bn_hidden;
    int bn_layers;
    int norm;           /* FSN_NORM_CUMULATIVE_LAPLACE */
} fsn_fast_cfg;
typedef struct fsn_fast_params {
    const float* mel_w;
    const float *enc0_w_ih, *enc0_w_hh, *enc0_b_ih, *enc0_b_hh;
    const float *enc1_w_ih, *enc1_w_hh, *enc1_b_ih, *enc1_b_hh, *enc1_fc_w, *enc1_fc_b;
    const float *bn_w_ih_l0, *bn_w_hh_l0, *bn_b_ih_l0, *bn_b_hh_l0;
    const float *bn_w_ih_l1, *bn_w_hh_l1, *bn_b_ih_l1, *bn_b_hh_l1, *bn_fc_w, *bn_fc_b;
    const float *dec0_w_ih, *dec0_w_hh, *dec0_b_ih, *dec0_b_hh;
    const float *dec1_w_ih, *dec1_w_hh, *dec1_b_ih, *dec1_b_hh, *dec1_fc_w, *dec1_fc_b;
} fsn_fast_params;
size_t fsn_fast_stream_packed_bytes(const fsn_fast_cfg* cfg);
int fsn_fast_stream_pack(const fsn_fast_cfg* cfg, const fsn_fast_params* w, void* packed, size_t packed_bytes, void* stream);
size_t fsn_fast_stream_state_bytes(const fsn_fast_cfg* cfg, int B);
size_t fsn_fast_stream_workspace_bytes(const fsn_fast_cfg* cfg, int B, int k);
int fsn_fast_stream_step(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes, int steps_done,
                         const float* mag, int B, int k, float* crm_out, void* workspace, size_t workspace_bytes,
                         void* stream);
int fsn_debug_fast_stream_state_layout(const fsn_fast_cfg* cfg, int B, long* out, int n);

/* ---- Fast FullSubNet, recordings of any length: the model in segments under the offline norm ---------------------------
 * The fsn_fullsubnet_segment_* contract for Fast FullSubNet with norm = FSN_NORM_OFFLINE_LAPLACE (the shipped norm).  The
 * one-call path stops at 65 535 frames and its memory grows with the recording at hidden-state width; here the model runs
 * on k (1 .. 4096) steps at a time.  What lives for the whole recording is the caller's: planes of F floats per frame
 * (magnitude, mask) and two time-major planes of num_mels floats per step, mel and enc [Tp][Bp][64] (Bp = B rounded up to
 * 16, Tp = T_max + look_ahead), of which a segment is the contiguous slice [k][Bp][64] at step frames_done.  Everything of
 * hidden-size width is inside `workspace` (fsn_fast_segment_workspace_bytes(cfg, B, k), one size for all passes).
 *
 * offline_laplace_norm divides by ONE mean per utterance and the model applies it twice (model.py:170,187): to the mel
 * spectrum and to the down-sampled unit tensor.  A recording therefore takes three passes over its segments, each pass in
 * frame order over the T_max + look_ahead model steps (the caller appends the look_ahead zero frames of model.py:161), one
 * pass finished before the next begins:
 *   1. fsn_fast_segment_stats: mag [B, 1, F, k] -> mel_out [k][Bp][64] (the filterbank product, padding rows zero); every
 *      frame's 64-band sum is added to an fp64 accumulator [B], in frame order.
 *   2. fsn_fast_segment_encoder: mel / den_mel[b], den_mel[b] = float(sum / (64 total_frames[b])) + 1e-5f, through the
 *      encoder pair from the carried (h, c) -> enc_out [k][Bp][64].  The unit windows of mel and enc_out are down-sampled
 *      as a running block sum that continues across segment edges, and every low-rate frame of row b that completes at a
 *      step t < total_frames[b] adds the fp64 sum of its 64 W fp32 values to a second accumulator [B].  The closing block
 *      counts: when (total_frames[b] - 1) % shrink != 0 the reference averages the last, shorter block over the frames it
 *      has (model.py:117-127) and that low-rate frame enters the utterance mean, although up-sampling never reads it.
 *      Steps at or beyond total_frames[b] add nothing.
 *   3. fsn_fast_segment_decoder: the low-rate frames of whole blocks that complete in the segment, divided by den_unit[b] =
 *      float(sum / (64 W Ts_b)) + 1e-5f with Ts_b = 1 + ceil((total_frames[b] - 1) / shrink), through the bottleneck from
 *      the carried (h, c); the held output joined to enc, the decoder pair -> crm_out [B, 2, F, k].  Step s is the
 *      compressed mask of frame s - look_ahead, as in fsn_fast_stream_step.
 * frames_done: model steps passed to THIS pass before the call.  total_frames (device memory, [B]): row b's own
 * T_b + look_ahead >= 2.  In a ragged batch every row runs to the longest row's end; a row's mag must be zero from its frame
 * T_b on (its mel is then exactly zero there), and only the divisors and the second sum depend on total_frames.
 * The order of every sum depends on the frames alone: two segmentations of one recording give the same divisors, the same
 * masks and the same state bit for bit.
 *
 * `state` (fsn_fast_segment_state_bytes(cfg, B), caller-owned, all zeros for a fresh recording) begins with
 * fsn_fast_stream_step's layout (pass 2 carries the encoder pair's (h, c) there, pass 3 the bottleneck's and the decoder
 * pair's, the open block's partial sum and the held output); behind it lie the two fp64 accumulators [B] each and the block
 * sum [B][num_mels][W] of pass 2's statistic, a field of its own: nothing is cleared between the passes.  `packed`:
 * fsn_fast_stream_pack's blob (its layout does not depend on the norm).  fsn_fast_segment_divisors writes den_mel and
 * den_unit (device memory, [B] each) as the passes form them; call it after pass 2 for den_unit.
 * FSN_ERR_ARG with fsn_last_error text (the size queries, which need no device, return 0): what fsn_fast_stream_step refuses
 * of a configuration, B or k outside 1 .. 4096, and any norm but FSN_NORM_OFFLINE_LAPLACE - the causal norm needs no passes:
 * run fsn_fast_stream_step over the same segments.  FSN_ERR_WORKSPACE for a short state or workspace buffer, before anything
 * is launched.
 * fsn_debug_fast_segment_state_layout (test hook, no device): out[0..25) (n >= 25): 0 - 15 as
 * fsn_debug_fast_stream_state_layout, 16 / 17 the byte offsets of the mel and the unit accumulator [B] doubles, 18 of the
 * statistic's block sum [B][num_mels][W] floats, 19 where fsn_fast_stream_step's fields end, 20 the padded row count of
 * 0 - 7, 21 the bottleneck's row count, 22 encoder.1's padded hidden size, 23 W, 24 the size fsn_fast_segment_state_bytes
 * returns.  -1 on bad arguments.  Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name). */
size_t fsn_fast_segment_state_bytes(const fsn_fast_cfg* cfg, int B);
size_t fsn_fast_segment_workspace_bytes(const fsn_fast_cfg* cfg, int B, int k);
int fsn_fast_segment_stats(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes, const float* mag, int B,
                           int k, float* mel_out, void* workspace, size_t workspace_bytes, void* stream);
int fsn_fast_segment_encoder(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes, int frames_done,
                             const int* total_frames, const float* mel, int B, int k, float* enc_out, void* workspace,
                             size_t workspace_bytes, void* stream);
int fsn_fast_segment_decoder(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes, int frames_done,
                             const int* total_frames, const float* mel, const float* enc, int B, int k, float* crm_out,
                             void* workspace, size_t workspace_bytes, void* stream);
int fsn_fast_segment_divisors(const fsn_fast_cfg* cfg, const void* state, size_t state_bytes, const int* total_frames, int B,
                              float* den_mel, float* den_unit, void* stream);
int fsn_debug_fast_segment_state_layout(const fsn_fast_cfg* cfg, int B, long* out, int n);

/* ---- Fast FullSubNet, streaming pool: sessions at their own block phases ------------------------------------------------
 * fsn_fast_stream_step for streams that are NOT in lockstep, as fsn_fullsubnet_stream_pool_step is for FullSubNet.  `state`
 * is a pool of `capacity` slots (1 .. 4096), fsn_fast_stream_pool_state_bytes(cfg, look_ahead, capacity) bytes = capacity
 * equal records, slot s at byte s * (state_bytes / capacity), each 256-byte aligned.  A record holds what ONE stream of
 * fsn_fast_stream_step carries ((h, c) of the five blocks, both norms' fp64 sums, the open block's partial sum, the held
 * bottleneck output), the slot's own step count (on the device: the kernels read and advance it) and the transform state of
 * the two transform entries (look_ahead, 0 .. 64, sizes its ring of spectra; fsn_fast_cfg has no such field).  All zeros is
 * a fresh pool; fsn_fast_stream_pool_reset returns the n listed slots to that state (stream-ordered).
 *
 * fsn_fast_stream_pool_step advances the n listed slots (`slots`: device memory, n DISTINCT ids, 1 <= n <= capacity) by k
 * model steps, each from its own step count: row i of mag [n, 1, F, k] and crm_out [n, 2, F, k] belongs to slots[i] and is
 * what fsn_fast_stream_step gives a batch of one with the same history (to the rounding of the recurrent kernels, which
 * are chosen by the call's row count; the same calls on a fresh pool give the same bits).  A window of k steps holds lo =
 * k / shrink or hi = ceil(k / shrink) multiples of shrink, so a slot completes lo or hi low-rate frames, as its count
 * decides.  ORDER: the slots that complete hi frames come first and n_long says how many they are (all n when shrink
 * divides k: anything else is refused); the bottleneck then runs lo steps on all rows and one more on the first n_long 64.
 * With lo == 0 and n_long == 0 it does not run and no bottleneck field of a listed record is written.  The call checks the
 * order on the device against the records' own counts: on a mismatch (or a count that would pass 2^31 - 1) crm_out is all
 * NaN, the stream's status record is raised (fsn_stream_status; fsn_stream_status_clear), the return value is still FSN_OK
 * - the host does not wait for the device - and the listed records are unspecified: a caller's error, like a repeated id.
 * Nothing is read or written outside the blob and the workspace either way.  Slots that are not listed are not written.
 * A row whose id is outside [0, capacity) is skipped on either side of n_long (its crm_out row is finite, no state is
 * touched).  FSN_ERR_ARG: what fsn_fast_stream_step refuses (configuration; n, k outside 1 .. 4096), capacity outside
 * 1 .. 4096, n outside 1 .. capacity, n_long outside 0 .. n, look_ahead outside 0 .. 64; the size queries need no device and
 * return 0 then.
 *
 * fsn_fast_stream_pool_analysis / _synthesis: fsn_stream_pool_analysis / _synthesis (same arguments, same kernels) on the
 * transform fields of these records.
 *
 * fsn_debug_fast_stream_pool_layout (test hook, no device): out[0..28) (n >= 28): byte offsets into a record of 0 - 7 h, c
 * of encoder.0 [384], encoder.1 [320], decoder_lstm.0 [512], decoder_lstm.1 [512]; 8 - 11 h, c of the bottleneck's layer 0
 * and 1 [64][bn_hidden] (-1: no such layer); 12 the mel norm's sum (double), 13 the unit norm's sums [64] doubles, 14 the
 * open block's partial sum [64][W], 15 the held output [64], 16 the step count (int), 17 in_tail [256], 18 ola_tail [256],
 * 19 / 20 ring_re / ring_im [look_ahead + 1][FP]; 21 the record's size; 22 F, 23 FP, 24 look_ahead + 1, 25 bn_hidden, 26
 * bn_layers, 27 W.  -1 on bad arguments.  Additive entries (no new FSN_ABI_VERSION). */
size_t fsn_fast_stream_pool_state_bytes(const fsn_fast_cfg* cfg, int look_ahead, int capacity);
size_t fsn_fast_stream_pool_workspace_bytes(const fsn_fast_cfg* cfg, int n, int k);
int fsn_fast_stream_pool_reset(const fsn_fast_cfg* cfg, int look_ahead, void* state, size_t state_bytes, int capacity,
                               const int* slots, int n, void* stream);
int fsn_fast_stream_pool_step(const fsn_fast_cfg* cfg, int look_ahead, const void* packed, void* state, size_t state_bytes,
                              int capacity, const int* slots, int n, int n_long, const float* mag, int k, float* crm_out,
                              void* workspace, size_t workspace_bytes, void* stream);
int fsn_fast_stream_pool_analysis(const fsn_fast_cfg* cfg, int look_ahead, void* state, size_t state_bytes, int capacity,
                                  const int* slots, int n, const float* hops, const float* prime, const int* frame_no,
                                  int n_fft, int hop, const float* window, float* mag, void* stream);
int fsn_fast_stream_pool_synthesis(const fsn_fast_cfg* cfg, int look_ahead, void* state, size_t state_bytes, int capacity,
                                   const int* slots, int n, const float* crm, int k, const int* first_frame,
                                   const int* tail_samples, int n_fft, int hop, const float* window, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream);
int fsn_debug_fast_stream_pool_layout(const fsn_fast_cfg* cfg, int look_ahead, long* out, int n);

/* ---- Improved FullSubNet, streaming: the model on k more frames with carried state -----------------------------------
 * fsn_fullsubnet_stream_step's contract for recipes/dns_interspeech_2020/improved_fullsubnet/model.py:541-591 with the
 * cumulative norm in front of the full-band model AND in front of every band section (the reference hands its sections
 * the offline norm whatever norm_type says; DESIGN "Improved FullSubNet as a stream" derives the causal counterpart: the
 * section input [B, N, 1, W, T] normalised as cumulative_laplace_norm of [B, 1, N W, T], eps = fp32 epsilon).  The model
 * has no look-ahead.  mag [B][F][k] are the next k frames of |STFT|, steps_done the number of frames passed in before
 * this call, mask [B][2][F][k] the mask of exactly these frames: the sections' outputs in bin order, the last bin an
 * exact zero; the caller multiplies real and imaginary parts by mask[:, 0] and mask[:, 1] (model.py:575-577: no
 * decompression, no complex product).
 * `state` (fsn_improved_stream_state_bytes, zero-filled for a new stream) carries (h, c) of the two full-band layers
 * [rows = B padded to 16][fb_hidden], (h, c) of both layers of every section [B units_i padded to 16][sb_hidden], the fp64
 * running sum of the full-band norm [B], one fp64 running sum per section and stream [sections][B], and the step count
 * [B] (written by every call as steps_done + k; the argument, kept by the caller, is what the divisors are taken from).
 * Any chunking of the same frames gives the same mask and the same final state bit for bit.
 * Configuration: F bins of the transform (the model runs on F - 1 <= 4096 of them), fdrc 0.5 or 1, 2 .. 8 sections that
 * tile [0, F - 1) in order, each with its centre and neighbour counts for the noisy and for the fb window (the two unit
 * counts (upper - lower) / centre must be whole and equal; a window sb_center + 2 sb_neighbors + fb_center + 2
 * fb_neighbors of at most 240 padded columns), hidden sizes that are multiples of 64 (pad with zero weights), cell 0
 * (LSTM; 1, GRU, is refused), output activations 0 (none) or 1 (ReLU).  Anything else: FSN_ERR_ARG with fsn_last_error
 * text; the size queries (which need no device) return 0, as they do for B or k outside 1 .. 4096.  A state or workspace
 * buffer that is too small: FSN_ERR_WORKSPACE, nothing launched.
 * Weights: fsn_improved_stream_pack copies them once into MFMA-fragment order (fsn_improved_stream_packed_bytes).  A block
 * of fsn_improved_params is the ten tensors w_ih_l0 [4H][I], w_hh_l0 [4H][H], b_ih_l0, b_hh_l0, w_ih_l1 [4H][H], w_hh_l1,
 * b_ih_l1, b_hh_l1, fc_w [O][H], fc_b [O] with H the (padded) hidden size: fb I = O = F - 1; section i I = its window,
 * O = 2 sb_center.
 * fsn_debug_improved_stream_state_layout (test hook, no device): out[0..50) (n >= 50): byte offsets of 0 - 3 the full-band
 * h0, c0, h1, c1; 4 + 4 i + (0 .. 3) the same of section i (-1: no such section); 36 the full-band sums, 37 the sections'
 * sums, 38 the step counts (longs); 39 the full-band row count, 40 + i section i's row count (-1: none), 48 the number of
 * sections, 49 the size fsn_improved_stream_state_bytes returns.  -1 on bad arguments.
 * Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name). */
#define FSN_IMPROVED_MAX_SECTIONS 8
typedef struct fsn_improved_section {
    int lower;         /* first bin of the band */
    int upper;         /* one past its last bin */
    int sb_center;     /* sb_num_center_freqs[i]: bins a unit predicts */
    int sb_neighbors;  /* sb_num_neighbor_freqs[i] */
    int fb_center;     /* fb_num_center_freqs[i] */
    int fb_neighbors;  /* fb_num_neighbor_freqs[i] */
} fsn_improved_section;
typedef struct fsn_improved_cfg {
    int F;              /* STFT bins, 481 at 48 kHz */
    float fdrc;         /* 0.5 or 1 */
    int num_sections;   /* 2 .. 8 */
    int fb_hidden;      /* padded to a multiple of 64 */
    int sb_hidden;
    int cell;           /* 0 LSTM */
    int fb_activation;  /* 0 none, 1 ReLU */
    int sb_activation;
    fsn_improved_section sec[FSN_IMPROVED_MAX_SECTIONS];
} fsn_improved_cfg;
typedef struct fsn_improved_params {
    const float* fb[10];
    const float* sb[FSN_IMPROVED_MAX_SECTIONS][10];
} fsn_improved_params;
size_t fsn_improved_stream_packed_bytes(const fsn_improved_cfg* cfg);
int fsn_improved_stream_pack(const fsn_improved_cfg* cfg, const fsn_improved_params* w, void* packed, size_t packed_bytes,
                             void* stream);
size_t fsn_improved_stream_state_bytes(const fsn_improved_cfg* cfg, int B);
size_t fsn_improved_stream_workspace_bytes(const fsn_improved_cfg* cfg, int B, int k);
int fsn_improved_stream_step(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes, long steps_done,
                             const float* mag, int B, int k, float* mask, void* workspace, size_t workspace_bytes,
                             void* stream);
int fsn_debug_improved_stream_state_layout(const fsn_improved_cfg* cfg, int B, long* out, int n);
/* Test hook: how fsn_improved_stream_step runs the sections' blocks.  0 (the default, the faster one as measured): a chain
 * of stateful layer launches per section, odd sections on the stream record's auxiliary stream beside the even ones.  1:
 * one step launch per layer and frame over the row tiles of all sections, each tile on its own section's weights (taken
 * while every section has fewer than 64 row tiles; beyond that the call runs form 0).  Both give the same bits in mask and
 * state.  0 or 1 selects a form for the whole process, any other value changes nothing; returns the form in use. */
int fsn_debug_improved_stream_form(int form);

/* ---- Improved FullSubNet, recordings of any length: the model in segments under the offline norms ----------------------
 * The fsn_fast_segment_* contract for Improved FullSubNet with the reference's norms.  The one-call path keeps gate planes
 * of hidden-state width for every frame of the recording; here the model runs on k (1 .. 4096) frames at a time.  What
 * lives for the whole recording is the caller's: planes of F floats per frame (magnitude, mask) and, between passes 2 and
 * 3, the full-band model's output fb_out [T][B][F - 1], time-major and unpadded in B, of which a segment is the contiguous
 * slice [k][B][F - 1] at frame frames_done.  Everything of hidden-size width is inside `workspace`
 * (fsn_improved_stream_workspace_bytes(cfg, B, k), one size for all passes).
 *
 * offline_laplace_norm divides by ONE mean per utterance and the model applies it twice (model.py:124-150, 565-567 in front
 * of the full-band model; :402-440 in front of every band section, over the section's unfolded windows of the noisy
 * magnitude AND of the full-band output).  A recording therefore takes three passes over its segments, each pass in frame
 * order, one pass finished before the next begins:
 *   1. fsn_improved_segment_stats: fb_sum[b] += the sum of mag ** fdrc over the first F - 1 bins of this call's frames
 *      inside row b, frame by frame (fp64).
 *   2. fsn_improved_segment_fullband: (mag ** fdrc) / den through the full-band block from its carried (h, c) -> fb_out
 *      [k][B][F - 1].  fb_norm 0 (offline): den = float(fb_sum[b] / ((F - 1) total_frames[b])) + eps from the finished sum
 *      of pass 1, eps the fp32 epsilon.  fb_norm 1 (cumulative; what the reference does under norm_type =
 *      "cumulative_laplace_norm", whose sections stay offline): the running mean exactly as fsn_improved_stream_step forms
 *      it, fb_sum carried by this pass itself - pass 1 is not run.  Any other fb_norm: FSN_ERR_ARG.  Every section's sum
 *      over all units and all window columns - the noisy window and the fb_out window, mirrored at both ends of the
 *      spectrum - of the frames inside the row is added to sb_sum[i][b] (fp64), frame by frame.
 *   3. fsn_improved_segment_sections: every section's input divided by float(sb_sum[i][b] / (N_i W_i total_frames[b])) +
 *      eps, through the sections' blocks from their carried (h, c) (in whichever form fsn_debug_improved_stream_form
 *      selects) -> mask [B][2][F][k], the last bin an exact zero.
 * frames_done: frames passed to THIS pass before the call.  total_frames (device memory, [B]): row b's own frame count
 * T_b (values below 1 count as 1).  In a ragged batch every row runs to the longest row's end.  A frame at or past T_b adds
 * nothing to any sum, its magnitude is not read and counts as zero wherever it is an input; what the blocks produce there
 * is finite and to be ignored.
 * A frame's own sum has a fixed shape and the fp64 carries advance frame by frame: two segmentations of one recording give
 * the same fb_out, the same masks, the same divisors and the same state bit for bit.
 *
 * `state`: the blob of fsn_improved_stream_state_bytes(cfg, B) in fsn_improved_stream_step's layout
 * (fsn_debug_improved_stream_state_layout), caller-owned, all zeros for a fresh recording: pass 2 carries the full-band
 * block's (h, c) and writes the step count (frames_done + k), pass 3 carries the sections'; fb_sum and sb_sum hold the sums
 * above.  `packed`: fsn_improved_stream_pack's blob.  fsn_improved_segment_divisors writes den_fb [B] and den_sb
 * [sections][B] (device memory) as passes 2 (fb_norm 0) and 3 form them: call it after pass 1 for den_fb, after pass 2 for
 * den_sb.
 * FSN_ERR_ARG with fsn_last_error text: what fsn_improved_stream_step refuses of a configuration, B or k outside 1 ..
 * 4096, a negative frames_done, a NULL pointer.  FSN_ERR_WORKSPACE for a short state or workspace buffer, before anything is
 * launched.  Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name). */
int fsn_improved_segment_stats(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, long frames_done,
                               const int* total_frames, const float* mag, int B, int k, void* stream);
int fsn_improved_segment_fullband(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes, int fb_norm,
                                  long frames_done, const int* total_frames, const float* mag, int B, int k, float* fb_out,
                                  void* workspace, size_t workspace_bytes, void* stream);
int fsn_improved_segment_sections(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                  long frames_done, const int* total_frames, const float* mag, const float* fb_out, int B, int k,
                                  float* mask, void* workspace, size_t workspace_bytes, void* stream);
int fsn_improved_segment_divisors(const fsn_improved_cfg* cfg, const void* state, size_t state_bytes, const int* total_frames,
                                  int B, float* den_fb, float* den_sb, void* stream);

/* ---- Improved FullSubNet, streaming pool: 48 kHz sessions share one step ------------------------------------------------
 * fsn_improved_stream_step for streams that are NOT in lockstep, as fsn_fast_stream_pool_step is for Fast FullSubNet.
 * `state` is a pool of `capacity` slots (1 .. 4096), fsn_improved_stream_pool_state_bytes(cfg, capacity) bytes = capacity
 * equal records, slot s at byte s * (state_bytes / capacity), each 256-byte aligned.  A record holds what ONE stream of
 * fsn_improved_stream_step carries at B = 1, without row padding ((h, c) of both full-band layers [fb_hidden], (h, c) of both
 * layers of section i [units_i][sb_hidden], the full-band norm's fp64 sum, one fp64 sum per section), the slot's own step
 * count (a long on the device: the kernels read and advance it) and the transform state of the two transform entries, sized
 * for hop = F - 1: the last hop [hop], the overlap-add half frame [hop], the spectrum (re, im [F]) of the ONE frame that
 * waits for its mask - the model has no look-ahead - and that frame's number.  All zeros is a fresh pool;
 * fsn_improved_stream_pool_reset returns the n listed slots to that state (stream-ordered).
 *
 * fsn_improved_stream_pool_step advances the n listed slots (`slots`: device memory, n DISTINCT ids, 1 <= n <= capacity) by
 * k (1 .. 4096) model steps, each from its own step count: row i of mag [n, 1, F, k] and mask_out [n, 2, F, k] belongs to
 * slots[i] and is what fsn_improved_stream_step gives a batch of one with the same history (to the rounding of the recurrent
 * kernels, which are chosen by the call's row count; the same calls on a fresh pool give the same bits, and so do two
 * chunkings of a slot's frames in calls of the same n).  The last bin is an exact zero.  Rows go in any order.  The call
 * gathers the listed records into a state of fsn_improved_stream_step's layout at B = n inside the workspace (pad rows and
 * skipped rows zeros), runs that entry's sequence with every row's divisors taken from its own count and fp64 carry, and
 * scatters (h, c), the sums and the counts + k back: its last kernel.  Slots that are not listed are not written.  A row
 * whose id is outside [0, capacity) is skipped (its mask_out row is finite - its mag row is not read -, no state is touched);
 * listing an id twice is the caller's error.  FSN_ERR_ARG with fsn_last_error text: what fsn_improved_stream_step refuses
 * (configuration; n, k outside 1 .. 4096), capacity outside 1 .. 4096, n outside 1 .. capacity; the size queries need no
 * device and return 0 then.  A state or workspace buffer that is too small: FSN_ERR_WORKSPACE, nothing launched.
 *
 * The transform around that step, one frame per listed slot and call: any even n_fft <= 4096 with hop = n_fft / 2 = F - 1 and
 * a window of n_fft taps (960 / 480 at 48 kHz); anything else is FSN_ERR_ARG.  All int arrays are device memory, [n]; ids
 * outside the pool are skipped (zeros out, no state touched).
 * fsn_improved_stream_pool_analysis: fsn_stream_pool_analysis's contract.  frame = the slot's last hop ++ hops[i] (hops
 * [n][hop]), windowed in fp32, its real DFT taken in fp64 from an exact twiddle table (fsn_stft's arithmetic at this size:
 * two-level where n_fft splits, direct where not) and rounded once to fp32.  The spectrum and frame_no[i] (>= 0; a negative
 * one skips the row) go to the record, the magnitude to mag [n, 1, F, 1], hops[i] becomes the slot's last hop.  Frame 0
 * reads its left half backwards from prime[i] = y[1 .. hop] (prime [n][hop]; NULL only when no listed session is at frame 0:
 * a frame 0 then takes the slot's carried hop, zeros on a fresh slot).
 * fsn_improved_stream_pool_synthesis: mask [n, 2, F, 1] is the model's mask of the frame in the record.  The enhanced
 * spectrum is mask[:, 0] re, mask[:, 1] im (model.py:575-577: no decompression, no complex product); then the inverse
 * transform, the window and the overlap-add with the record's half frame, divided by the overlap-added squared window as
 * fsn_istft / torch.istft do.  THE FRAME NUMBER m IS THE RECORD'S: the one the analysis call stored with the spectrum.  Frame
 * m >= 1 gives the hop samples [(m - 1) hop, m hop) at out[i][0 .. hop); frame 0 gives none.  tail_samples[i] >= 0 marks
 * the session's last frame: the samples [(T - 1) hop, L), tail_samples[i] <= hop of them, follow at out[i][hop ..] (pass -1
 * otherwise).  out [n][2 hop] is written completely (zeros where there is no sample).
 *
 * fsn_debug_improved_stream_pool_layout (test hook, no device): out[0..58) (n >= 58): byte offsets into a record of 0 - 3 the
 * full-band h0, c0, h1, c1; 4 + 4 i + (0 .. 3) the same of section i (-1: no such section); 36 the full-band sum (double),
 * 37 the sections' sums [8] doubles, 38 the step count (long), 39 the last hop [hop], 40 the overlap-add half frame [hop],
 * 41 / 42 the waiting spectrum's re / im [F], 43 its frame number (int); 44 the record's size; 45 F, 46 hop, 47 fb_hidden,
 * 48 sb_hidden, 49 the number of sections, 50 + i section i's units (-1: none).  -1 on bad arguments.
 * Additive entries (no new FSN_ABI_VERSION; a binding looks them up by name). */
size_t fsn_improved_stream_pool_state_bytes(const fsn_improved_cfg* cfg, int capacity);
size_t fsn_improved_stream_pool_workspace_bytes(const fsn_improved_cfg* cfg, int n, int k);
int fsn_improved_stream_pool_reset(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, int capacity, const int* slots,
                                   int n, void* stream);
int fsn_improved_stream_pool_step(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes, int capacity,
                                  const int* slots, int n, const float* mag, int k, float* mask_out, void* workspace,
                                  size_t workspace_bytes, void* stream);
int fsn_improved_stream_pool_analysis(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                      const int* slots, int n, const float* hops, const float* prime, const int* frame_no,
                                      int n_fft, int hop, const float* window, float* mag, void* stream);
int fsn_improved_stream_pool_synthesis(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                       const int* slots, int n, const float* mask, const int* tail_samples, int n_fft, int hop,
                                       const float* window, float* out, void* stream);
int fsn_debug_improved_stream_pool_layout(const fsn_improved_cfg* cfg, long* out, int n);

int fsn_profile_num_stages(void);
const char* fsn_profile_stage_name(int stage);
int fsn_profile_read(void* stream, float* ms_per_stage, int n);

#ifdef __cplusplus
}
#endif
#endif /* FSN_HIP_H */
