// Shared device/host helpers for libfsn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

#include "../../include/fsn_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define FSN_WAVE 64

static inline int fsn_round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline size_t fsn_round_up_sz(size_t x, size_t m) { return (x + m - 1) / m * m; }

// frequency axis padded to a multiple of 16 floats: rows stay 16-byte aligned for float4 operand
// loads and the zero padding doubles as the K padding of the full-band input projection.
static inline int fsn_fpad(int F) { return fsn_round_up(F, 16); }

void fsn_set_error(const char* fmt, ...);

// Ragged batches (fsn_enhance_ragged, 512 / 256 transform): row b of a [B][L] signal holds lengths[b] samples, the rest
// of the row is padding.  A value outside [n_fft / 2 + 1, L] is clamped into it, so that no length can index outside the
// row; lengths == NULL: every row is L samples long.  The row's frames: 1 + L_b / hop, never more than T = 1 + L / hop.
__device__ __forceinline__ int fsn_row_samples(const int* lengths, int b, int L) {
    if (!lengths) return L;
    const int l = lengths[b];
    return l < 257 ? 257 : (l > L ? L : l);
}
__device__ __forceinline__ int fsn_row_frames(const int* lengths, int b, int T) {
    if (!lengths) return T;
    const int l = lengths[b];
    const int t = 1 + (l < 257 ? 257 : l) / 256;
    return t < T ? t : T;
}

// Opened by every entry point that enqueues work (fsn_api.hip): makes the device of the caller's stream the
// current one for the duration of the call and selects the per-(device, stream) record of the library.
struct FsnCallScope {
    int prev;
    bool switched;
    explicit FsnCallScope(void* stream);
    ~FsnCallScope();
};
int fsn_check_launch(const char* what);

// Launch trace (test hook, fsn_debug_core_last_launches): one 32-bit mask per host thread, cleared by FsnCallScope at
// entry; every launcher the model core can reach, and the core's three sub-band GEMM sites, OR their bit in.
enum FsnTraceBit : unsigned {
    FSN_TR_LSTM_REC = 1u << 0,
    FSN_TR_LSTM_REC_IN = 1u << 1,
    FSN_TR_LSTM_REC_X = 1u << 2,
    FSN_TR_LSTM_STEP = 1u << 3,
    FSN_TR_LSTM_STEP_CU = 1u << 4,
    FSN_TR_LSTM_WAVEFRONT2 = 1u << 5,
    FSN_TR_LSTM2_GROUP = 1u << 6,
    FSN_TR_FB_CHAIN = 1u << 7,
    FSN_TR_GEMM_SB_PROJ = 1u << 8,  // layer-0 projection of rows that run step by step (core_sb_projection)
    FSN_TR_GEMM_SB_L1 = 1u << 9,    // layer-1 projection GEMM (whole, or of the left-over rows under lstm_rec_x)
    FSN_TR_GEMM_SB_OUT = 1u << 10,  // output layer as a GEMM (core_sb_output)
};
void fsn_trace(unsigned bit);  // fsn_api.hip

// Raise `kernel`'s dynamic-LDS limit to at least `bytes` on the current device, before a launch that asks for more than
// the 64 KB every kernel may have.  Called at every such launch; the runtime is asked once per (device, kernel) and size
// that grows - the limit belongs to that pair, so the record is keyed by it, and it is kept under a mutex (the per-launcher
// `static bool` flags this replaces skipped a process's second device and raced between threads; with no record at all
// the training figures were not reliably inside the parent's range: profiles/gemm_tn_split.md).
// fsn_request_lds: false on failure, nothing refused and nothing recorded - for the launches the runtime was measured to
// accept anyway; fsn_reserve_lds: the launcher's return value, the failure on record as "<what>: cannot reserve ..".
inline bool fsn_request_lds_of(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> raised;  // (device, kernel) -> the limit it has been given
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = raised[{dev, kernel}];
    if (have >= bytes) return true;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    have = bytes;
    return true;
}
template <class Kernel>
inline bool fsn_request_lds(Kernel kernel, size_t bytes) {
    return fsn_request_lds_of(reinterpret_cast<const void*>(kernel), bytes);
}
template <class Kernel>
inline int fsn_reserve_lds(const char* what, Kernel kernel, size_t bytes) {
    if (fsn_request_lds(kernel, bytes)) return FSN_OK;
    fsn_set_error("%s: cannot reserve %zu bytes of LDS", what, bytes);
    return FSN_ERR_LAUNCH;
}
#define FSN_TRY_RESERVE_LDS(what, kernel, bytes)                   \
    do {                                                           \
        const int _rc = fsn_reserve_lds(what, kernel, bytes);      \
        if (_rc != FSN_OK) return _rc;                             \
    } while (0)

#define FSN_TRY_LAUNCH(what)                        \
    do {                                            \
        const int _rc = fsn_check_launch(what);     \
        if (_rc != FSN_OK) return _rc;              \
    } while (0)

#define FSN_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            fsn_set_error(__VA_ARGS__); \
            return FSN_ERR_ARG;         \
        }                               \
    } while (0)

// D = A(16x4) * B(4x16) + C, exact fp32 (k-ordered fmaf chain).  Lane l supplies A[l&15][l>>4]
// and B[l>>4][l&15]; D/C: col = l&15, row = 4*(l>>4) + reg.
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// One K = 16 block of a product, D = A(16 x 16) B(16 x 16) + C, from the fp32 fragments every kernel of this library
// moves (lane (i, q) holds A[i][4q .. 4q+3] / B[4q .. 4q+3][i]), in the arithmetic AR of the call:
//   FSN_ARITH_F32   four v_mfma_f32_16x16x4_f32: exact fp32 products, the arithmetic of every parity claim;
//   FSN_ARITH_F16   both operands rounded to fp16 (round to nearest even) AT THE MATRIX CORE'S INPUT, one
//   FSN_ARITH_BF16  v_mfma_f32_16x16x16_{f16,bf16}, fp32 accumulation - what torch.autocast does to nn.LSTM / nn.Linear
//                   (recipes/dns_interspeech_2020/fullsubnet/trainer.py:56), an eighth of the matrix-core time.
// Everything around the product (storage, cell update, reductions) is fp32 in every mode.
typedef _Float16 fsn_f16x4 __attribute__((ext_vector_type(4)));
typedef short fsn_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned fsn_u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 fsn_bf16x2 __attribute__((ext_vector_type(2)));
template <int AR>
struct FsnOperand {
    typedef f32x4 type;
};
template <>
struct FsnOperand<FSN_ARITH_F16> {
    typedef fsn_f16x4 type;
};
template <>
struct FsnOperand<FSN_ARITH_BF16> {
    typedef fsn_s16x4 type;
};
// A weight fragment as it travels L2 -> registers -> LDS under arithmetic AR: fp32 (16 bytes per lane), or - 16-bit
// arithmetic - the 16-bit copy of the packed weights (8 bytes per lane: half the L2 traffic and half the LDS of a K
// loop whose matrix work is an eighth); fragment ORDER is the same, so element offsets carry over.
template <int AR>
struct FsnWFrag {
    typedef f32x4 type;
};
template <>
struct FsnWFrag<FSN_ARITH_F16> {
    typedef fsn_u32x2 type;
};
template <>
struct FsnWFrag<FSN_ARITH_BF16> {
    typedef fsn_u32x2 type;
};
template <int AR>
__device__ __forceinline__ typename FsnOperand<AR>::type fsn_wfrag_operand(const typename FsnWFrag<AR>::type w) {
    if constexpr (AR == FSN_ARITH_F32) return w;
    else return __builtin_bit_cast(typename FsnOperand<AR>::type, w);
}
template <int AR>
__device__ __forceinline__ typename FsnOperand<AR>::type fsn_operand(const f32x4 v) {
    if constexpr (AR == FSN_ARITH_F16) {
        return __builtin_convertvector(v, fsn_f16x4);  // v_cvt_pk_f16_f32 x 2
    } else if constexpr (AR == FSN_ARITH_BF16) {
        // pairs through __builtin_convertvector: one v_cvt_pk_bf16_f32 each (round to nearest even), and - unlike the
        // same instruction from inline asm, which produced NaNs here - the compiler knows it is a VALU write feeding a
        // matrix instruction and inserts the wait state that hazard needs
        const fsn_bf16x2 lo = __builtin_convertvector(f32x2{v[0], v[1]}, fsn_bf16x2);
        const fsn_bf16x2 hi = __builtin_convertvector(f32x2{v[2], v[3]}, fsn_bf16x2);
        const fsn_u32x2 r = {__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)};
        return __builtin_bit_cast(fsn_s16x4, r);
    } else {
        return v;
    }
}
template <int AR>
__device__ __forceinline__ f32x4 fsn_mma_k16(const typename FsnOperand<AR>::type a, const typename FsnOperand<AR>::type b,
                                             f32x4 c) {
    if constexpr (AR == FSN_ARITH_F16) {
        return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
    } else if constexpr (AR == FSN_ARITH_BF16) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) c = mfma16(a[j], b[j], c);
        return c;
    }
}

// Two K = 16 blocks of the same product at once, as ONE K = 32 instruction of gfx950 (v_mfma_f32_16x16x32_{f16,bf16}: the
// K = 16 shapes issue at half its rate there).  The matrix instruction sums a_lane(i, q)[j] b_lane(n, q)[j] over the four
// lane groups q and the lane's elements j: as long as A and B give the same k to the same (q, j), ANY assignment of k to
// (q, j) is the same contraction - so the eight values of a lane are simply block 0's four followed by block 1's, and the
// result is fsn_mma_k16(a0, b0, fsn_mma_k16(a1, b1, c)) up to the order of the fp32 sums inside the instruction.
typedef _Float16 fsn_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 fsn_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned fsn_u32x4 __attribute__((ext_vector_type(4)));
template <int AR>
__device__ __forceinline__ f32x4 fsn_mma_k32(const typename FsnOperand<AR>::type a0, const typename FsnOperand<AR>::type a1,
                                             const typename FsnOperand<AR>::type b0, const typename FsnOperand<AR>::type b1,
                                             f32x4 c) {
    if constexpr (AR == FSN_ARITH_F16) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7),
                                                      __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7), c, 0, 0, 0);
    } else if constexpr (AR == FSN_ARITH_BF16) {
        const fsn_u32x2 pa0 = __builtin_bit_cast(fsn_u32x2, a0), pa1 = __builtin_bit_cast(fsn_u32x2, a1);
        const fsn_u32x2 pb0 = __builtin_bit_cast(fsn_u32x2, b0), pb1 = __builtin_bit_cast(fsn_u32x2, b1);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(fsn_bf16x8, fsn_u32x4{pa0[0], pa0[1], pa1[0], pa1[1]}),
            __builtin_bit_cast(fsn_bf16x8, fsn_u32x4{pb0[0], pb0[1], pb1[0], pb1[1]}), c, 0, 0, 0);
    } else {
        return fsn_mma_k16<AR>(a1, b1, fsn_mma_k16<AR>(a0, b0, c));
    }
}

// gfx950 store-data hazard (measured: tools/probe_store_hazard.hip, profiles/r06_store_hazard.md).  A 12 / 16-byte-per-lane
// store reads its data registers lane quad by lane quad over the cycles after issue; a vector instruction that writes them
// again 1 - 2 issue slots later (global stores, buffer stores with an immediate soffset) or 1 slot later (buffer stores with
// an SGPR soffset) reaches memory in lanes 8 - 15 / 12 - 15 of every 16.  hipcc (ROCm 7.2) keeps two wait states in the
// first case and none in the second (its hazard recogniser exempts a register soffset): lstm2_g16_bwd_kernel's layer-0 gate
// gradients were 6e-2 off in round 5 behind `buffer_store_dwordx4 v[38:41], .., s0 offen ; v_pk_add_f32 v[38:39], ..`.
// Call this right behind such a store when the value is re-used as an accumulator: the data registers stay allocated and
// untouched for two more issue slots (the distance that was never wrong is 3).  tests/test_host_cpu.py scans EVERY kernel
// of the shipped library for vector writes inside the unsafe distance (tools/check_store_hazard.py).
// FSN_HOLD_MODE (diagnosis builds only, tools/build_variant.py): 1 = nothing (the failing build), 2 = kept allocated, no wait.
#ifndef FSN_HOLD_MODE
#define FSN_HOLD_MODE 0
#endif
__device__ __forceinline__ void fsn_hold_store_data(const f32x4& v) {
#if FSN_HOLD_MODE == 0
    asm volatile("s_nop 1" ::"v"(v) : "memory");
#elif FSN_HOLD_MODE == 2
    asm volatile("" ::"v"(v) : "memory");
#endif
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

// Gate non-linearities of every LSTM forward kernel (persistent, per-step, wavefront) on the hardware transcendentals
// (v_exp_f32 / v_rcp_f32, ~1 ULP each): 4-5 VALU instructions per value instead of ~30 for the
// libm-accurate forms.  Absolute error <= ~2e-7, the size of one fp32 rounding of the gate
// pre-activation itself; the end-to-end effect on the compressed mask is measured by the parity
// tests (tests/test_gpu_parity.py).  -DFSN_ACCURATE_ACT=1 switches back to expf / tanhf.
#ifndef FSN_ACCURATE_ACT
#define FSN_ACCURATE_ACT 0
#endif
__device__ __forceinline__ float sigmoid_fast(float x) {
#if FSN_ACCURATE_ACT
    return sigmoid_f(x);
#else
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
#endif
}
__device__ __forceinline__ float tanh_fast(float x) {
#if FSN_ACCURATE_ACT
    return tanhf(x);
#else
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(2.8853900817779268f * x));
#endif
}

// Bijective XCD-aware block remap: block b runs on XCD b % 8 (observed, speed only); give each
// XCD a contiguous chunk of the virtual grid so neighbouring tiles share that XCD's L2.
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
    const unsigned q = nblk >> 3, r = nblk & 7u;
    const unsigned xcd = bid & 7u, slot = bid >> 3;
    const unsigned base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + slot;
}

// CU count of the current device for the plans; 256 if the query fails or returns < 1.
inline int plan_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus < 1 ? 256 : cus;
}

// ---- kernels' host launchers (one per translation unit) -------------------------------------
struct FsnStream {
    hipStream_t s;
};

// fft_kernels.hip.  lengths (device, [B], may be NULL): per-row sample counts of a ragged batch (fsn_row_samples); L /
// length is then the row stride and the longest row, T its frame count.
int fsn_launch_stft(const float* y, int B, int L, const float* window, float* re, float* im, float* mag,
                    int T, int Tp, int F, int FP, bool frame_major, hipStream_t s, const int* lengths = nullptr);
// crm_batch_stride: the reference layout's batch stride of crm_r / crm_i (0: F T, separate [B][F][T] planes)
int fsn_launch_mask_irfft(const float* re, const float* im, const float* crm_r, const float* crm_i,
                          int B, int T, int F, int FP, bool frame_major, const float* window,
                          float* wframes, hipStream_t s, const int* lengths = nullptr, long crm_batch_stride = 0);
int fsn_launch_ola(const float* wframes, const float* window, int B, int T, int length, float* y,
                   hipStream_t s, const int* lengths = nullptr);

// ---- streaming pool (fsn_fullsubnet_stream_pool_*) --------------------------------------------------------------------
// The pool's state blob is `capacity` records of slot_bytes each, one per slot; all zeros is a fresh slot.  Byte offsets
// into a record (every array 256-byte aligned, slot_bytes a multiple of 256):
//   fb[a] / sb[a]   a = h0, h1, c0, c1 of the full-band model [Hf] / of the sub-band model [F][Hs]
//   fb_sum, sb_sum  running fp64 sums of the two cumulative norms (1 and F doubles)
//   steps           model steps this slot has taken (int; read and advanced on the device)
//   in_tail         the last 256 input samples (left half of the next analysis frame)
//   ola_tail        second half of the last synthesised frame (overlap-add partner of the next one)
//   ring_re/_im     spectra of the last R = look_ahead + 1 analysed frames, [R][FP], frame t at t % R
struct FsnPoolLayout {
    size_t fb[4], sb[4], fb_sum, sb_sum, steps, in_tail, ola_tail, ring_re, ring_im, slot_bytes;
    int F, FP, Hf, Hs, R;
};
static inline FsnPoolLayout fsn_pool_layout(int F, int Hf, int Hs, int look_ahead) {
    FsnPoolLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t r = o;
        o = fsn_round_up_sz(o + bytes, 256);
        return r;
    };
    L.F = F;
    L.FP = fsn_fpad(F);
    L.Hf = Hf;
    L.Hs = Hs;
    L.R = look_ahead + 1;
    for (int a = 0; a < 4; ++a) L.fb[a] = take((size_t)Hf * sizeof(float));
    for (int a = 0; a < 4; ++a) L.sb[a] = take((size_t)F * Hs * sizeof(float));
    L.fb_sum = take(sizeof(double));
    L.sb_sum = take((size_t)F * sizeof(double));
    L.steps = take(sizeof(int));
    L.in_tail = take(256 * sizeof(float));
    L.ola_tail = take(256 * sizeof(float));
    L.ring_re = take((size_t)L.R * L.FP * sizeof(float));
    L.ring_im = take((size_t)L.R * L.FP * sizeof(float));
    L.slot_bytes = o;
    return L;
}
// the record of slots[i], or NULL for i >= n or an id outside the pool (such a row is skipped by every pool kernel)
__device__ __forceinline__ char* fsn_pool_record(char* state, const FsnPoolLayout& L, int capacity, const int* slots, int n,
                                                 int i) {
    if (i >= n) return nullptr;
    const int slot = slots[i];
    return (slot >= 0 && slot < capacity) ? state + (size_t)slot * L.slot_bytes : nullptr;
}

// Shared by the cumulative-norm kernels of elementwise_kernels.hip and their per-slot forms in stream_pool_kernels.hip
// (the pool's bit-identity to the lockstep entry rests on both using exactly this arithmetic).
constexpr float kFsnEpsilon = 1.1920928955078125e-07f;  // audio_zen/constant.py:9
// reflect(j) of F.pad(mode="reflect") for j in [-N, F+N)
__device__ __forceinline__ int fsn_reflect_idx(int j, int F) {
    j = j < 0 ? -j : j;
    return j >= F ? 2 * (F - 1) - j : j;
}
// sum of v over the workgroup (whole waves, at most 16), every thread gets it; fixed order
__device__ __forceinline__ double fsn_block_sum(double v, double* scratch) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) tot += scratch[w];
    return tot;
}

// stream_pool_kernels.hip.  slots: device, n ids; a row whose id is outside [0, capacity) is skipped by every kernel.
// which: 0 full-band model (Npad = round_up(n, 16) rows), 1 sub-band model (Npad = round_up(n F, 16) rows, row i F + f).
int fsn_launch_pool_gather(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, int which, float* h0,
                           float* h1, float* c0, float* c1, int Npad, hipStream_t s);
// which == 1 also advances the listed slots' step counts by k: it is the last launch of a step
int fsn_launch_pool_scatter(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, int which, float* h0,
                            float* h1, float* c0, float* c1, int Npad, int k, hipStream_t s);
// mag / fb_out [n][k][FP]; den [n][k] (full band) and [k][Npad] (sub band), as fsn_launch_cumulative_den_*
int fsn_launch_pool_den_fb(const float* mag, float* den, void* state, const FsnPoolLayout& L, int capacity, const int* slots,
                           int n, int k, hipStream_t s);
int fsn_launch_pool_den_sb(const float* mag, const float* fb_out, float* den, void* state, const FsnPoolLayout& L,
                           int capacity, const int* slots, int n, int k, int nb, int Npad, hipStream_t s);
int fsn_launch_pool_reset(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, hipStream_t s);
// fft_kernels.hip: one analysis frame per listed slot / k synthesis frames per listed slot (see the kernels)
int fsn_launch_pool_analysis(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, const float* hops,
                             const float* prime, const int* frame_no, const float* window, float* mag, hipStream_t s);
int fsn_launch_pool_synthesis(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, const float* crm,
                              int k, const int* first_frame, const int* tail_samples, const float* window, float* wframes,
                              float* out, hipStream_t s);

// mix_kernels.hip (fsn_conv_rows / fsn_mix_pairs).  Z: B rows of 2^logN fp64 complex points, or NULL when the workspace
// holds no transform (rows with a response then come back as NaN, the others are copied); live: B ints of scratch
// h_off / h_len: row b's offset (long) and length (int) at byte b * stride of each (arrays, or fields of the item table)
int fsn_launch_conv_rows(const float* x, int B, int L, const void* h_slab, int fmt, const void* h_off, int off_stride,
                         const void* h_len, int len_stride, float* y, void* Z, int* live, int logN, hipStream_t s);
int fsn_launch_mix_gather(const void* clean_slab, const void* noise_slab, int fmt, const fsn_mix_item* items,
                          const fsn_mix_seg* segs, int n_segs, int B, int L, float* c0, float* nz, hipStream_t s);
int fsn_launch_mix_level(const float* c, const float* nz, const fsn_mix_item* items, int B, int L, float eps, float* noisy,
                         float* clean, hipStream_t s);
// fsn_rir_shorten / fsn_mix_pairs_target.  One workgroup per response: out (and win, idx when not NULL) as the header
// states them; t_off / t_len (both or neither): row b's place in `out` (b ld) and the taps a convolution with it takes
// (min(h_len, ld), 0 for a row whose target is its reverberant row: no response, or mode 0) - the Taps of the second
// convolution.  h_off / h_len with strides as in fsn_launch_conv_rows.
int fsn_launch_rir_shorten(const void* h_slab, int fmt, const void* h_off, int off_stride, const void* h_len, int len_stride,
                           int B, const fsn_mix_target* targets, float* out, int ld, float* win, int* idx, long* t_off,
                           int* t_len, hipStream_t s);
// the level kernel's three-row form: target = (t_len[b] > 0 ? c2 : c) under the clean row's scalars; clean may be NULL
int fsn_launch_mix_level_target(const float* c, const float* nz, const float* c2, const int* t_len, const fsn_mix_item* items,
                                int B, int L, float eps, float* noisy, float* clean, float* target, hipStream_t s);

// stoi_kernels.hip (fsn_stoi / fsn_si_sdr).  The plan is host arithmetic on (B, L_max, sr) alone (fsn_api_metrics.hip);
// every per-row count follows on the device from the row's own length.
struct FsnStoiPlan {
    int B, L_max;
    int up, down, half;  // resampling ratio and half-length of its filter (2 half + 1 taps); half = 0: the rate is 10 kHz
    int n10_max;         // samples of the longest row at 10 kHz
    int nf_max;          // its 256-sample frames at hop 128 (the last full one not taken)
    int m_max;           // spectral frames when nothing is removed: nf_max - 1
    int j_blocks;        // workgroups of the correlation kernel per (row, band)
};
struct FsnStoiBuffers {
    double* taps;     // [2 half + 1]
    double* rs;       // [B][2][n10_max] clean, estimate at 10 kHz
    double* energy;   // [B][nf_max] frame energies of the clean row in dB
    int* kept;        // [B][nf_max] indices of the frames that stay, in order
    int* n_kept;      // [B]
    double* tob;      // [B][2][15][m_max] one-third-octave band magnitudes
    double* partial;  // [B][15][j_blocks] per-workgroup sums of the correlations
};
// a row's samples (lengths[b] clamped into [0, L_max]; NULL: L_max), its samples at 10 kHz (ceil(n up / down)) and its
// frames of 256 at hop 128 whose start is < n10 - 256 (the last full frame is not taken)
__device__ __forceinline__ int fsn_stoi_row_samples(const int* lengths, int b, int L_max) {
    if (!lengths) return L_max;
    const int l = lengths[b];
    return l < 0 ? 0 : (l > L_max ? L_max : l);
}
__host__ __device__ inline int fsn_stoi_n10(int n, int up, int down, int half) {
    return half ? (int)(((long)n * up + down - 1) / down) : n;
}
__host__ __device__ inline int fsn_stoi_frames(int n10) { return n10 > 256 ? (n10 - 256 + 127) / 128 : 0; }
int fsn_launch_stoi(const float* clean, const float* estimate, const int* lengths, const FsnStoiPlan& p,
                    const FsnStoiBuffers& w, double* d, hipStream_t s);
int fsn_launch_si_sdr(const float* reference, const float* estimate, const int* lengths, int B, int L_max, double* out_db,
                      hipStream_t s);

// resample_kernels.hip (fsn_resample / fsn_resample_taps).  The plan is host arithmetic on the rates and the design
// (fsn_api_resample.hip); a row's output length follows on the device from the row's own length.
constexpr int kFsnResampleThreads = 512;
constexpr int kFsnResampleOutPerThread = 8;       // outputs of one phase per thread: one tap load per eight multiply-adds
constexpr int kFsnResampleMaxStretch = 24576;     // input samples a workgroup stages (fp32: 96 KB)
constexpr size_t kFsnResampleLdsBytes = 160 * 1024;  // what a workgroup of gfx950 may hold
struct FsnResamplePlan {
    int u, d;         // sr_out / g, sr_in / g
    int H, taps;      // half length zeros * max(u, d), 2 H + 1
    int J, Js;        // taps of the longest phase ceil(taps / u); row stride of the polyphase table (J made odd)
    int S;            // outputs of one pass of a workgroup (its threads take them 512 at a time): a multiple of u, so that
                      // k and k + S share their phase
    int tile;         // outputs of a workgroup: kFsnResampleOutPerThread * S
    int stretch;      // input samples a workgroup stages at most: (tile - 1) d / u + J + 1
    int taps_in_lds;  // the whole polyphase table sits in LDS beside the stretch
    double beta, rolloff;
};
__host__ __device__ inline long fsn_resample_n_out(long n, int u, int d) { return (n * u + d - 1) / d; }
// h [taps]: the filter in natural order; poly [u][Js] (may be NULL): the same in polyphase order, zero-padded rows
int fsn_launch_resample_taps(const FsnResamplePlan& p, double* h, double* poly, hipStream_t s);
int fsn_launch_resample(const float* x, const int* lengths, int B, int L_max, const FsnResamplePlan& p, const double* poly,
                        float* y, int L_out_max, int* out_lengths, hipStream_t s);

// resample_stream_kernels.hip (fsn_resample_stream_*).  A tick of a serving pool is a few hundred outputs per session, so
// a workgroup takes `tile` consecutive outputs of one session, one per thread.
constexpr int kFsnResampleStreamThreads = 256;
constexpr int kFsnResampleStreamMaxStretch = 16384;  // input samples a workgroup stages (fp32: 64 KB)
struct FsnResampleStreamPlan {
    int u, d, H;      // as FsnResamplePlan; H = 0 for u == d == 1 (the chunks pass through)
    int J, Js;        // taps per phase (1 for u == d == 1); row stride of the polyphase table
    int tile;         // outputs of a workgroup: 256, halved until its stretch can be staged
    int stretch;      // input samples a workgroup stages at most: (tile - 1) d / u + J + 1
    int taps_in_lds;  // the table is staged: it fits beside the stretch and is no longer than the tile's tile * J reads
    int slot_floats;  // two history buffers of J - 1 samples, rounded up to 64 floats
};
int fsn_launch_resample_stream(const FsnResampleStreamPlan& p, const double* poly, float* slots, int capacity,
                               const fsn_resample_stream_item* items, int n, const float* x, int C_max, float* y, int O_max,
                               hipStream_t s);
int fsn_launch_resample_stream_reset(const FsnResampleStreamPlan& p, float* slots, int capacity, const int* ids, int n,
                                     hipStream_t s);

// dft_kernels.hip (any even n_fft / any hop: direct fp64 DFT; reference layout [B][F][T] only).  lengths (device, [B], may
// be NULL): per-row sample counts of a ragged batch; L / length is then the row stride and the longest row, T its frames
int fsn_launch_dft_stft(const float* y, int B, int L, const float* window, float* re, float* im, float* mag, int T,
                        int N, int hop, hipStream_t s, const int* lengths = nullptr);
int fsn_launch_dft_istft(const float* re, const float* im, const float* window, float* wframes, float* y, int B, int T,
                         int N, int hop, int length, hipStream_t s, const int* lengths = nullptr);

// elementwise_kernels.hip
int fsn_launch_decompress(const float* in, float* out, size_t n, hipStream_t s);
int fsn_launch_compress(const float* in, float* out, size_t n, hipStream_t s);
int fsn_launch_build_cirm(const float* nr, const float* ni, const float* cr, const float* ci, float* out,
                          size_t n, hipStream_t s);
// lengths (may be NULL): ragged batch, rows r >= fsn_row_frames(lengths, b, R_valid) of batch entry b are zero too
int fsn_launch_transpose(const float* in, float* out, int batch, int R, int C, long ld_in, long bs_in,
                         long ld_out, long bs_out, int R_valid, int C_valid, hipStream_t s,
                         const int* lengths = nullptr);
int fsn_launch_crm_rows(const float* crm_r, const float* crm_i, float* out, long r0, long n, int F, int FP, int T,
                        hipStream_t s);
int fsn_launch_binsum(const float* mag, double* binsum, int B, int Tp, int FP, hipStream_t s);
// lengths (may be NULL): ragged batch of T frames; utterance b's mean covers its own fsn_row_frames + Tp - T frames
int fsn_launch_offline_den(const double* binsum, const float* fb_out, float* den_fb, float* den_sb, int B,
                           int Tp, int F, int FP, int nb, int which, hipStream_t s, const int* lengths = nullptr,
                           int T = 0);
// The offline norm over segments (elementwise_kernels.hip): binsum [B][FP] += this segment's per-bin sums of mag [B][F][k];
// acc [B] += the sum of x [B][k][FP] over the frames frames_done + t < total_frames[b]; the two divisors (either output
// may be NULL) from the finished accumulators.  total_frames: device memory, [B].
int fsn_launch_binsum_accumulate(const float* mag, double* binsum, int B, int F, int FP, int k, hipStream_t s);
int fsn_launch_masked_sum_accumulate(const float* x, double* acc, const int* total_frames, int frames_done, int B, int k,
                                     int FP, hipStream_t s);
int fsn_launch_segment_den(const double* binsum, const double* fbsum, const int* total_frames, float* den_fb, float* den_sb,
                           int B, int F, int FP, int nb, hipStream_t s);
// carry / t0: streaming continuation (running sums of the t0 frames already seen, updated in place); NULL / 0 offline
int fsn_launch_cumulative_den_fb(const float* mag, float* den, int B, int Tp, int F, int FP, hipStream_t s,
                                 double* carry = nullptr, int t0 = 0);
int fsn_launch_cumulative_den_sb(const float* mag, const float* fb_out, float* den, int B, int Tp, int F,
                                 int FP, int nb, int Npad, hipStream_t s, double* carry = nullptr, int t0 = 0);

// gemm_kernels.hip
struct FsnGemmA {  // A operand description
    int kind;      // 0 row-major, 1 full-band input, 2 sub-band input
    const float* p0;  // row-major: matrix; fb/sb: mag [B][Tp][FP]
    const float* p1;  // sb: fb_out [B][Tp][FP]
    const float* den;  // fb/sb: divisor
    int den_mode;      // 0: den[b]   1: den[b*Tp + t] (fb) / den[t*den_stride + n] (sb)
    long ld;           // row-major leading dimension
    int B, Tp, F, FP, Npad, N, nb;
    int n_offset;      // sb: first unit of this launch (rows are n_offset .. n_offset + Npad - 1)
    int den_stride;    // sb, den_mode 1: row stride of den
};
struct FsnGemmC {  // C store description
    int kind;      // 0 fragment-order + bias, 1 fb_out rows (bias + relu), 2 crm planes, 3 plain row-major
    float* p0;
    float* p1;
    const float* bias;
    int B, Tp, T, F, FP, Npad, N, la;
    int n_off;     // kind 2: first unit of the rows (row r is step r / Npad, unit n_off + r % Npad)
    long ld;       // kind 3: leading dimension of p0
    int rows, cols;  // kind 3: valid extent
};
// input of one band section of Improved FullSubNet, normalised, in the LSTM entries' layout (section_kernels.hip)
size_t fsn_section_input_workspace_floats(int B, int F);
int fsn_launch_section_input(const float* noisy, const float* fb, int B, int F, int T, int lower, int units, int sc, int sn,
                             int fc, int fn, int u_lo, int u_hi, float eps, float* out, int Np, int ldo, void* workspace,
                             hipStream_t s, const int* frames = nullptr);  // frames (device, [B]): a ragged batch
void fsn_tn_plan_splits(int M, int Nc, long K, int arith, int* splits, long* bound);  // gemm_tn_kernels.hip (test hook)
// nn.Linear with O <= 4 outputs and I % 64 == 0 inputs as row dot products / outer products (gemm_kernels.hip)
bool fsn_linear_small_out_ok(int I, int O, long ldx);
int fsn_launch_linear_small_out(const float* x, long ldx, const float* w, const float* b, float* y, long R, int I, int O,
                                int relu, hipStream_t s);
int fsn_launch_linear_small_dx(const float* dy, long lddy, const float* w, float* dx, long lddx, long R, int I, int O,
                               hipStream_t s);
int fsn_launch_gemm(const FsnGemmA& a, const float* w_packed, const FsnGemmC& c, int row_tiles, int col_tiles,
                    int k_chunks, hipStream_t s);
// W [n_out][k] (transposed = 0) or W^T stored as [k][n_out] (transposed = 1, row stride ldw) -> B fragments
int fsn_launch_pack(const float* w, float* wp, int n_out, int k, int n_out_pad, int k_pad, hipStream_t s,
                    int transposed = 0, int ldw = 0);
int fsn_launch_bias_sum(const float* a, const float* b, float* out, int n, int n_pad, hipStream_t s);
int fsn_launch_bias_frag(const float* bias, float* frag, int n, hipStream_t s);

// fast_stream_kernels.hip: the stateful glue of fsn_fast_stream_step, time-major like fast_glue_kernels.hip.  One call
// advances B streams by k model steps t0 .. t0 + k - 1; n_low low-rate frames complete in it (the steps t % shrink == 0).
struct FsnFastStream {
    int B, Bp, M, k, t0, shrink, n_mel, n_enc, W, Wp, Np, n_low;
};
static inline int fsn_fast_stream_low_frames(int t0, int k, int shrink) {  // multiples of shrink in [t0, t0 + k)
    return (t0 + k - 1) / shrink - (t0 > 0 ? (t0 - 1) / shrink : -1);
}
// out[t][b] = mel[t][b] / (float(sum of the stream's mel values up to step t0 + t / (M (t0 + t + 1))) + EPSILON); mel_sum [B]
int fsn_launch_fast_stream_mel_norm(const float* mel, float* out, double* mel_sum, const FsnFastStream& a, hipStream_t s);
// unit windows of mel and enc, block accumulation from t0's phase (partial [B][M][W]), the unit norm (unit_sum [B M]):
// the n_low completed frames as units [n_low][Np][Wp]
int fsn_launch_fast_stream_units(const float* mel, const float* enc, long ld_enc, float* partial, double* unit_sum,
                                 float* units, const FsnFastStream& a, hipStream_t s);
// out[t][b] = enc[t][b] | the bottleneck output of low-rate frame (t0 + t) / shrink: slow [n_low][Np] where it completed in
// this call, held [B][M] otherwise; held becomes the call's last one
int fsn_launch_fast_stream_decoder_input(const float* enc, long ld_enc, const float* slow, float* held, float* out,
                                         const FsnFastStream& a, hipStream_t s);

// fast_segment_kernels.hip: the same glue under the offline norm, for fsn_fast_segment_*.  acc_mel / acc_unit [B]: the fp64
// accumulators of the two utterance means; total [B] (device): row b's own step count T_b + look_ahead.
// acc_mel[b] += the 64-band sums of mel [k][Bp][64], frame by frame
int fsn_launch_fast_segment_mel_stat(const float* mel, double* acc_mel, const FsnFastStream& a, hipStream_t s);
// out[t][b] = mel[t][b] / (float(acc_mel[b] / (64 total[b])) + 1e-5f), rows beyond B zero
int fsn_launch_fast_segment_mel_norm(const float* mel, float* out, const double* acc_mel, const int* total, const FsnFastStream& a,
                                     hipStream_t s);
// unit windows and block accumulation from t0's phase (partial [B][M][W]).  emit false: every low-rate frame of row b that
// completes at a step < total[b], its closing short block included, joins acc_unit[b]; units is not touched.  emit true: the
// n_low whole blocks as units [n_low][Np][Wp], divided by float(acc_unit[b] / (64 W Ts_b)) + 1e-5f
int fsn_launch_fast_segment_units(bool emit, const float* mel, const float* enc, long ld_enc, float* partial, double* acc_unit,
                                  const int* total, float* units, const FsnFastStream& a, hipStream_t s);
int fsn_launch_fast_segment_divisors(const double* acc_mel, const double* acc_unit, const int* total, float* den_mel,
                                     float* den_unit, int B, int shrink, int W, hipStream_t s);

// improved_stream_kernels.hip: the stateful glue of fsn_improved_stream_step, time-major.  One call advances B streams by k
// model steps t0 .. t0 + k - 1 on Fm = F - 1 bins (rows of FmP = round_up(Fm, 16) floats).
constexpr int kFsnImprovedMaxBins = 4096;  // Fm the sections kernels stage per frame (two rows of it in LDS)
struct FsnImprovedSection {
    int lower, units, sc, sn, fc, fn;  // the band's first bin, its units, centre / neighbours of the noisy and the fb window
    int W, Np, Ip;                     // sc + 2 sn + fc + 2 fn; the section's padded rows (B units) and columns
    float* x;                          // [k][Np][Ip]: the section's normalised input
    const float* o;                    // [k][Np][2 sc]: its output layer's rows
};
struct FsnImprovedStream {
    int B, Bp, F, Fm, FmP, k, sqrt_mode, n;
    long t0;
    FsnImprovedSection s[8];
    // NULL: every row stands at t0 (the lockstep entry).  Else [B] on the device, row b's own count (the streaming pool, whose
    // sessions are not in lockstep); a negative one marks a row that belongs to no session: its magnitudes count as zeros
    const long* t0_rows;
};
// (a) comp [k][Bp][FmP] = mag[b][f][t] ** fdrc without the last bin; fb_in = comp / (float(the stream's sum so far /
// (Fm (t0 + t + 1))) + EPSILON), zero in the padding; fb_sum [B] carries the sum, steps [B] becomes t0 + k
int fsn_launch_improved_stream_front(const float* mag, float* comp, float* fb_in, double* fb_sum, long* steps,
                                     const FsnImprovedStream& a, hipStream_t s);
// (c) every section's windows of comp and fb_out [k][Bp][ld_fb] (reflection at both spectrum ends), divided by the running
// mean of the section's units x W entries over the frames so far; sb_sum [n][B] carries the sums
int fsn_launch_improved_stream_sections(const float* comp, const float* fb_out, long ld_fb, double* sb_sum,
                                        const FsnImprovedStream& a, hipStream_t s);
// dst[j][0 .. count[j]) = src[j][..] for n <= 8 pairs in one launch: the sections' last h into the state
struct FsnImprovedKeep {
    float* dst[8];
    const float* src[8];
    long count[8];
    int n;
};
int fsn_launch_improved_stream_keep(const FsnImprovedKeep& a, hipStream_t s);
// (e) the sections' rows in bin order as the mask [B][2][F][k]; the last bin is zero
int fsn_launch_improved_stream_mask(float* mask, const FsnImprovedStream& a, hipStream_t s);

// improved_segment_kernels.hip: the same glue under the offline norms, for fsn_improved_segment_*.  total [B] (device): row
// b's own frame count T_b; a frame at or past it adds nothing to a sum and its compressed magnitude counts as zero.
// fb_sum[b] += the frames' sums of mag ** fdrc over the first Fm bins, frame by frame
int fsn_launch_improved_segment_stat(const float* mag, double* fb_sum, const int* total, const FsnImprovedStream& a, hipStream_t s);
// comp [k][Bp][FmP] and fb_in = comp / den.  mode 0: den = float(fb_sum[b] / (Fm T_b)) + EPSILON; 1: the running mean of
// fsn_launch_improved_stream_front, fb_sum carried here; 2: comp alone (fb_in, fb_sum, steps untouched).  0, 1: steps = t0 + k
int fsn_launch_improved_segment_front(int mode, const float* mag, float* comp, float* fb_in, double* fb_sum, long* steps,
                                      const int* total, const FsnImprovedStream& a, hipStream_t s);
// sb_sum[i][b] += every frame's sum over section i's windows of comp and fb_ws [k][Bp][ld_fb]; fb_out [k][B][Fm] = fb_ws
int fsn_launch_improved_segment_sums(const float* comp, const float* fb_ws, long ld_fb, float* fb_out, double* sb_sum,
                                     const int* total, const FsnImprovedStream& a, hipStream_t s);
// every section's windows of comp and fb_out [k][B][Fm] divided by float(sb_sum[i][b] / (units_i W_i T_b)) + EPSILON
int fsn_launch_improved_segment_sections(const float* comp, const float* fb_out, const double* sb_sum, const int* total,
                                         const FsnImprovedStream& a, hipStream_t s);
// den_fb [B], den_sb [n][B]: the divisors as the two kernels above form them
int fsn_launch_improved_segment_divisors(const double* fb_sum, const double* sb_sum, const int* total, float* den_fb, float* den_sb,
                                         const FsnImprovedStream& a, hipStream_t s);

// ---- streaming pool for Improved FullSubNet (fsn_improved_stream_pool_*, improved_stream_pool_kernels.hip) ------------------
// `capacity` records of slot_bytes each; all zeros is a fresh slot.  Byte offsets into a record (every array 256-byte
// aligned, slot_bytes a multiple of 256): what ONE stream of fsn_improved_stream_step carries at B = 1, without row padding -
//   fb[a]           a = h0, c0, h1, c1 of the full-band block [fb_hidden]
//   sb[i][a]        the same of section i [units_i][sb_hidden]
//   fb_sum, sb_sum  the full-band norm's fp64 sum; one fp64 sum per section [8]
//   steps           model steps this slot has taken (long; read and advanced on the device)
// - and the transform state at hop = F - 1, n_fft = 2 hop:
//   in_tail         the last hop of input [hop];  ola_tail  second half of the last synthesised frame [hop]
//   spec_re/_im     the spectrum [F] of the one frame that waits for its mask (the model has no look-ahead)
//   frame           that frame's number in its session (int; written by the analysis, read by the synthesis)
struct FsnImprovedPoolLayout {
    size_t fb[4], sb[8][4], fb_sum, sb_sum, steps, in_tail, ola_tail, spec_re, spec_im, frame, slot_bytes;
    int F, hop, Hf, Hs, n, units[8];
};
static inline FsnImprovedPoolLayout fsn_improved_pool_layout(int F, int Hf, int Hs, int sections, const int* units) {
    FsnImprovedPoolLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t r = o;
        o = fsn_round_up_sz(o + bytes, 256);
        return r;
    };
    L.F = F;
    L.hop = F - 1;
    L.Hf = Hf;
    L.Hs = Hs;
    L.n = sections;
    for (int a = 0; a < 4; ++a) L.fb[a] = take((size_t)Hf * sizeof(float));
    for (int i = 0; i < sections; ++i) {
        L.units[i] = units[i];
        for (int a = 0; a < 4; ++a) L.sb[i][a] = take((size_t)units[i] * Hs * sizeof(float));
    }
    L.fb_sum = take(sizeof(double));
    L.sb_sum = take(8 * sizeof(double));
    L.steps = take(sizeof(long));
    L.in_tail = take((size_t)L.hop * sizeof(float));
    L.ola_tail = take((size_t)L.hop * sizeof(float));
    L.spec_re = take((size_t)F * sizeof(float));
    L.spec_im = take((size_t)F * sizeof(float));
    L.frame = take(sizeof(int));
    L.slot_bytes = o;
    return L;
}
// One call on the n listed slots.  The compact batch is a state in fsn_improved_stream_step's layout at B = n: tile[0][a]
// [Bp][Hf] the full-band block's arrays, tile[1 + i][a] [rows[1 + i]][Hs] section i's (row b units_i + u), fb_sum [n], sb_sum
// [sections][n], and t0 [n] each row's own count (-1: the row's id is outside the pool).
struct FsnImprovedPool {
    char* state;
    FsnImprovedPoolLayout L;
    const int* slots;
    int capacity, n, k;
    float* tile[9][4];
    int rows[9];
    double *fb_sum, *sb_sum;
    long* t0;
};
// the listed records' rows, sums and counts into the compact batch; pad rows and rows of an id outside the pool are zeros
int fsn_launch_improved_pool_gather(const FsnImprovedPool& a, hipStream_t s);
// ... and back to the listed, valid records, their counts advanced by k: the last launch of a step
int fsn_launch_improved_pool_scatter(const FsnImprovedPool& a, hipStream_t s);
// one analysis / synthesis frame per listed slot at n_fft = 2 hop = 2 (F - 1) (see the kernels)
int fsn_launch_improved_pool_analysis(void* state, const FsnImprovedPoolLayout& L, int capacity, const int* slots, int n,
                                      const float* hops, const float* prime, const int* frame_no, const float* window, float* mag,
                                      hipStream_t s);
int fsn_launch_improved_pool_synthesis(void* state, const FsnImprovedPoolLayout& L, int capacity, const int* slots, int n,
                                       const float* mask, const int* tail_samples, const float* window, float* out, hipStream_t s);

// ---- streaming pool for Fast FullSubNet (fsn_fast_stream_pool_*, fast_stream_pool_kernels.hip) -------------------------------
// `capacity` records of slot_bytes each; all zeros is a fresh slot.  Byte offsets into a record (every array 256-byte
// aligned, slot_bytes a multiple of 256): what ONE stream of fsn_fast_stream_step carries -
//   pair[a]          a = 2 layer + (0 h | 1 c), layer = encoder.0 [384], encoder.1 [320], decoder_lstm.0 [512], decoder_lstm.1 [512]
//   bn[l][0 h | 1 c] the bottleneck's layer l, [64][H]
//   mel_sum          the mel norm's fp64 sum;  unit_sum  the unit norm's 64 fp64 sums
//   partial          the open block's sum [64][W];  held  the held bottleneck output [64]
// - then the slot's own step count and the four transform fields as in FsnPoolLayout.
__host__ __device__ __forceinline__ int fsn_fast_pair_h(int layer) { return layer == 0 ? 384 : layer == 1 ? 320 : 512; }
struct FsnFastPoolLayout {
    size_t pair[8], bn[2][2], mel_sum, unit_sum, partial, held, steps, in_tail, ola_tail, ring_re, ring_im, slot_bytes;
    int F, FP, R, H, layers, W;
};
static inline FsnFastPoolLayout fsn_fast_pool_layout(int F, int bn_hidden, int bn_layers, int W, int look_ahead) {
    FsnFastPoolLayout L{};
    size_t o = 0;
    auto take = [&](size_t bytes) {
        const size_t r = o;
        o = fsn_round_up_sz(o + bytes, 256);
        return r;
    };
    L.F = F;
    L.FP = fsn_fpad(F);
    L.R = look_ahead + 1;
    L.H = bn_hidden;
    L.layers = bn_layers;
    L.W = W;
    for (int a = 0; a < 8; ++a) L.pair[a] = take((size_t)fsn_fast_pair_h(a / 2) * sizeof(float));
    for (int l = 0; l < bn_layers; ++l)
        for (int a = 0; a < 2; ++a) L.bn[l][a] = take((size_t)64 * bn_hidden * sizeof(float));
    L.mel_sum = take(sizeof(double));
    L.unit_sum = take(64 * sizeof(double));
    L.partial = take((size_t)64 * W * sizeof(float));
    L.held = take(64 * sizeof(float));
    L.steps = take(sizeof(int));
    L.in_tail = take(256 * sizeof(float));
    L.ola_tail = take(256 * sizeof(float));
    L.ring_re = take((size_t)L.R * L.FP * sizeof(float));
    L.ring_im = take((size_t)L.R * L.FP * sizeof(float));
    L.slot_bytes = o;
    return L;
}
// What fft_kernels.hip's pool kernels (and the reset kernel) read of a layout: the transform fields, F, FP, R, slot_bytes
static inline FsnPoolLayout fsn_fast_pool_transform_layout(const FsnFastPoolLayout& f) {
    FsnPoolLayout L{};
    L.in_tail = f.in_tail;
    L.ola_tail = f.ola_tail;
    L.ring_re = f.ring_re;
    L.ring_im = f.ring_im;
    L.slot_bytes = f.slot_bytes;
    L.F = f.F;
    L.FP = f.FP;
    L.R = f.R;
    return L;
}
// One call on the n listed slots, k steps each from the slot's own count: every slot completes lo = k / shrink or hi =
// ceil(k / shrink) low-rate frames, and rows [0, n_long) of `slots` are the ones that complete hi (status: raised by the order
// check when they are not; every kernel that writes a record then leaves it alone).  Tensors are time-major with Bp =
// round_up(n, 16) rows per step; the bottleneck's rows are n 64 per low-rate frame ordinal (Np), of ordinal lo the first
// n_long 64.
struct FsnFastPool {
    char* state;
    FsnFastPoolLayout L;
    const int* slots;
    unsigned* status;
    int capacity, n, n_long, k, Bp, Np, shrink, n_mel, n_enc, W, Wp, lo, hi;
};
// (h, c) tiles of a call: pair[a] [Bp][fsn_fast_pair_h(a / 2)], bn[l][0 h | 1 c] [Np][H]
struct FsnFastPoolTiles {
    float *pair[8], *bn[2][2];
};
int fsn_launch_fast_pool_check(const FsnFastPool& a, hipStream_t s);
int fsn_launch_fast_pool_gather_pairs(const FsnFastPool& a, const FsnFastPoolTiles& t, hipStream_t s);
// the last launch of a step: it also advances the listed slots' step counts by k
int fsn_launch_fast_pool_scatter_pairs(const FsnFastPool& a, const FsnFastPoolTiles& t, hipStream_t s);
// the bottleneck rows of the first `slots_run` listed slots
int fsn_launch_fast_pool_gather_bn(const FsnFastPool& a, const FsnFastPoolTiles& t, int slots_run, hipStream_t s);
int fsn_launch_fast_pool_scatter_bn(const FsnFastPool& a, const FsnFastPoolTiles& t, int slots_run, hipStream_t s);
// the three state-touching stages of fast_stream_kernels.hip with t0 and the state taken from each row's record
int fsn_launch_fast_pool_mel_norm(const float* mel, float* out, const FsnFastPool& a, hipStream_t s);
int fsn_launch_fast_pool_units(const float* mel, const float* enc, long ld_enc, float* units, const FsnFastPool& a, hipStream_t s);
int fsn_launch_fast_pool_decoder_input(const float* enc, long ld_enc, const float* slow, float* out, const FsnFastPool& a,
                                       hipStream_t s);

size_t fsn_lstm2_group_bptt_flag_words(int clusters);  // lstm_group_bptt_kernels.hip
int fsn_lstm2_group_bptt_clusters(int tiles);
int fsn_launch_lstm2_group_bptt(const float* dh1, const float* whh1T_p, const float* wih1T_p, const float* whh0T_p,
                                const float* save0, const float* save1, float* dg0, float* dg1, float* dx, unsigned* flags,
                                int Tp, int Nrows, int clusters, int H, hipStream_t s, int arith = FSN_ARITH_F32,
                                const void* w16 = nullptr);
// lstm_group16_kernels.hip: the same two-layer forward-with-saves / BPTT for the 16-bit training arithmetic (autocast),
// built for it: transposed products, per-wave weight streams, 16-byte hand-offs, K-split BPTT (see the file)
int fsn_lstm2_g16_clusters(int tiles);
size_t fsn_lstm2_g16_flag_words(int clusters);
size_t fsn_lstm2_g16_status_word(int clusters);
size_t fsn_lstm2_g16_partial_floats(int clusters);
size_t fsn_lstm2_g16_fwd_weight_halves(int Ipad);
size_t fsn_lstm2_g16_bwd_weight_bytes();
int fsn_launch_lstm2_g16_train(const float* x, int I, int Nrows, const float* w_ih0, const float* w_hh0, const float* w_ih1,
                               const float* w_hh1, const float* bias0, const float* bias1, float* hseq0, float* hseq1,
                               float* save0, float* save1, unsigned* flags, void* w16, int Tp, int clusters, int H,
                               hipStream_t s, int arith);
int fsn_launch_lstm2_g16_bptt(const float* dh1, const float* w_hh1, const float* w_ih1, const float* w_hh0, const float* save0,
                              const float* save1, float* dg0, float* dg1, float* exchange, unsigned* flags, void* wbuf, int Tp,
                              int Nrows, int clusters, int H, hipStream_t s, int arith, void* dg16_0, void* dg16_1, float* dbp,
                              int dg1_f32, int dg0_f32 = 1);
int fsn_launch_g16_left_to16(const float* dg, void* dg16, int Tp, int Nrows, long row0, int left, hipStream_t s, int arith);
int fsn_launch_lstm2_g16_finish(const float* dg1, const float* dg0, void* dg16_1, void* dg16_0, const float* dbp, int clusters, int Tp,
                                int Nrows, int left, float* db1, float* db0, hipStream_t s, int arith);
// fb_chain_bptt_kernels.hip: BPTT of the full-band model's two layers (16 rows, H = 512) as one persistent launch
bool fsn_fb_chain_bptt_supported(int H, int N);
int fsn_fb_chain_bptt_max_steps();
size_t fsn_fb_chain_bptt_dx_floats(int Tp, int N);
size_t fsn_fb_chain_bptt_flag_words();
size_t fsn_fb_chain_bptt_status_word();
int fsn_launch_fb_chain_bptt(const float* dh1, const float* whh1T_p, const float* wih1T_p, const float* whh0T_p,
                             const float* save0, const float* save1, float* dg0, float* dg1, float* dx, unsigned* flags,
                             int Tp, int N, int H, hipStream_t s);
int fsn_launch_zero_words(unsigned* p, size_t n, hipStream_t s);  // elementwise_kernels.hip
// dst[i] = src[i] rounded to fp16 / bf16 (arith = FSN_ARITH_F16 / _BF16): the 16-bit copy of a packed weight buffer
int fsn_launch_to16(const float* src, void* dst, size_t n, int arith, hipStream_t s);
// out[0..n) = NaN if *status != 0 (a persistent kernel hit its wait bound); status words of the kernels' flag arrays.
// The same kernel reports the event to the host: the sticky status record of the caller's stream (fsn_stream_status).
int fsn_launch_poison_if(const unsigned* status, float* out, size_t n, hipStream_t s);
int fsn_launch_hog(int workgroups, int lds_bytes, int heavy, unsigned long long ticks, float* sink, hipStream_t s);

// ---- residency contract of the persistent kernels whose workgroups wait for each other ----------
// (fsn_api.hip)  fb_chain_kernel, lstm2_group_kernel, lstm2_group_bptt_kernel and fb_chain_bptt_kernel make progress
// only when their WHOLE grid is resident.  The library guarantees what it can decide alone - the grid fits an idle
// device (fsn_grid_fits, from the compiled kernel's occupancy), its own persistent launches of different streams
// share the chip only when the set is provably placeable (PersistLaunch / fsn_persist_admit) - and bounds what it cannot: a foreign kernel (RCCL, another stream of the process) that holds CUs
// delays the missing workgroups until it ends; the resident ones wait for them, by the CLOCK (fsn_spin_ticks, not by a
// poll count), and a wait that runs out raises the launch's status word: outputs become NaN and the host learns of it
// through the stream's sticky status (FSN_ERR_TIMEOUT).
bool fsn_persistent_allowed();        // false: the caller switched these kernels off (fsn_set_persistent_mode)
unsigned long long fsn_spin_ticks();  // the wait bound in ticks of wall_clock64() on the current device
// whole grid co-resident on an idle device?  (blocks per CU from hipOccupancyMaxActiveBlocksPerMultiprocessor, cached)
bool fsn_grid_fits(const void* kernel, int block_threads, unsigned grid);
// every launch of such a kernel reports its footprint first: the launch then waits for earlier persistent launches on
// other streams until the set that may run beside it is provably placeable (fsn_api.hip, PersistLaunch)
void fsn_persist_admit(const void* kernel, int block_threads, unsigned grid);
#define FSN_PERSIST_LAUNCH(kernel, grid, block, s, ...)                                   \
    do {                                                                                  \
        fsn_persist_admit((const void*)(kernel), (int)(block).x, (unsigned)(grid).x);     \
        hipLaunchKernelGGL((kernel), grid, block, 0, s, __VA_ARGS__);                     \
    } while (0)
unsigned* fsn_ctx_sticky();           // device-visible sticky status record {status, events} of the running call's stream

size_t fsn_fb_chain_status_word();
size_t fsn_lstm2_group_status_word(int clusters);
size_t fsn_lstm2_group_bptt_status_word(int clusters);

// one stack of fsn_launch_lstm2_group_multi (lstm_group_kernels.hip)
struct FsnGroupStack {
    const float* gx;
    const float *whh0_p, *wih1_p, *whh1_p, *bias1;
    float *hseq0, *hseq1;
    int N;
};
int fsn_lstm2_group_multi_cap();
int fsn_launch_lstm2_group_multi(int n, const FsnGroupStack* st, unsigned* flags, int Tp, int H, hipStream_t s);
int fsn_launch_lstm2_group_train(const float* x, long x_ld, int x_cols, int Nrows, const float* wih0_p, const float* whh0_p,
                                 const float* wih1_p, const float* whh1_p, const float* bias0, const float* bias1,
                                 float* hseq0, float* hseq1, float* save0, float* save1, unsigned* flags, int Tp,
                                 int clusters, int H, hipStream_t s, int arith = FSN_ARITH_F32,
                                 const void* w16 = nullptr);  // lstm_group_kernels.hip; w16: fsn_launch_to16 of the packed weights

// fb_chain_kernels.hip: the full-band model's two LSTM layers over all frames as one persistent launch
bool fsn_fb_chain_supported(int H, int Npad);
int fsn_fb_chain_max_steps();
size_t fsn_fb_chain_exchange_floats(int Tp, int Npad);
size_t fsn_fb_chain_flag_words();
int fsn_launch_fb_chain(const float* gx0, const float* whh0_p, const float* wih1_p, const float* whh1_p, const float* b1,
                        float* exchange, unsigned* flags, float* hseq1, int Tp, int Npad, int H, hipStream_t s,
                        float* hseq0 = nullptr, float* save0 = nullptr, float* save1 = nullptr, int cell = 0);
// gru_kernels.hip: nn.GRU's [3H] gate rows (r, z, n) of one layer as the FOUR-gate cell the chain kernel runs (r | z | nx | nh):
// w_ih4 [4H][I] = W_ir; W_iz; W_in; 0   w_hh4 [4H][H] = W_hr; W_hz; 0; W_hn   b4 [4H] = b_ir + b_hr; b_iz + b_hz; b_in; b_hn
// order 1: the gate slots of the many-row persistent kernels (lstm_cell.h): nh | r | nx | z
int fsn_launch_gru_expand4(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* w_ih4, float* w_hh4,
                           float* b4, int I, int H, hipStream_t s, int order = 0);

// gemm_tn_kernels.hip (training step: weight gradients)
// C [M][Nc] = sum_k A[k][M]^T B[k][Nc]   (both operands row-major over k; split-K, deterministic 2-pass)
size_t fsn_gemm_tn_workspace_bytes(int M, int Nc, long K);
int fsn_launch_gemm_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int Nc, long K,
                       void* workspace, hipStream_t s, float* colsum_out = nullptr, int arith = FSN_ARITH_F32);
int fsn_launch_colsum(const float* A, long lda, float* out, int cols, long rows, void* workspace, hipStream_t s);
size_t fsn_colsum_workspace_bytes(int cols, long rows);
// its split-K plan (host code), shared with the 16-bit-operand forms
struct FsnTnPlan {
    int m_blocks, n_blocks, splits, narrow;
    int square;  // 192 x 192 tiles, every K split's tiles on one XCD (bandwidth-bound under the 16-bit arithmetic)
    long k_per_split;
};
FsnTnPlan fsn_tn_plan(int M, int Nc, long K, int arith = FSN_ARITH_F32, bool allow_square = true);
long fsn_tn_max_splits(int M, int Nc);
constexpr size_t kFsnTnOnePerCu = 96 * 1024;  // LDS reservation (never touched): one workgroup per CU
// gemm_tn16_kernels.hip: the same product with both operands 16-bit in memory (LDS-DMA staging, transposing LDS reads);
// workspace as above
bool fsn_gemm_tn16h_supported(int M, int Nc, long K);
int fsn_gemm_tn16h_form(int M, int Nc, long K, int* splits);  // 0 no plan, 1 the 192 x 192 form, 2 the 192 x 384 form; its K splits
bool fsn_gemm_tn16n_supported(int M, int Nc, long K);  // the narrow form (Nc <= 32) and dx from the 16-bit gate gradients
int fsn_gemm_tn16n_splits(int M, int Nc, long K);      // its K splits (0: unsupported)
int fsn_launch_gemm_tn16n(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                          void* workspace, hipStream_t s, int arith);
bool fsn_gemm_dx16_supported(long rows, int G, int I);
int fsn_launch_gemm_dx16(const void* dg16, long ld16, const float* w, void* wfrag, float* dx, long lddx, long rows, int G, int I,
                         hipStream_t s, int arith);
int fsn_launch_gemm_tn16h(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                          void* workspace, hipStream_t s, int arith);
// bptt_step_kernels.hip (training step: BPTT one step at a time)
int fsn_launch_bptt_step(const float* dh_out, const float* dgates_next, const float* whhT_p, float* dc,
                         const float* gates, const float* c_t, const float* c_prev, float* dgates, int row_tiles, int H,
                         int last, int first, hipStream_t s);
int fsn_launch_bptt_elem(const float* dh_out, const float* dh_rec, float* dc, const float* gates, const float* c_t,
                         const float* c_prev, float* dgates, long n_elems, int H, int last, int first, hipStream_t s);

// gru_kernels.hip
int fsn_launch_gru_step(const float* gx, const float* whh_p, const float* b_hn, const float* h_prev, float* h_out,
                        float* save, long gx_rt0, int row_tiles, int H, int first, hipStream_t s, int beside_persistent = 0);
int fsn_launch_gru_bptt_step(const float* dh_out, const float* dgx_next, const float* dghn_next, const float* whhT_p,
                             float* carry, const float* save, const float* h_prev, float* dgx, float* dghn,
                             int row_tiles, int H, int last, int first, hipStream_t s);

// lstm_rec_kernels.hip, lstm_rec_in_kernels.hip, lstm_rec_x_kernels.hip, lstm_step_kernels.hip
// Sub-band model input (fullsubnet/model.py:98-111) for kernels that build it on the fly:
// channel c < 2nb+1 of unit n = b F + f at frame t is mag[b][t][reflect(f + c - nb)], channel 2nb+1
// is fb_out[b][t][f]; everything divided by den (den_mode 0: den[b], 1: den[t * den_stride + n]).
struct FsnSbInput {
    const float* mag;
    const float* fb_out;
    const float* den;
    const float* wih_p;  // packed W_ih [4H/16][kin_pad/16][64][4]
    const float* bias;   // b_ih + b_hh [4H]
    int den_mode, den_stride;
    int B, Tp, F, FP, N, nb, kin_chunks;
    // generic form (x_rows != NULL): the layer input is a plain row-major matrix, element (t, n, c) at
    // x_rows[(t * x_step + n) * x_ld + c] with zero padding up to 16 kin_chunks columns; N = valid rows
    const float* x_rows;
    long x_ld, x_step;
    // row-range calls (fsn_fullsubnet_forward_rows): local row n of this launch is row n + row0 of the flattened
    // (b, f) index space; N stays the number of valid LOCAL rows.  0 everywhere else.
    long row0;
};

#ifdef __HIPCC__
// Element (row n, column c) of frame t of the sub-band model input: freq_unfold + cat + norm of
// fullsubnet/model.py:98-111 (reflect-padded neighbours of the noisy magnitude, then the full-band output,
// divided by the norm statistic), or the plain row-major form; zero beyond the valid rows / columns.
__device__ __forceinline__ float fsn_sb_input_value(const FsnSbInput& x, long n, int c, int t) {
    if (x.x_rows) return n < x.N ? x.x_rows[((long)t * x.x_step + n) * x.x_ld + c] : 0.f;
    if (n >= x.N || c > 2 * x.nb + 1) return 0.f;
    n += x.row0;
    const int b = (int)(n / x.F), f = (int)(n % x.F);
    const long fo = ((long)b * x.Tp + t) * x.FP;
    int j = f + c - x.nb;
    j = j < 0 ? -j : j;
    j = j >= x.F ? 2 * (x.F - 1) - j : j;
    const float raw = c <= 2 * x.nb ? x.mag[fo + j] : x.fb_out[fo + f];
    return raw / x.den[x.den_mode ? (long)t * x.den_stride + n : b];
}
#endif

// Output layer (nn.Linear(H, 2), fullsubnet/model.py:53-61 + the reshape of :129-135) fused into the
// last sub-band recurrent layer: the two mask values of a row are formed from h_t while it sits in LDS
// and go straight to the compressed-mask planes; the hidden sequence of that layer is never written.
struct FsnRecFc {
    const float* w_p;   // packed output weights [1][H/16][64][4] (rows 0, 1); NULL: not fused
    const float* bias;  // [16]
    float* crm_r;
    float* crm_i;       // [B][T][FP]
    int N, F, FP, T, la;
    long row0;          // first row of a row-range call in the flattened (b, f) space (N = valid local rows)
};

struct FsnRecPlan {
    int rt;          // 16-row tiles per workgroup of the persistent recurrent kernel
    int main_wgs;    // its grid: rows [0, main_wgs * rt * 16)
    int left_tiles;  // trailing tiles handled step by step on the auxiliary stream
    int tiles;       // all tiles = npad / 16
    int npad;        // padded row count (row stride of every [t][n] buffer)
};
FsnRecPlan fsn_lstm_rec_plan(int N, int H);
// beside_persistent: the launch runs concurrently with a resident lstm_rec_kernel (left-over tiles) and must
// use the small-footprint single-tile kernel to get a slot next to it
int fsn_launch_lstm_step(const float* gx, const float* whh_p, const float* h_prev, float* h_out, float* c,
                         long gx_rt0, int row_tiles, int H, int first, hipStream_t s, int beside_persistent = 0);
int fsn_launch_lstm_step_cu(const float* gx, const float* whh_p, const float* h_prev, float* h_out, float* c,
                            long gx_rt0, int row_tiles, int H, int first, hipStream_t s, const float* c_prev = nullptr,
                            float* gates_out = nullptr);
int fsn_launch_lstm_step_train(const float* gx, const float* whh_p, const float* h_prev, float* h_out,
                               const float* c_prev, float* c_out, float* gates_out, long gx_rt0, int row_tiles, int H,
                               int first, hipStream_t s);
// several independent layers of one hidden size per step launch (lstm_step_multi_kernel): set j is the arguments of
// fsn_launch_lstm_step for its own rows, which are the launch's row tiles [tile0, tile0 + tiles)
struct FsnStepSet {
    const float *gx, *whh_p, *h_prev;
    float *h_out, *c;
    long gx_rt0;
    int tile0, tiles;
};
struct FsnStepSets {
    FsnStepSet s[8];
    int n;
};
int fsn_launch_lstm_step_multi(const FsnStepSets& sets, int H, hipStream_t s);
// xin == NULL: accumulators start from the precomputed projection gx; otherwise the (K = 2nb+2)
// input projection of the sub-band model's first layer is computed inside the kernel from xin.
int fsn_launch_lstm_rec(const float* gx, const FsnSbInput* xin, const float* whh_p, float* hseq, int Tp, int Npad,
                        int H, int RT, int main_wgs, hipStream_t s, const FsnRecFc* fc = nullptr);
bool fsn_lstm_rec_can_fuse_fc(int RT, bool xin);
// first sub-band layer on the persistent kernel with the weight ring / deferred input staging (see the kernel)
bool fsn_lstm_rec_in_supported(const FsnSbInput* xin, const float* whh_p, int H, int RT);
int fsn_launch_lstm_rec_in(const FsnSbInput* xin, const float* whh_p, float* hseq, int Tp, int Npad, int H, int RT,
                           int main_wgs, hipStream_t s, int cell = 0);
// a layer with its input projection inside: xseq [Tp][Npad][H] is the hidden sequence of the layer below,
// wih_p / whh_p the packed weights, bias = b_ih + b_hh [4H]; either the output layer (fc) is fused and nothing else is
// stored (the last layer of the sub-band model), or hseq_out [Tp][Npad][H] receives h_t (a layer inside a stack)
bool fsn_lstm_rec_x_supported(int H, int RT);
int fsn_launch_lstm_rec_x(const float* xseq, const float* wih_p, const float* whh_p, const float* bias, int Tp, int Npad,
                          int H, int RT, int main_wgs, hipStream_t s, const FsnRecFc* fc, float* hseq_out = nullptr, int cell = 0);
// state_h0 / state_h1 (may be NULL): streaming continuation - the hidden states before this call ([rows][H],
// updated to the last step's on return); c0 / c1 then hold the carried cell states.
int fsn_launch_lstm_wavefront2(const float* gx0, long gx_stride, long gx_off, const float* whh0_p, const float* wih1_p,
                               const float* bias1_frag, const float* whh1_p, float* hseq0, float* hseq1, long hs_stride,
                               long hs_off, float* c0, float* c1, int T, int row_tiles, int H, hipStream_t s,
                               float* state_h0 = nullptr, float* state_h1 = nullptr, int beside_group = 0);
int fsn_launch_lstm_wavefront2w(const float* gx0, long gx_stride, long gx_off, const float* whh0_p,
                                const float* wih1_p, const float* bias1_frag, const float* whh1_p, float* hseq0,
                                float* hseq1, long hs_stride, long hs_off, float* c0, float* c1, int T, int row_tiles,
                                int H0, int H1, hipStream_t s, float* state_h0 = nullptr, float* state_h1 = nullptr,
                                int beside_group = 0);

// lstm_group_kernels.hip: the sub-band model for few rows as ONE persistent launch (clusters of 8 workgroups per 64
// rows, both layers + output layer; see the file).  exchange: fsn_lstm2_group_exchange_floats(clusters) floats,
// flags: fsn_lstm2_group_flag_words(clusters) 32-bit words (cleared inside the launcher).
size_t fsn_lstm2_group_exchange_floats(int clusters);
size_t fsn_lstm2_group_flag_words(int clusters);
int fsn_lstm2_group_clusters(int tiles);
int fsn_launch_lstm2_group(const FsnSbInput* xin, const float* whh0_p, const float* wih1_p, const float* whh1_p,
                           const float* bias1, float* exchange, unsigned* flags, const FsnRecFc* fc, int Tp, int clusters,
                           int H, hipStream_t s);

// gemm_f16x3_kernels.hip (experimental, opt-in: FSN_F16X3=1)
size_t fsn_f16x3_packed_halves(int n_out, int k);
int fsn_launch_pack_f16x3(const float* w, void* packed, int n_out, int k, hipStream_t s, float scale = 256.f);
int fsn_launch_gemm_f16x3(const float* A, long lda, const void* packed, const float* bias, float* C, long row_tiles,
                          int n_out, int k, hipStream_t s);
// lstm_f16x3_kernels.hip (experimental, opt-in: FSN_F16X3=1)
int fsn_launch_lstm_rec_f16x3(const float* gx, const void* packed, int Tp, int Npad, int H, int RT, int main_wgs,
                              const FsnRecFc* fc, hipStream_t s);
float fsn_f16x3_wih0_scale();
int fsn_launch_lstm_rec_xin_f16x3(const FsnSbInput* xin, const void* wih_packed, const void* whh_packed, float* hseq,
                                  int Tp, int Npad, int H, int RT, int main_wgs, hipStream_t s);
