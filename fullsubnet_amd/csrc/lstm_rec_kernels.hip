// Recurrent half of nn.LSTM (audio_zen/model/module/sequence_model.py:52-58,116-117) for gfx950: per step
//     gates = gx[t] + h_{t-1} W_hh^T ;  c = sig(f) c + sig(i) tanh(g) ;  h = sig(o) tanh(c)
// with PyTorch's gate order (i, f, g, o) along the 4H axis and h_0 = c_0 = 0.  The input half  gx = W_ih x_t + b_ih + b_hh
// is produced beforehand by gemm_kernels.hip in accumulator-fragment order, or formed inside the kernel.
//
// This file: the MANY-ROW regime's general kernels and its row-tile planner (the sub-band model: N = B F = 16 448
// independent sequences).  A workgroup owns 16 RT rows for the whole utterance: h lives in LDS, c in registers, W_hh
// streams from L2 as pre-tiled B fragments (2.4 MB, re-read once per step by each workgroup, ~15 GB/s per CU at RT = 5).
// Each wave owns 32 hidden units x all four gates, so the cell update is lane-local in MFMA accumulator layout; the four
// gates are accumulated one after the other to keep accumulators + c + one temporary inside the 168-VGPR budget of 3
// waves per SIMD.  MFMA-bound: 16 RT x 384 x 1536 MAC per step per workgroup.
// The successors with the input projection inside and a weight-fragment ring are lstm_rec_in_kernels.hip (first layer of
// a stack) and lstm_rec_x_kernels.hip (a layer above another); the FEW-row regime is lstm_step_kernels.hip.
//
// Which plan reaches which instantiation (all through run_recurrence, fsn_api_fullsubnet.hip, with the FsnRecPlan of
// fsn_lstm_rec_plan below or of fsn_api_layers.hip's layer_plan; H = 384 only):
//   lstm_rec_kernel<384, 2..4, 2, XIN = true>   the fallback of a first layer when fsn_lstm_rec_in_supported says no: a
//       gathered sub-band input whose padded neighbourhood width is not 32 columns, W_hh not packed behind W_ih, or the
//       f16x3 arithmetic for a layer its own split-precision form does not take
//   lstm_rec_kernel<384, 5, 2, XIN = true>      the same at five row tiles per workgroup (the whole-rounds plan / one
//       round of five), which neither successor holds in LDS
//   lstm_rec_kernel<384, 2..4, 2, XIN = false>  a layer on a precomputed projection: the last sub-band layer when
//       lstm_rec_x_kernel is not used (CoreDims::l1x false: 16-bit / f16x3 arithmetic), with the output layer fused when
//       fsn_lstm_rec_can_fuse_fc; a stand-alone layer (fsn_lstm_layer_forward) whose input is wider than 32 columns and
//       is not an equally wide layer below
//   lstm_rec_kernel<384, 5, 2, XIN = false>     the same at five row tiles (fused output layer included)
//   lstm_rec_small_kernel<384, 1, 2, XIN>       RT = 1: 160 - 256 row tiles, one tile per CU (both input forms; never
//       with the fused output layer - launch_rec refuses it)
#include "fsn_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// One frame of the sub-band model input for the rows of this workgroup, written to LDS as
// xl[row][0 .. 16 kin_chunks) (zero padded): freq_unfold + cat + norm of fullsubnet/model.py:98-111.
template <int NTHREADS>
__device__ __forceinline__ void stage_sb_input(const FsnSbInput& x, float* xl, int xs, long n0, int rows, int t) {
    const int kin = 16 * x.kin_chunks;
    for (int i = threadIdx.x; i < rows * kin; i += NTHREADS) {
        const int row = i / kin, c = i % kin;
        const float v = fsn_sb_input_value(x, n0 + row, c, t);
        xl[row * xs + c] = v;
    }
}

template <int H, int RT, int UG, bool XIN>
__global__ __launch_bounds__((H / (16 * UG)) * 64) void lstm_rec_kernel(const float* __restrict__ gx,
                                                                        const FsnSbInput xin,
                                                                        const float* __restrict__ whh_p,
                                                                        float* __restrict__ hseq, int Tp, int Npad,
                                                                        const FsnRecFc fc) {
    constexpr int NW = H / (16 * UG);   // waves per workgroup
    constexpr int KC = H / 16;          // k chunks == unit groups
    constexpr int CT = 4 * KC;          // column tiles of the gate matrix
    constexpr int HS = H + 4;           // LDS row stride (floats): 16 B aligned, breaks the 64-bank period
    constexpr int ROWS = RT * 16;
    constexpr int UNR = RT >= 3 ? 1 : (RT == 2 ? 2 : 4);  // K-loop unroll: bound the in-flight B fragments
    extern __shared__ __attribute__((aligned(16))) float hl[];  // [ROWS][HS] (+ 2 x [ROWS][XS] when XIN)
    // XIN: the first sub-band layer builds its input projection itself (K = 2nb+2 = 32: two more
    // chunks per gate) from a double-buffered LDS tile of the unfolded, normalised input, instead of
    // reading a 19.2 GB precomputed gx that an HBM-write-bound GEMM would have to produce first.
    const int XS = XIN ? 16 * xin.kin_chunks + 4 : 0;
    float* xl = hl + ROWS * HS;
    float* wl = xl;  // !XIN with the output layer fused: its two weight rows [2][H] sit here instead

    // wave-uniform, and told so: everything derived from it (unit group, weight / projection tile bases) then lives in
    // scalar registers and the loads take the scalar-base + 32-bit lane offset form
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const long n0 = (long)blockIdx.x * ROWS;
    const bool fuse_fc = !XIN && fc.w_p != nullptr;
    if (fuse_fc) {  // un-tile rows 0 / 1 of the packed output weights: element (c, k) of fragment order
        for (int i = threadIdx.x; i < 2 * H; i += NW * 64) {
            const int c = i / H, k = i % H;
            wl[i] = fc.w_p[(((k >> 4) * 64) + ((k & 15) >> 2) * 16 + c) * 4 + (k & 3)];
        }
    }

    float cst[RT][UG][4], tmp[RT][UG][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int u = 0; u < UG; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) cst[rt][u][i] = 0.f;
    for (int i = threadIdx.x; i < ROWS * HS; i += NW * 64) hl[i] = 0.f;
    if (XIN) stage_sb_input<NW * 64>(xin, xl, XS, n0, ROWS, 0);
    __syncthreads();

    for (int t = 0; t < Tp; ++t) {
        const long gx_rt0 = ((long)t * Npad + n0) >> 4;
        // frame t+1 goes into the other x buffer; it was last read in step t-1, which ended with
        // two barriers, and is first read after the two barriers that end this step
        if (XIN && t + 1 < Tp) stage_sb_input<NW * 64>(xin, xl + ((t + 1) & 1) * ROWS * XS, XS, n0, ROWS, t + 1);
        const float* xt = xl + (t & 1) * ROWS * XS;
        // gate order of evaluation: f (1), i (0), g (2), o (3)
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            // The four passes are unrolled, so that the cell update of each is straight-line code that updates c and
            // the temporary in place.  Two things keep the register count of the rolled loop: nothing is scheduled
            // across a pass boundary, and the gate index is opaque to the optimiser - as a constant, the per-gate
            // operand addresses of all four passes are hoisted out of the time loop and held live (85+ spills).
            __builtin_amdgcn_sched_barrier(0);
            int g = pass == 0 ? 1 : (pass == 1 ? 0 : pass);
            asm volatile("" : "+s"(g));
            f32x4 acc[RT][UG];
            unsigned bo[UG];  // 32-bit element offsets from the (uniform) weight base: one register per stream
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const int ug = wave * UG + u;
                bo[u] = (unsigned)(((g * KC + ug) * KC * 64 + lane) * 4);
                if (!XIN) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[rt][u] = *reinterpret_cast<const f32x4*>(
                            gx + (((gx_rt0 + rt) * CT + g * KC + ug) * 64 + lane) * 4);
                } else {
                    const float bias = xin.bias[(g * KC + ug) * 16 + lr];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) acc[rt][u] = f32x4{bias, bias, bias, bias};
                }
            }
            if (XIN) {  // W_ih x_t: the same fragment scheme with A from the staged input tile
                for (int kx = 0; kx < xin.kin_chunks; ++kx) {
                    f32x4 bx[UG];
#pragma unroll
                    for (int u = 0; u < UG; ++u)
                        bx[u] = *reinterpret_cast<const f32x4*>(
                            xin.wih_p + (((long)(g * KC + wave * UG + u) * xin.kin_chunks + kx) * 64 + lane) * 4);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(xt + (rt * 16 + lr) * XS + kx * 16 + 4 * lq);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int u = 0; u < UG; ++u) acc[rt][u] = mfma16(a[j], bx[u][j], acc[rt][u]);
                    }
                }
            }
            if (t > 0) {  // h_{-1} = 0
                f32x4 bn[UG];
#pragma unroll
                for (int u = 0; u < UG; ++u) bn[u] = *reinterpret_cast<const f32x4*>(whh_p + bo[u]);
#pragma unroll UNR
                for (int kc = 0; kc < KC; ++kc) {
                    f32x4 bc[UG];
#pragma unroll
                    for (int u = 0; u < UG; ++u) bc[u] = bn[u];
                    if (kc + 1 < KC) {
#pragma unroll
                        for (int u = 0; u < UG; ++u)
                            bn[u] = *reinterpret_cast<const f32x4*>(whh_p + (bo[u] + (unsigned)(kc + 1) * 256u));
                    }
                    const float* ap = hl + lr * HS + kc * 16 + 4 * lq;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const f32x4 a = *reinterpret_cast<const f32x4*>(ap + rt * 16 * HS);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int u = 0; u < UG; ++u) acc[rt][u] = mfma16(a[j], bc[u][j], acc[rt][u]);
                    }
                }
            }
            // the branch on the (uniform) pass sits OUTSIDE the unrolled element loops, and c / the temporary are
            // scalar arrays rather than 4-vectors: written per element on vectors, hipcc emits a four-way scalar
            // branch tree and register-tuple copies around every single value
#define FSN_REC_EPILOGUE(VAR, EXPR)                                                                   \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                                 \
    _Pragma("unroll") for (int u = 0; u < UG; ++u)                                                    \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                   \
        VAR[rt][u][i] = EXPR;                                                                         \
        asm volatile("" : "+v"(VAR[rt][u][i])); /* computed HERE: not sunk towards its use two passes later */ \
    }
            if (pass == 0) {
                FSN_REC_EPILOGUE(cst, sigmoid_fast(acc[rt][u][i]) * cst[rt][u][i])
            } else if (pass == 1) {
                FSN_REC_EPILOGUE(tmp, sigmoid_fast(acc[rt][u][i]))
            } else if (pass == 2) {
                FSN_REC_EPILOGUE(cst, cst[rt][u][i] + tmp[rt][u][i] * tanh_fast(acc[rt][u][i]))
            } else {
                FSN_REC_EPILOGUE(tmp, sigmoid_fast(acc[rt][u][i]) * tanh_fast(cst[rt][u][i]))
            }
#undef FSN_REC_EPILOGUE
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();  // every wave has finished reading h_{t-1}
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int u = 0; u < UG; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    hl[(rt * 16 + 4 * lq + i) * HS + (wave * UG + u) * 16 + lr] = tmp[rt][u][i];
        __syncthreads();  // h_t complete in LDS
        if (fuse_fc) {
            // output layer on the spot: 4 threads per (row, output), a quarter of K each, joined by two
            // lane shuffles; frame t - la of the mask (the first la steps are the look-ahead warm-up)
            const int tid = threadIdx.x;
            if (tid < ROWS * 8) {
                const int part = tid & 3, c = (tid >> 2) & 1, row = tid >> 3;
                const float* hp = hl + row * HS + part * (H / 4);
                const float* wp = wl + c * H + part * (H / 4);
                float a0 = 0.f, a1 = 0.f;
#pragma unroll 2  // deeper unrolling costs the registers the left-over step kernels need beside this one
                for (int k = 0; k < H / 4; k += 8) {
                    const f32x4 h0 = *reinterpret_cast<const f32x4*>(hp + k), w0 = *reinterpret_cast<const f32x4*>(wp + k);
                    const f32x4 h1 = *reinterpret_cast<const f32x4*>(hp + k + 4),
                                w1 = *reinterpret_cast<const f32x4*>(wp + k + 4);
                    a0 = fmaf(h0[0], w0[0], a0);
                    a0 = fmaf(h0[1], w0[1], a0);
                    a0 = fmaf(h0[2], w0[2], a0);
                    a0 = fmaf(h0[3], w0[3], a0);
                    a1 = fmaf(h1[0], w1[0], a1);
                    a1 = fmaf(h1[1], w1[1], a1);
                    a1 = fmaf(h1[2], w1[2], a1);
                    a1 = fmaf(h1[3], w1[3], a1);
                }
                float v = a0 + a1;
                v += __shfl_xor(v, 1, 64);
                v += __shfl_xor(v, 2, 64);
                const long n = n0 + row;
                if (part == 0 && t >= fc.la && n < fc.N) {
                    const long ng = n + fc.row0;
                    const int b = (int)(ng / fc.F), f = (int)(ng % fc.F);
                    (c ? fc.crm_i : fc.crm_r)[((long)b * fc.T + (t - fc.la)) * fc.FP + f] = v + fc.bias[c];
                }
            }
        } else {
            // stream h_t out as whole rows: hseq[t][n0 + row][0..H)
            float* dst = hseq + ((long)t * Npad + n0) * H;
            for (int i = threadIdx.x; i < ROWS * (H / 4); i += NW * 64) {
                const int row = i / (H / 4), c4 = i % (H / 4);
                *reinterpret_cast<f32x4*>(dst + (long)row * H + c4 * 4) =
                    *reinterpret_cast<const f32x4*>(hl + row * HS + c4 * 4);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Small-N variant (RT <= 2, i.e. fewer row tiles than ~2 per CU: small batches, per-rank shards of a
// strong-scaled batch, single utterances).  With 16-32 rows per workgroup a K chunk is only 8-16 MFMAs
// per gate, far shorter than the L2 latency of its B fragments, and lstm_rec_kernel's four sequential
// gate passes leave the step latency-bound (52 us per step at RT = 1, 10 us of MFMA).  Registers are
// plentiful here, so all four gates accumulate in ONE pass: a quarter of the dependent chunk
// iterations, four times the MFMA work between two waits, no temporaries in the cell update.
template <int H, int RT, int UG, bool XIN>
__global__ __launch_bounds__((H / (16 * UG)) * 64) void lstm_rec_small_kernel(const float* __restrict__ gx,
                                                                              const FsnSbInput xin,
                                                                              const float* __restrict__ whh_p,
                                                                              float* __restrict__ hseq, int Tp,
                                                                              int Npad, const FsnRecFc) {
    constexpr int NW = H / (16 * UG);
    constexpr int KC = H / 16;
    constexpr int CT = 4 * KC;
    constexpr int HS = H + 4;
    constexpr int ROWS = RT * 16;
    extern __shared__ __attribute__((aligned(16))) float hl[];
    const int XS = XIN ? 16 * xin.kin_chunks + 4 : 0;
    float* xl = hl + ROWS * HS;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const long n0 = (long)blockIdx.x * ROWS;

    f32x4 cst[RT][UG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int u = 0; u < UG; ++u) cst[rt][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < ROWS * HS; i += NW * 64) hl[i] = 0.f;
    if (XIN) stage_sb_input<NW * 64>(xin, xl, XS, n0, ROWS, 0);
    __syncthreads();

    const float* bp[4][UG];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int u = 0; u < UG; ++u) bp[g][u] = whh_p + ((long)(g * KC + wave * UG + u) * KC * 64 + lane) * 4;

    for (int t = 0; t < Tp; ++t) {
        const long gx_rt0 = ((long)t * Npad + n0) >> 4;
        if (XIN && t + 1 < Tp) stage_sb_input<NW * 64>(xin, xl + ((t + 1) & 1) * ROWS * XS, XS, n0, ROWS, t + 1);
        const float* xt = xl + (t & 1) * ROWS * XS;
        f32x4 acc[4][RT][UG];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                const int ug = wave * UG + u;
                if (!XIN) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[g][rt][u] = *reinterpret_cast<const f32x4*>(
                            gx + (((gx_rt0 + rt) * CT + g * KC + ug) * 64 + lane) * 4);
                } else {
                    const float bias = xin.bias[(g * KC + ug) * 16 + lr];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) acc[g][rt][u] = f32x4{bias, bias, bias, bias};
                }
            }
        if (XIN) {
            for (int kx = 0; kx < xin.kin_chunks; ++kx) {
                f32x4 a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    a[rt] = *reinterpret_cast<const f32x4*>(xt + (rt * 16 + lr) * XS + kx * 16 + 4 * lq);
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int u = 0; u < UG; ++u) {
                        const f32x4 bx = *reinterpret_cast<const f32x4*>(
                            xin.wih_p + (((long)(g * KC + wave * UG + u) * xin.kin_chunks + kx) * 64 + lane) * 4);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) acc[g][rt][u] = mfma16(a[rt][j], bx[j], acc[g][rt][u]);
                    }
            }
        }
        if (t > 0) {  // h_{-1} = 0
            f32x4 bn[4][UG];
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int u = 0; u < UG; ++u) bn[g][u] = *reinterpret_cast<const f32x4*>(bp[g][u]);
#pragma unroll 1
            for (int kc = 0; kc < KC; ++kc) {
                f32x4 bc[4][UG], a[RT];
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int u = 0; u < UG; ++u) bc[g][u] = bn[g][u];
                const int kn = kc + 1 < KC ? kc + 1 : kc;  // clamped: branch-free, counted waits
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int u = 0; u < UG; ++u)
                        bn[g][u] = *reinterpret_cast<const f32x4*>(bp[g][u] + (long)kn * 256);
                const float* ap = hl + lr * HS + kc * 16 + 4 * lq;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(ap + rt * 16 * HS);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int u = 0; u < UG; ++u)
                                acc[g][rt][u] = mfma16(a[rt][j], bc[g][u][j], acc[g][rt][u]);
            }
        }
        f32x4 hv[RT][UG];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int u = 0; u < UG; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float ig = sigmoid_fast(acc[0][rt][u][i]), fg = sigmoid_fast(acc[1][rt][u][i]);
                    const float gg = tanh_fast(acc[2][rt][u][i]), og = sigmoid_fast(acc[3][rt][u][i]);
                    const float cn = fg * cst[rt][u][i] + ig * gg;
                    cst[rt][u][i] = cn;
                    hv[rt][u][i] = og * tanh_fast(cn);
                }
        __syncthreads();
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int u = 0; u < UG; ++u)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    hl[(rt * 16 + 4 * lq + i) * HS + (wave * UG + u) * 16 + lr] = hv[rt][u][i];
        __syncthreads();
        float* dst = hseq + ((long)t * Npad + n0) * H;
        for (int i = threadIdx.x; i < ROWS * (H / 4); i += NW * 64) {
            const int row = i / (H / 4), c4 = i % (H / 4);
            *reinterpret_cast<f32x4*>(dst + (long)row * H + c4 * 4) =
                *reinterpret_cast<const f32x4*>(hl + row * HS + c4 * 4);
        }
    }
}

template <int H, int RT, bool XIN, int UG = 2>
int launch_rec(const float* gx, const FsnSbInput* xin, const float* whh_p, float* hseq, int Tp, int Npad,
               int main_wgs, hipStream_t s, const FsnRecFc* fc = nullptr) {
    constexpr int NW = H / (16 * UG);
    size_t lds = (size_t)RT * 16 * (H + 4) * sizeof(float);
    if (XIN) lds += (size_t)2 * RT * 16 * (16 * xin->kin_chunks + 4) * sizeof(float);
    const bool fuse = fc && fc->w_p;
    if (fuse && (XIN || RT <= 1)) {
        fsn_set_error("lstm_rec: the output layer can only be fused into the 4-pass kernel without input staging");
        return FSN_ERR_ARG;
    }
    if (fuse) lds += (size_t)2 * H * sizeof(float);
    // RT == 1 (fewer row tiles than CUs): the one-pass-all-gates variant, ~10 % faster there (8.8 vs
    // 10.0 ms per layer; a 16-row workgroup still owes 9216 MFMAs = 31 us per step, so small batches
    // stay bound by one tile per CU until the hidden units of a tile are split across CUs).  At
    // RT = 2 it spills and loses.
    void (*kern)(const float*, const FsnSbInput, const float*, float*, int, int, const FsnRecFc) =
        lstm_rec_kernel<H, RT, UG, XIN>;
    if constexpr (RT <= 1) kern = lstm_rec_small_kernel<H, RT, UG, XIN>;
    if (lds > 160 * 1024) {
        fsn_set_error("lstm_rec: cannot reserve %zu bytes of LDS", lds);
        return FSN_ERR_LAUNCH;
    }
    FSN_TRY_RESERVE_LDS("lstm_rec", kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)main_wgs), dim3(NW * 64), lds, s, gx, XIN ? *xin : FsnSbInput{}, whh_p,
                       hseq, Tp, Npad, fuse ? *fc : FsnRecFc{});
    return fsn_check_launch("lstm_rec_kernel");
}

}  // namespace

// How the N sub-band sequences are laid out on the chip.  One workgroup per CU (LDS-bound), RT
// 16-row tiles per workgroup, so a single launch is worth max-RT tile-times and
// N = B F = 64 * 257 = 1028 tiles is the worst case for 256 CUs: 4.016 tiles per CU.  Instead of
// paying a fifth tile on every CU (206 workgroups x 5 tiles, 50 CUs idle), the main kernel takes
// floor(tiles / CUs) tiles per CU on all CUs and the few left-over tiles (4 of 1028) run
// concurrently as per-step lstm_step_kernel launches on an auxiliary stream: those small workgroups
// fit next to the resident main workgroup (40 VGPRs, 12 KB LDS) and add 0.4 % of MFMA work.
FsnRecPlan fsn_lstm_rec_plan(int N, int H) {
    (void)H;
    const int rt_max = 5;    // LDS: 16 RT (H + 4) floats = 124 KB at H = 384
    const int left_max = 16;  // tiles worth handing to the step kernels
    const int cus = plan_cus();
    FsnRecPlan p;
    p.tiles = (N + 15) / 16;
    p.npad = p.tiles * 16;
    // Few rows: one 16-row tile per CU leaves most CUs idle and makes every busy one stream the whole
    // W_hh (2.4 MB) from L2 per step (~31 us/step, measured); below this many tiles the per-step
    // kernels, which spread a step over (H/16) x tiles workgroups, are faster (batch 1: 21.4 -> 8.4 ms
    // for 3 s of audio; break-even at ~160 tiles = batch 10).
    constexpr int step_below = 160;
    if (p.tiles < step_below) {
        p.rt = 1;
        p.main_wgs = 0;
        p.left_tiles = p.tiles;
        return p;
    }
    if (p.tiles <= cus) {
        p.rt = 1;
        p.main_wgs = p.tiles;
        p.left_tiles = 0;
        return p;
    }
    const int rt_floor = p.tiles / cus < rt_max ? p.tiles / cus : rt_max;
    const int left = p.tiles - cus * rt_floor;
    if (left <= left_max) {
        p.rt = rt_floor;
        p.main_wgs = cus;
        p.left_tiles = left;
        return p;
    }
    // general case: whole rounds, pick the RT with the smallest makespan (rounds x RT) ...
    int best = 1;
    long best_cost = -1;
    for (int rt = 1; rt <= rt_max; ++rt) {
        const long wgs = (p.tiles + rt - 1) / rt;
        const long rounds = (wgs + cus - 1) / cus;
        const long cost = rounds * rt * 64 + rounds;
        if (best_cost < 0 || cost < best_cost || (cost == best_cost && rt > best)) {
            best = rt;
            best_cost = cost;
        }
    }
    // ... unless FULL rounds of some RT leave only a few tiles for the step kernels: 128 utterances are 2056 tiles = two
    // full rounds at 4 tiles per workgroup + 8 left over, where whole rounds would take three of RT = 3 (188 ms against
    // 2 x 84); 96 utterances two rounds of 3 + 6 tiles instead of three
    for (int rt = rt_max; rt >= 1; --rt) {
        const long rounds = p.tiles / ((long)cus * rt);
        if (rounds < 1) continue;
        const long left2 = p.tiles - rounds * cus * rt;
        const long cost = rounds * rt * 64 + rounds;
        if (left2 <= left_max && cost < best_cost) {
            p.rt = rt;
            p.main_wgs = (int)(rounds * cus);
            p.left_tiles = (int)left2;
            return p;
        }
    }
    p.rt = best;
    p.main_wgs = (p.tiles + best - 1) / best;
    p.left_tiles = 0;
    p.npad = p.main_wgs * best * 16;
    p.tiles = p.npad / 16;
    return p;
}

bool fsn_lstm_rec_can_fuse_fc(int RT, bool xin) { return !xin && RT >= 2; }

int fsn_launch_lstm_rec(const float* gx, const FsnSbInput* xin, const float* whh_p, float* hseq, int Tp, int Npad,
                        int H, int RT, int main_wgs, hipStream_t s, const FsnRecFc* fc) {
    fsn_trace(FSN_TR_LSTM_REC);
#define FSN_REC_CASE(HH, R)                                                                             \
    if (H == HH && RT == R)                                                                              \
        return xin ? launch_rec<HH, R, true>(gx, xin, whh_p, hseq, Tp, Npad, main_wgs, s, fc)            \
                   : launch_rec<HH, R, false>(gx, xin, whh_p, hseq, Tp, Npad, main_wgs, s, fc);
    FSN_REC_CASE(384, 1)
    FSN_REC_CASE(384, 2)
    FSN_REC_CASE(384, 3)
    FSN_REC_CASE(384, 4)
    FSN_REC_CASE(384, 5)
#undef FSN_REC_CASE
    fsn_set_error("lstm_rec: unsupported hidden size %d / row tiles %d (built for H = 384)", H, RT);
    return FSN_ERR_ARG;
}
