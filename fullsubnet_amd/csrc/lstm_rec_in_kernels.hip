// Persistent many-row LSTM / GRU layer with a NARROW INPUT PROJECTION INSIDE (K = 16 or 32): the first layer of a stack.
// See lstm_rec_kernels.hip for the recurrence and the regime (a workgroup owns 16 RT rows for the whole utterance, h in
// LDS, c in registers); this kernel adds the weight-fragment ring and the deferred input staging described at the kernel.
//
// Which plan reaches which instantiation (H = 384, two unit groups per wave, RT = 2 - 4 row tiles per workgroup - what
// fsn_lstm_rec_in_supported admits; everything else stays on lstm_rec_kernel<.., XIN = true>):
//   lstm_rec_in_kernel<384, RT, 2, GRU = false, KX = 2, ROWSIN = false>  the sub-band model's first layer (fsn_api_fullsubnet.hip:
//       run_recurrence with the gathered FsnSbInput, 2 nb + 2 padded to 32 columns, fp32 arithmetic) - BASELINE config 2
//   lstm_rec_in_kernel<384, RT, 2, false, KX = 1 | 2, ROWSIN = true>     a stand-alone layer with at most 32 input columns
//       (fsn_lstm_layer_forward in inference mode, fsn_api_layers.hip: Fast FullSubNet's bottleneck, a composed FullSubNet's
//       first sub-band layer), with or without left-over tiles beside it
//   lstm_rec_in_kernel<384, RT, 2, GRU = true, KX = 1 | 2, ROWSIN = true>  the same for nn.GRU (fsn_gru_layer_forward,
//       fsn_api_gru.hip), weights expanded to the four-gate cell of lstm_cell.h
#include "lstm_cell.h"
#include "persist_sync.h"

namespace {

// One frame of the sub-band model input for the persistent first-layer kernel, in two halves so that the memory
// latency is never exposed: `issue` requests ALL of a thread's elements (and their divisors) at once, `commit`
// divides and writes them to the LDS tile a gate pass later.  No 64-bit division per element: the rows of a
// workgroup are consecutive, so (b, f) of a row follow from (b0, f0) of the workgroup's first row by a carry.
// Same operands, same IEEE division as fsn_sb_input_value: bit-identical values.
// ROWSIN: the plain row-major form of the layer input (FsnSbInput::x_rows, COLS = 16 or 32 columns, zero padded in
// memory) - requested the same way, nothing to divide.
template <int NTHREADS, int ROWS, int EPT, int COLS = 32, bool ROWSIN = false>
struct SbStage {
    static constexpr int LOGC = COLS == 32 ? 5 : 4;
    static_assert(COLS == 32 || COLS == 16, "one or two K chunks");
    float raw[EPT], den[ROWSIN ? 1 : EPT];
    __device__ __forceinline__ void issue(const FsnSbInput& x, long n0, int b0, int f0, int t) {
        // the element indices do not depend on the step; left visible, the optimiser computes them once and keeps
        // a dozen registers live through the whole kernel
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        if constexpr (ROWSIN) {
            const float* frame = x.x_rows + ((long)t * x.x_step + n0) * x.x_ld;  // wave-uniform
#pragma unroll
            for (int e = 0; e < EPT; ++e) {
                const int i = tid + e * NTHREADS;
                const int row = i >> LOGC, c = i & (COLS - 1);
                const bool ok = i < ROWS * COLS && n0 + row < x.N;
                raw[e] = frame[ok ? (long)row * x.x_ld + c : 0];  // branch-free; replaced by zero in commit()
            }
            return;
        }
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NTHREADS;
            const int row = i >> LOGC, c = i & (COLS - 1);  // 32 input columns (two K chunks)
            const long n = n0 + row;             // local row (validity, per-row divisors); (b, f) are global
            const bool ok = i < ROWS * COLS && n < x.N && c <= 2 * x.nb + 1;
            const unsigned fr = (unsigned)(f0 + row), q = fr / (unsigned)x.F;  // the carry: rows are consecutive
            const int b = b0 + (int)q, f = (int)(fr - q * (unsigned)x.F);
            const long fo = ((long)b * x.Tp + t) * x.FP;
            int j = f + c - x.nb;
            j = j < 0 ? -j : j;
            j = j >= x.F ? 2 * (x.F - 1) - j : j;
            const float* src = c <= 2 * x.nb ? x.mag + fo + j : x.fb_out + fo + f;
            // branch-free: an element that is not there reads element 0 and is replaced by zero in commit()
            raw[e] = *(ok ? src : x.mag);
            den[e] = x.den[ok ? (x.den_mode ? (long)t * x.den_stride + (n + x.row0) : (long)b) : 0];
        }
    }
    __device__ __forceinline__ void commit(const FsnSbInput& x, float* xl, int xs, long n0) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int i = tid + e * NTHREADS;
            const int row = i >> LOGC, c = i & (COLS - 1);
            if constexpr (ROWSIN) {
                if (i < ROWS * COLS) xl[row * xs + c] = n0 + row < x.N ? raw[e] : 0.f;
            } else {
                const bool ok = n0 + row < x.N && c <= 2 * x.nb + 1;
                if (i < ROWS * COLS) xl[row * xs + c] = ok ? raw[e] / den[e] : 0.f;
            }
        }
    }
};

// First sub-band layer, persistent (the successor of lstm_rec_kernel<.., XIN = true> for the 32-column sub-band
// input): gates = b + x_t W_ih^T (K = 32, x_t = freq_unfold ++ fb_output, normalised: fullsubnet/model.py:98-111,
// gathered into a double-buffered LDS tile) + h_{t-1} W_hh^T.  Against its predecessor:
//   - weight fragments travel in a two-deep buffer-load ring that runs through the x chunks, the h chunks, and on
//     into the next pass / step (a gate pass never starts cold; no per-load address arithmetic);
//   - the next frame's gather is requested at the start of a step and written to LDS one gate pass later, into
//     registers that are dead during that pass (its latency used to be exposed on all 12 waves once per step);
//   - the two barriers of a step only order LDS traffic;
//   - the bias of the next pass is requested a pass ahead.
// W_hh must follow W_ih in one packed buffer (element offset whh_off).  hseq [Tp][Npad][H] receives h_t.
// KX: K chunks of the layer input (2: the sub-band model's 32 columns; 1 or 2 with ROWSIN, the plain row-major input of
// any stacked LSTM's first layer - Fast FullSubNet's bottleneck is 16 columns wide: fast_fullsubnet/model.py:66-74).  With
// ONE x chunk a pass walks an odd number of K chunks, so the two weight-fragment registers sets swap roles from pass to pass
// (four passes per step: every step starts the same way).
#ifndef FSN_REC_IN_VCAP
#define FSN_REC_IN_VCAP 76  // x 2 = 152 registers: three waves per SIMD + a step workgroup beside them (tests/test_host_cpu.py)
#endif
template <int H, int RT, int UG, bool GRU, int KX, bool ROWSIN>
__global__ __launch_bounds__((H / (16 * UG)) * 64) __attribute__((amdgpu_num_vgpr(FSN_REC_IN_VCAP))) void lstm_rec_in_kernel(
    const FsnSbInput xin, const float* __restrict__ w_p, unsigned whh_off, float* __restrict__ hseq, int Tp, int Npad) {
    constexpr int NW = H / (16 * UG);
    constexpr int KC = H / 16;
    static_assert(KX == 2 || (KX == 1 && ROWSIN), "the gathered sub-band input is two chunks wide");
    constexpr int HS = H + 4;
    constexpr int XS = 16 * KX + 4;  // row stride of the x tile
    constexpr int ROWS = RT * 16;
    constexpr int EPT = (ROWS * 16 * KX + NW * 64 - 1) / (NW * 64);
    extern __shared__ __attribute__((aligned(16))) float hl[];  // [ROWS][HS] | xl [2][ROWS][XS]
    float* xl = hl + ROWS * HS;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const long n0 = (long)blockIdx.x * ROWS;
    const int sb_b0 = ROWSIN ? 0 : (int)((n0 + xin.row0) / xin.F);  // (b, f) of the workgroup's first row, once
    const int sb_f0 = ROWSIN ? 0 : (int)((n0 + xin.row0) - (long)sb_b0 * xin.F);

    // KOPT (see lstm_rec_x_kernel): the recurrent product's K loop keeps two LDS base addresses for row tiles 0-1 / 2-3 and
    // advances them once per six chunks
    static_assert(RT >= 2 && RT <= 4 && KC % 6 == 0, "the recurrent K loop is written for 2 - 4 row tiles and blocks of six chunks");
    // GRU: the GRU as a four-gate cell (lstm_cell.h).  Gate non-linearities on pairs (PK: v_pk_*_f32, see sigmoid_fast2)
    f32x4 cst[RT][UG], tmp[RT][UG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int u = 0; u < UG; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) cst[rt][u][i] = 0.f;
    for (int i = threadIdx.x; i < ROWS * HS; i += NW * 64) hl[i] = 0.f;
    SbStage<NW * 64, ROWS, EPT, 16 * KX, ROWSIN> stage;
    stage.issue(xin, n0, sb_b0, sb_f0, 0);
    stage.commit(xin, xl, XS, n0);
    __syncthreads();

    const __amdgpu_buffer_rsrc_t wrsrc = fsn_buffer_rsrc(w_p);
    const unsigned lane16 = (unsigned)lane * 16u;
    auto wload = [&](unsigned ofs) { return fsn_buffer_load<f32x4>(wrsrc, lane16, ofs * 4u); };
    auto wxofs = [&](int g, int u) { return (unsigned)((g * KC + wave * UG + u) * KX) * 256u; };
    auto whofs = [&](int g, int u) { return whh_off + (unsigned)((g * KC + wave * UG + u) * KC) * 256u; };
    f32x4 b0[UG], b1[UG];
    float bias_n[UG];
    {
        int g0 = 1;
        asm volatile("" : "+s"(g0));
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            b0[u] = wload(wxofs(g0, u));
            bias_n[u] = xin.bias[(g0 * KC + wave * UG + u) * 16 + lr];
        }
    }
    auto mma = [&](f32x4 (&acc)[RT][UG], const float* a, int a_rt_stride, const f32x4 (&b)[UG]) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const f32x4 av = *reinterpret_cast<const f32x4*>(a + rt * a_rt_stride);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int u = 0; u < UG; ++u) acc[rt][u] = mfma16(av[jj], b[u][jj], acc[rt][u]);
        }
    };
    for (int t = 0; t < Tp; ++t) {
        // frame t + 1: requested now, written to the other x buffer after the first gate pass (that buffer was last
        // read in step t - 1 and is first read after the two barriers that end this step)
        const bool more = t + 1 < Tp;
        if (more) stage.issue(xin, n0, sb_b0, sb_f0, t + 1);
        const float* xa = xl + (t & 1) * ROWS * XS + lr * XS + 4 * lq;
        const float* ha = hl + lr * HS + 4 * lq;
        // gate order of evaluation: f (1), i (0), g (2), o (3)
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            __builtin_amdgcn_sched_barrier(0);
            int g = pass == 0 ? 1 : (pass == 1 ? 0 : pass);
            int gn = pass == 0 ? 0 : (pass == 1 ? 2 : (pass == 2 ? 3 : 1));  // the gate after this one
            asm volatile("" : "+s"(g));  // opaque: see lstm_rec_kernel
            asm volatile("" : "+s"(gn));
            const bool hpart = t > 0 && !(GRU && pass == 2);  // h_{-1} = 0; the GRU's nx gate has no recurrent part
            // ... and its nh gate no input part: skipped from step 1 on in the two-chunk form (with ONE x chunk the skipped pass
            // would change the parity of the fragment sets' roles; the zero block is multiplied there)
            const bool xpart = !(GRU && KX == 2 && pass == 1 && t > 0);
            const bool next_h_first = GRU && KX == 2 && pass == 0 && t > 0;  // the next pass opens with its recurrent product
            f32x4 acc[RT][UG];
            // B0: the fragments this pass starts with, B1: the other set; C0 / C1: the same for the recurrent product
            const bool SW = KX == 1 && (pass & 1);  // (a constant once the passes are unrolled)
            f32x4 (&B0)[UG] = SW ? b1 : b0;
            f32x4 (&B1)[UG] = SW ? b0 : b1;
            f32x4 (&C0)[UG] = KX == 1 ? B1 : B0;
            f32x4 (&C1)[UG] = KX == 1 ? B0 : B1;
            unsigned wx[UG], wh[UG], wxn[UG];
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                wx[u] = wxofs(g, u);
                wh[u] = whofs(g, u);
                wxn[u] = next_h_first ? whofs(gn, u) : wxofs(gn, u);
                const float b = bias_n[u];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][u] = f32x4{b, b, b, b};
                bias_n[u] = xin.bias[(gn * KC + wave * UG + u) * 16 + lr];  // a pass ahead
            }
            // ---- x_t W_ih^T: two chunks (or one) --------------------------------------------------
            if constexpr (KX == 2) {
              if (xpart) {
#pragma unroll
                for (int u = 0; u < UG; ++u) B1[u] = wload(wx[u] + 256u);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc, xa, 16 * XS, B0);
#pragma unroll
                for (int u = 0; u < UG; ++u) B0[u] = wload(hpart ? wh[u] : wxn[u]);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc, xa + 16, 16 * XS, B1);
              }
            } else {
#pragma unroll
                for (int u = 0; u < UG; ++u) B1[u] = wload(hpart ? wh[u] : wxn[u]);
                __builtin_amdgcn_sched_barrier(0);
                mma(acc, xa, 16 * XS, B0);
            }
            __builtin_amdgcn_sched_barrier(0);
            // ---- h_{t-1} W_hh^T (h_{-1} = 0) -------------------------------------------------------
            if (hpart) {
                typedef const __attribute__((address_space(3))) float* lds_cptr;
                unsigned hb01 = (unsigned)(size_t)(lds_cptr)(hl + lr * HS + 4 * lq), hb23 = hb01 + 32u * HS * 4u;
                asm volatile("" : "+v"(hb01));
                asm volatile("" : "+v"(hb23));
                lds_cptr ha01 = (lds_cptr)(size_t)hb01;
                lds_cptr ha23 = (lds_cptr)(size_t)hb23;
                // APF: the first row tile's A fragment of block k + 1 is requested right behind block k's first-tile MFMAs
                // (into the registers they have just read) instead of at the head of block k + 1, where the block's first
                // MFMA waits for it; tiles 1 - 3 have the MFMAs before them to land
                auto lda = [&](int rt, int kofs) {
                    return *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>((rt < 2 ? ha01 : ha23) + (rt & 1) * 16 * HS + kofs);
                };
                f32x4 apre = lda(0, 0);
                auto blk = [&](int kofs, const f32x4 (&b)[UG], bool more) {
                    f32x4 av[RT];
#pragma unroll
                    for (int rt = 1; rt < RT; ++rt) av[rt] = lda(rt, kofs);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                        for (int u = 0; u < UG; ++u) acc[0][u] = mfma16(apre[jj], b[u][jj], acc[0][u]);
                    __builtin_amdgcn_sched_barrier(0);
                    if (more) apre = lda(0, kofs + 16);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int rt = 1; rt < RT; ++rt)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                            for (int u = 0; u < UG; ++u) acc[rt][u] = mfma16(av[rt][jj], b[u][jj], acc[rt][u]);
                };
#pragma unroll 1
                for (int hs = 0; hs < KC / 6; ++hs) {
#pragma unroll
                    for (int kk = 0; kk < 6; kk += 2) {
                        const int kc = hs * 6 + kk;
#pragma unroll
                        for (int u = 0; u < UG; ++u) C1[u] = wload(wh[u] + (unsigned)(kc + 1) * 256u);
                        __builtin_amdgcn_sched_barrier(0);
                        blk(kk * 16, C0, true);
                        __builtin_amdgcn_sched_barrier(0);
                        const bool more_h = kc + 2 < KC;
#pragma unroll
                        for (int u = 0; u < UG; ++u) C0[u] = wload(more_h ? wh[u] + (unsigned)(kc + 2) * 256u : wxn[u]);
                        __builtin_amdgcn_sched_barrier(0);
                        blk((kk + 1) * 16, C1, more_h);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    ha01 += 6 * 16;
                    ha23 += 6 * 16;
                }
            }
            if constexpr (GRU) {  // cst = h_{t-1} (and h_t after the z pass); tmp: r, r * (W_hn h + b_hn), n
                if (pass == 0) {
                    FSN_CELL_PASS2(tmp, sigmoid_fast2(a))
                    if (more) stage.commit(xin, xl + ((t + 1) & 1) * ROWS * XS, XS, n0);
                } else if (pass == 1) {
                    FSN_CELL_PASS2(tmp, m * a)
                } else if (pass == 2) {
                    FSN_CELL_PASS2(tmp, tanh_fast2(a + m))
                } else {
                    FSN_CELL_PASS2(cst, m + sigmoid_fast2(a) * (c - m))
                }
            } else if (pass == 0) {
                FSN_CELL_PASS2(cst, sigmoid_fast2(a) * c)
                if (more) stage.commit(xin, xl + ((t + 1) & 1) * ROWS * XS, XS, n0);  // tmp's registers are free here
            } else if (pass == 1) {
                FSN_CELL_PASS2(tmp, sigmoid_fast2(a))
            } else if (pass == 2) {
                FSN_CELL_PASS2(cst, c + m * tanh_fast2(a))
            } else {
                FSN_CELL_PASS2(tmp, sigmoid_fast2(a) * tanh_fast2(c))
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // every wave has finished reading h_{t-1}
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        {
            unsigned hwb = (unsigned)((4 * lq) * HS + (wave * UG) * 16 + lr);
            asm volatile("" : "+v"(hwb));  // re-derived every step: see lstm_rec_x_kernel
            float* hw = hl + hwb;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int u = 0; u < UG; ++u)
#pragma unroll
                    for (int i = 0; i < 4; ++i) hw[(rt * 16 + i) * HS + u * 16] = GRU ? cst[rt][u][i] : tmp[rt][u][i];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();  // h_t complete in LDS
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        // stream h_t out as whole rows: hseq[t][n0 + row][0..H)
        float* dst = hseq + ((long)t * Npad + n0) * H;
        // (Round 5, measured and not kept: the gather's step-independent index arithmetic read back from an LDS table, and
        // these stores from one address pair per step - ~250 fewer vector instructions per wave and step, no change in
        // time: the step's ends wait on the barriers anyway.  Without the stores 0.1 ms, without the gather 0.2.)
        for (int i = threadIdx.x; i < ROWS * (H / 4); i += NW * 64) {
            const int row = i / (H / 4), c4 = i % (H / 4);
            const f32x4 v = *reinterpret_cast<const f32x4*>(hl + row * HS + c4 * 4);
            *reinterpret_cast<f32x4*>(dst + (long)row * H + c4 * 4) = v;
        }
    }
}

template <int H, int RT, int KX = 2, bool ROWSIN = false, int CELL = 0, int UG = 2>
int launch_rec_in(const FsnSbInput* xin, const float* whh_p, float* hseq, int Tp, int Npad, int main_wgs, hipStream_t s) {
    constexpr int NW = H / (16 * UG);
    const size_t lds = ((size_t)RT * 16 * (H + 4) + (size_t)2 * RT * 16 * (16 * KX + 4)) * sizeof(float);
    auto kern = lstm_rec_in_kernel<H, RT, UG, CELL != 0, KX, ROWSIN>;
    if (lds > 160 * 1024) {
        fsn_set_error("lstm_rec_in: cannot reserve %zu bytes of LDS", lds);
        return FSN_ERR_LAUNCH;
    }
    FSN_TRY_RESERVE_LDS("lstm_rec_in", kern, lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)main_wgs), dim3(NW * 64), lds, s, *xin, xin->wih_p,
                       (unsigned)(whh_p - xin->wih_p), hseq, Tp, Npad);
    return fsn_check_launch("lstm_rec_in_kernel");
}

}  // namespace

// First layer of a stack on lstm_rec_in_kernel: the 32-column gathered sub-band input (two K chunks) or a plain row-major
// input of one or two chunks, H = 384, 2 - 4 row tiles per workgroup, W_hh packed right behind W_ih.  Anything else stays
// on lstm_rec_kernel<.., XIN = true>.
bool fsn_lstm_rec_in_supported(const FsnSbInput* xin, const float* whh_p, int H, int RT) {
    const bool shape = xin && (xin->x_rows ? (xin->kin_chunks == 1 || xin->kin_chunks == 2) && xin->x_ld >= 16 * xin->kin_chunks
                                           : xin->kin_chunks == 2);
    return shape && H == 384 && RT >= 2 && RT <= 4 && whh_p > xin->wih_p && whh_p - xin->wih_p < 0x3fffffffL;
}

int fsn_launch_lstm_rec_in(const FsnSbInput* xin, const float* whh_p, float* hseq, int Tp, int Npad, int H, int RT,
                           int main_wgs, hipStream_t s, int cell) {
    fsn_trace(FSN_TR_LSTM_REC_IN);
    if (!fsn_lstm_rec_in_supported(xin, whh_p, H, RT) || (cell && !xin->x_rows)) {
        fsn_set_error("lstm_rec_in: unsupported configuration");
        return FSN_ERR_ARG;
    }
    if (cell) {  // GRU (lstm_cell.h): the row-major input forms, weights expanded by fsn_launch_gru_expand4(.., order 1)
#define FSN_REC_IN_GRU(R)                                                                                             \
    if (RT == R)                                                                                                      \
        return xin->kin_chunks == 2 ? launch_rec_in<384, R, 2, true, 1>(xin, whh_p, hseq, Tp, Npad, main_wgs, s)      \
                                    : launch_rec_in<384, R, 1, true, 1>(xin, whh_p, hseq, Tp, Npad, main_wgs, s);
        FSN_REC_IN_GRU(2)
        FSN_REC_IN_GRU(3)
        FSN_REC_IN_GRU(4)
#undef FSN_REC_IN_GRU
    }
#define FSN_REC_IN_CASE(R)                                                                                         \
    if (RT == R) {                                                                                                 \
        if (!xin->x_rows) return launch_rec_in<384, R>(xin, whh_p, hseq, Tp, Npad, main_wgs, s);                   \
        if (xin->kin_chunks == 2) return launch_rec_in<384, R, 2, true>(xin, whh_p, hseq, Tp, Npad, main_wgs, s);  \
        return launch_rec_in<384, R, 1, true>(xin, whh_p, hseq, Tp, Npad, main_wgs, s);                            \
    }
    FSN_REC_IN_CASE(2)
    FSN_REC_IN_CASE(3)
    FSN_REC_IN_CASE(4)
#undef FSN_REC_IN_CASE
    fsn_set_error("lstm_rec_in: unsupported row tiles %d", RT);
    return FSN_ERR_ARG;
}
