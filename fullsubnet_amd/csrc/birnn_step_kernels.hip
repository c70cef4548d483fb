// Bidirectional nn.LSTM / nn.GRU layer (audio_zen/model/module/sequence_model.py:52-66 with bidirectional = True) for FEW
// rows, one launch per time step for BOTH directions.  The two directions of a layer are independent recurrences over the
// same rows: blockIdx.z picks one of two jobs from a by-value job table (the shape of lstm_step2_kernel, lstm_step_kernels.hip),
// the forward direction at frame s and the reverse one at frame T - 1 - s, so a layer over T frames is T dependent launches
// instead of 2 T, with no time flips and no concatenation: both jobs read their tiles of ONE fragment-ordered input
// projection (2 g H columns) and write their column half of ONE hidden sequence [T][N][ldh].
// A workgroup owns RTS 16-row tiles x one 16-unit group x the g gates of its direction; its 4 waves split K four ways and the
// partials are reduced through LDS in a fixed order; wave w < RTS then finishes row tile w (lstm_step_kernel / gru_step_kernel).
// A job's arithmetic does not depend on its slot: the same code on the same values, whichever direction it is.
// BPTT is the mirror image (bptt_step_kernel / gru_bptt_step_kernel): the forward direction walks T - 1 .. 0 while the reverse
// one walks 0 .. T - 1.
#include "fsn_birnn.h"

namespace {

struct BiStepJob {
    const float* whh_p;
    const float* h_prev;  // this direction's columns of the hidden sequence at its previous frame (row stride ldh)
    float* h_out;         // ... at its own frame
    const float* c_prev;  // LSTM [N][H]
    float* c_out;
    float* gates_out;     // training: [N][4H] of this frame, else NULL
    const float* b_hn;    // GRU [H]
    long gx_tile0;        // projection tile of (this frame, row tile 0, this direction's column tile 0)
};
struct BiStepJobs {
    BiStepJob j[2];
};

// gx_ct: column tiles of a row tile of the projection (both directions).  first: step 0 of BOTH directions (h = c = 0).
template <int RTS>
__global__ __launch_bounds__(256) void bilstm_step_kernel(const float* __restrict__ gx, const BiStepJobs jobs, int gx_ct,
                                                          int row_tiles, int H, long ldh, int first) {
    const BiStepJob job = jobs.j[blockIdx.z];  // one uniform kernarg fetch
    __shared__ f32x4 red[4][RTS][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.x, rtile0 = blockIdx.y * RTS;
    const int KC = H >> 4;
    f32x4 acc[RTS][4];
#pragma unroll
    for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[rt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // what the finishing wave's epilogue reads is requested before the K loop (cold lines)
    const int ftile = rtile0 + wave < row_tiles ? rtile0 + wave : row_tiles - 1;
    f32x4 addv[4];
    float c_old[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        addv[g] = *reinterpret_cast<const f32x4*>(gx + ((job.gx_tile0 + (long)ftile * gx_ct + g * KC + ug) * 64 + lane) * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) c_old[i] = first ? 0.f : job.c_prev[((long)ftile * 16 + 4 * lq + i) * H + ug * 16 + lr];
    if (!first) {
        const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
        const float* ap[RTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
            int rtile = rtile0 + rt;
            rtile = rtile < row_tiles ? rtile : row_tiles - 1;
            ap[rt] = job.h_prev + ((long)rtile * 16 + lr) * ldh + 4 * lq;
        }
#pragma unroll 2
        for (int kc = kc0; kc < kc1; ++kc) {
            f32x4 a[RTS], b[4];
#pragma unroll
            for (int rt = 0; rt < RTS; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(ap[rt] + kc * 16);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = *reinterpret_cast<const f32x4*>(job.whh_p + (((long)(g * KC + ug) * KC + kc) * 64 + lane) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[rt][g] = mfma16(a[rt][j], b[g][j], acc[rt][g]);
        }
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int g = 0; g < 4; ++g) red[wave][rt][g][lane] = acc[rt][g];
        __syncthreads();
    }
    const int rt = wave, rtile = rtile0 + rt;
    if (rt >= RTS || rtile >= row_tiles) return;
    f32x4 pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!first) {  // partials summed in wave order 0, 1, 2, 3
            v = red[0][rt][g][lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const f32x4 r = red[w][rt][g][lane];
                v = f32x4{v[0] + r[0], v[1] + r[1], v[2] + r[2], v[3] + r[3]};
            }
        }
        const f32x4 x = addv[g];
        pre[g] = f32x4{v[0] + x[0], v[1] + x[1], v[2] + x[2], v[3] + x[3]};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long row = (long)rtile * 16 + 4 * lq + i;
        const int u = ug * 16 + lr;
        const float ig = sigmoid_fast(pre[0][i]), fg = sigmoid_fast(pre[1][i]);
        const float gg = tanh_fast(pre[2][i]), og = sigmoid_fast(pre[3][i]);
        const float cn = fg * c_old[i] + ig * gg;
        job.c_out[row * H + u] = cn;
        job.h_out[row * ldh + u] = og * tanh_fast(cn);
        if (job.gates_out) {  // training: the activated gates for the backward pass, [row][4H]
            float* gp = job.gates_out + row * 4 * H + u;
            gp[0] = ig;
            gp[H] = fg;
            gp[2 * H] = gg;
            gp[3 * H] = og;
        }
    }
}

template <int RTS>
__global__ __launch_bounds__(256) void bigru_step_kernel(const float* __restrict__ gx, const BiStepJobs jobs, int gx_ct,
                                                         int row_tiles, int H, long ldh, int first) {
    const BiStepJob job = jobs.j[blockIdx.z];
    __shared__ f32x4 red[4][RTS][3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.x, rtile0 = blockIdx.y * RTS;
    const int KC = H >> 4;
    if (!first) {
        f32x4 acc[RTS][3];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[rt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
        const float* ap[RTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
            int rtile = rtile0 + rt;
            rtile = rtile < row_tiles ? rtile : row_tiles - 1;
            ap[rt] = job.h_prev + ((long)rtile * 16 + lr) * ldh + 4 * lq;
        }
#pragma unroll 2
        for (int kc = kc0; kc < kc1; ++kc) {
            f32x4 a[RTS], b[3];
#pragma unroll
            for (int rt = 0; rt < RTS; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(ap[rt] + kc * 16);
#pragma unroll
            for (int g = 0; g < 3; ++g)
                b[g] = *reinterpret_cast<const f32x4*>(job.whh_p + (((long)(g * KC + ug) * KC + kc) * 64 + lane) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
                    for (int g = 0; g < 3; ++g) acc[rt][g] = mfma16(a[rt][j], b[g][j], acc[rt][g]);
        }
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int g = 0; g < 3; ++g) red[wave][rt][g][lane] = acc[rt][g];
        __syncthreads();
    }
    const int rt = wave, rtile = rtile0 + rt;
    if (rt >= RTS || rtile >= row_tiles) return;
    f32x4 hh[3], xg[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!first) {
            v = red[0][rt][g][lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const f32x4 r = red[w][rt][g][lane];
                v = f32x4{v[0] + r[0], v[1] + r[1], v[2] + r[2], v[3] + r[3]};
            }
        }
        hh[g] = v;
        xg[g] = *reinterpret_cast<const f32x4*>(gx + ((job.gx_tile0 + (long)rtile * gx_ct + g * KC + ug) * 64 + lane) * 4);
    }
    const int u = ug * 16 + lr;
    const float bn = job.b_hn[u];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long row = (long)rtile * 16 + 4 * lq + i;
        const float hp = first ? 0.f : job.h_prev[row * ldh + u];
        const float r = sigmoid_f(xg[0][i] + hh[0][i]);
        const float z = sigmoid_f(xg[1][i] + hh[1][i]);
        const float hn = hh[2][i] + bn;
        const float n = tanhf(xg[2][i] + r * hn);
        job.h_out[row * ldh + u] = n + z * (hp - n);
        if (job.gates_out) {  // training: [row][4H] = r | z | n | hn
            float* sp = job.gates_out + row * 4 * H + u;
            sp[0] = r;
            sp[H] = z;
            sp[2 * H] = n;
            sp[3 * H] = hn;
        }
    }
}

// ---- BPTT ----------------------------------------------------------------------------------------------------------------
struct BiBpttJob {
    const float* dh_out;     // this direction's columns of dh at its frame (row stride lddh)
    const float* dg_next;    // its gate gradients at the frame of its previous BPTT step (row stride ldg)
    const float* dghn_next;  // GRU [N][H]
    const float* whhT_p;
    float* carry;            // dc (LSTM) / carry (GRU) [N][H]
    const float* save;       // [N][4H] of this frame
    const float* c_t;        // LSTM [N][H]
    const float* c_prev;     // LSTM: the cell state this frame's step started from
    const float* h_prev;     // GRU: its columns of the hidden sequence at the frame its step started from (row stride ldh)
    float* dg;               // its gate gradients at this frame (row stride ldg)
    float* dghn;             // GRU [N][H]
};
struct BiBpttJobs {
    BiBpttJob j[2];
};

// dh_rec = dgates_next W_hh for RTS x CTS blocks (K = 4H, 4-way split-K, fixed-order reduction), then the cell derivative.
// last: BPTT step 0 of both directions (nothing flows in from a later step); first: its last step (the zero initial state).
template <int RTS, int CTS>
__global__ __launch_bounds__(256) void bilstm_bptt_step_kernel(const BiBpttJobs jobs, int row_tiles, int H, long lddh, long ldg,
                                                               int last, int first) {
    const BiBpttJob job = jobs.j[blockIdx.z];
    __shared__ f32x4 red[4][RTS][CTS][64];
    static_assert(RTS * CTS <= 4, "one finished tile per wave at most");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug0 = blockIdx.x * CTS, rtile0 = blockIdx.y * RTS;
    const int G = 4 * H, KC = G >> 4;
    const int ert = wave / CTS, ect = wave % CTS;
    const bool fin = wave < RTS * CTS && rtile0 + ert < row_tiles;
    float e_gate[4][4], e_dh[4], e_ct[4], e_dc[4], e_cp[4];
    if (fin) {  // everything the element-wise part reads, before the K loop
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = (long)(rtile0 + ert) * 16 + 4 * lq + i;
            const int u = (ug0 + ect) * 16 + lr;
            const float* gp = job.save + row * G + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) e_gate[i][g] = gp[(long)g * H];
            e_dh[i] = job.dh_out[row * lddh + u];
            e_ct[i] = job.c_t[row * H + u];
            e_dc[i] = last ? 0.f : job.carry[row * H + u];
            e_cp[i] = first ? 0.f : job.c_prev[row * H + u];
        }
    }
    if (!last) {
        f32x4 acc[RTS][CTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
        const float* ap[RTS];
        const float* bp[CTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
            int rtile = rtile0 + rt;
            rtile = rtile < row_tiles ? rtile : row_tiles - 1;
            ap[rt] = job.dg_next + ((long)rtile * 16 + lr) * ldg + 4 * lq;
        }
#pragma unroll
        for (int ct = 0; ct < CTS; ++ct) bp[ct] = job.whhT_p + ((long)(ug0 + ct) * KC * 64 + lane) * 4;
#pragma unroll 2
        for (int kc = kc0; kc < kc1; ++kc) {
            f32x4 a[RTS], b[CTS];
#pragma unroll
            for (int rt = 0; rt < RTS; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(ap[rt] + kc * 16);
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) b[ct] = *reinterpret_cast<const f32x4*>(bp[ct] + (long)kc * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
                    for (int ct = 0; ct < CTS; ++ct) acc[rt][ct] = mfma16(a[rt][j], b[ct][j], acc[rt][ct]);
        }
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) red[wave][rt][ct][lane] = acc[rt][ct];
        __syncthreads();
    }
    if (!fin) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!last) {
        v = red[0][ert][ect][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const f32x4 r = red[w][ert][ect][lane];
            v = f32x4{v[0] + r[0], v[1] + r[1], v[2] + r[2], v[3] + r[3]};
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long row = (long)(rtile0 + ert) * 16 + 4 * lq + i;
        const int u = (ug0 + ect) * 16 + lr;
        const float ig = e_gate[i][0], fg = e_gate[i][1], gg = e_gate[i][2], og = e_gate[i][3];
        const float dh = e_dh[i] + v[i];
        const float tc = tanhf(e_ct[i]);
        const float d_o = dh * tc;
        const float dct = e_dc[i] + dh * og * (1.f - tc * tc);
        const float cp = e_cp[i];
        float* dg = job.dg + row * ldg + u;
        dg[0] = dct * gg * ig * (1.f - ig);
        dg[H] = dct * cp * fg * (1.f - fg);
        dg[2 * H] = dct * ig * (1.f - gg * gg);
        dg[3 * H] = d_o * og * (1.f - og);
        job.carry[row * H + u] = dct * fg;
    }
}

// rec = [dgx_next[:, :2H] | dghn_next] W_hh (K = 3H), then the GRU cell derivative (gru_bptt_step_kernel's formulas)
template <int RTS, int CTS>
__global__ __launch_bounds__(256) void bigru_bptt_step_kernel(const BiBpttJobs jobs, int row_tiles, int H, long lddh, long ldg,
                                                              long ldh, int last, int first) {
    const BiBpttJob job = jobs.j[blockIdx.z];
    __shared__ f32x4 red[4][RTS][CTS][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug0 = blockIdx.x * CTS, rtile0 = blockIdx.y * RTS;
    const int KC = (3 * H) >> 4, KX = (2 * H) >> 4;
    if (!last) {
        f32x4 acc[RTS][CTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
        long arow[RTS];
        const float* bp[CTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
            int rtile = rtile0 + rt;
            rtile = rtile < row_tiles ? rtile : row_tiles - 1;
            arow[rt] = (long)rtile * 16 + lr;
        }
#pragma unroll
        for (int ct = 0; ct < CTS; ++ct) bp[ct] = job.whhT_p + ((long)(ug0 + ct) * KC * 64 + lane) * 4;
#pragma unroll 2
        for (int kc = kc0; kc < kc1; ++kc) {
            f32x4 a[RTS], b[CTS];
#pragma unroll
            for (int rt = 0; rt < RTS; ++rt) {
                const float* src = kc < KX ? job.dg_next + arow[rt] * ldg + kc * 16 : job.dghn_next + arow[rt] * H + (kc - KX) * 16;
                a[rt] = *reinterpret_cast<const f32x4*>(src + 4 * lq);
            }
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) b[ct] = *reinterpret_cast<const f32x4*>(bp[ct] + (long)kc * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
                    for (int ct = 0; ct < CTS; ++ct) acc[rt][ct] = mfma16(a[rt][j], b[ct][j], acc[rt][ct]);
        }
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) red[wave][rt][ct][lane] = acc[rt][ct];
        __syncthreads();
    }
    for (int tt = wave; tt < RTS * CTS; tt += 4) {
        const int rt = tt / CTS, ct = tt % CTS;
        const int rtile = rtile0 + rt;
        if (rtile >= row_tiles) continue;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!last) {
            v = red[0][rt][ct][lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const f32x4 r = red[w][rt][ct][lane];
                v = f32x4{v[0] + r[0], v[1] + r[1], v[2] + r[2], v[3] + r[3]};
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = (long)rtile * 16 + 4 * lq + i;
            const int u = (ug0 + ct) * 16 + lr;
            const long idx = row * H + u;
            const float* sp = job.save + row * 4 * H + u;
            const float r = sp[0], z = sp[H], n = sp[2 * H], hn = sp[3 * H];
            const float dh = job.dh_out[row * lddh + u] + v[i] + (last ? 0.f : job.carry[idx]);
            const float hp = first ? 0.f : job.h_prev[row * ldh + u];
            const float dn_pre = dh * (1.f - z) * (1.f - n * n);
            const float dz_pre = dh * (hp - n) * z * (1.f - z);
            const float dr_pre = dn_pre * hn * r * (1.f - r);
            float* dg = job.dg + row * ldg + u;
            dg[0] = dr_pre;
            dg[H] = dz_pre;
            dg[2 * H] = dn_pre;
            job.dghn[idx] = dn_pre * r;
            job.carry[idx] = dh * z;
        }
    }
}

__global__ __launch_bounds__(256) void time_flip_kernel(const float* __restrict__ src, long lds, float* __restrict__ dst, long ldd,
                                                        int T, int N, int K) {
    const long total = (long)T * N * K;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % K);
        const long tn = i / K;
        const int n = (int)(tn % N), t = (int)(tn / N);
        dst[((long)t * N + n) * ldd + c] = src[((long)(T - 1 - t) * N + n) * lds + c];
    }
}

__global__ __launch_bounds__(256) void add_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, long ld,
                                                       float* __restrict__ out, long ldo, long rows, int cols) {
    const long total = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols;
        const int c = (int)(i % cols);
        out[r * ldo + c] = a[r * ld + c] + b[r * ld + c];
    }
}

// Row tiles per workgroup: one up to four tiles (64 rows x 512 units x two directions are already a workgroup per CU), two
// beyond (one W_hh fragment load then feeds two MFMAs).
inline int bi_rts(int row_tiles) { return row_tiles > 4 ? 2 : 1; }

// frame of direction d at step s, and the frame its step started from (-1 / T: none, the zero state)
inline int bi_frame(int d, int s, int T) { return d ? T - 1 - s : s; }

int bi_check(int T, int N, int H, int s) {
    if (T < 1 || N < 16 || N % 16 != 0 || H < 64 || H % 64 != 0 || s < 0 || s >= T) {
        fsn_set_error("birnn step: need T >= 1, N a positive multiple of 16, H a multiple of 64 and 0 <= s < T (got %d, %d, %d, %d)", T,
                      N, H, s);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

BiStepJobs bi_step_jobs(const FsnBiLayer& L, int s, int g) {
    const int row_tiles = L.N / 16, KC = L.H / 16;
    const long ct = (long)2 * g * KC;
    const size_t nh = (size_t)L.N * L.H;
    BiStepJobs jobs{};
    for (int d = 0; d < 2; ++d) {
        const int t = bi_frame(d, s, L.T), tp = d ? t + 1 : t - 1;
        BiStepJob& j = jobs.j[d];
        j.whh_p = L.whh_p[d];
        j.h_out = L.hseq + (size_t)t * L.N * L.ldh + (size_t)d * L.H;
        j.h_prev = s ? L.hseq + (size_t)tp * L.N * L.ldh + (size_t)d * L.H : j.h_out;  // step 0: any valid address, not read
        j.b_hn = L.b_hn[d];
        j.gx_tile0 = (long)t * row_tiles * ct + (long)d * g * KC;
        if (L.save[d]) {
            j.gates_out = L.save[d] + (size_t)t * nh * 4;
            if (g == 4) {  // LSTM: the cell sequence behind the gates
                float* cseq = L.save[d] + (size_t)L.T * nh * 4;
                j.c_out = cseq + (size_t)t * nh;
                j.c_prev = s ? cseq + (size_t)tp * nh : j.c_out;
            }
        } else {
            j.c_prev = j.c_out = L.c[d];
        }
    }
    return jobs;
}

}  // namespace

int fsn_launch_bilstm_step(const FsnBiLayer& L, int s, hipStream_t stream) {
    if (bi_check(L.T, L.N, L.H, s) != FSN_OK) return FSN_ERR_ARG;
    const int row_tiles = L.N / 16, KC = L.H / 16;
    const BiStepJobs jobs = bi_step_jobs(L, s, 4);
    if (bi_rts(row_tiles) == 2)
        hipLaunchKernelGGL(bilstm_step_kernel<2>, dim3(KC, (row_tiles + 1) / 2, 2), dim3(256), 0, stream, L.gx, jobs, 8 * KC,
                           row_tiles, L.H, L.ldh, s == 0);
    else
        hipLaunchKernelGGL(bilstm_step_kernel<1>, dim3(KC, row_tiles, 2), dim3(256), 0, stream, L.gx, jobs, 8 * KC, row_tiles,
                           L.H, L.ldh, s == 0);
    return fsn_check_launch("bilstm_step_kernel");
}

int fsn_launch_bigru_step(const FsnBiLayer& L, int s, hipStream_t stream) {
    if (bi_check(L.T, L.N, L.H, s) != FSN_OK) return FSN_ERR_ARG;
    const int row_tiles = L.N / 16, KC = L.H / 16;
    const BiStepJobs jobs = bi_step_jobs(L, s, 3);
    if (bi_rts(row_tiles) == 2)
        hipLaunchKernelGGL(bigru_step_kernel<2>, dim3(KC, (row_tiles + 1) / 2, 2), dim3(256), 0, stream, L.gx, jobs, 6 * KC,
                           row_tiles, L.H, L.ldh, s == 0);
    else
        hipLaunchKernelGGL(bigru_step_kernel<1>, dim3(KC, row_tiles, 2), dim3(256), 0, stream, L.gx, jobs, 6 * KC, row_tiles,
                           L.H, L.ldh, s == 0);
    return fsn_check_launch("bigru_step_kernel");
}

// BPTT step s: the forward direction at frame T - 1 - s, the reverse one at frame s; both are at their first BPTT step in
// launch 0 and reach their zero initial state in launch T - 1.
int fsn_launch_bilstm_bptt_step(const FsnBiBptt& B, int s, hipStream_t stream) {
    if (bi_check(B.T, B.N, B.H, s) != FSN_OK) return FSN_ERR_ARG;
    const int row_tiles = B.N / 16, T = B.T, H = B.H;
    const size_t nh = (size_t)B.N * H;
    const long ldg = (long)8 * H;
    BiBpttJobs jobs{};
    for (int d = 0; d < 2; ++d) {
        const int t = bi_frame(d, T - 1 - s, T);  // d = 0: T - 1 - s, d = 1: s
        const int t_from = d ? t + 1 : t - 1;     // the frame this frame's forward step started from
        const int t_next = d ? t - 1 : t + 1;     // the frame of the previous BPTT step
        const float* gates = B.save[d];
        const float* cseq = gates + (size_t)T * nh * 4;
        BiBpttJob& j = jobs.j[d];
        j.dh_out = B.dh + (size_t)t * B.N * B.lddh + (size_t)d * H;
        j.dg = B.dg + (size_t)t * B.N * ldg + (size_t)d * 4 * H;
        j.dg_next = s ? B.dg + (size_t)t_next * B.N * ldg + (size_t)d * 4 * H : j.dg;
        j.whhT_p = B.whhT_p[d];
        j.carry = B.carry[d];
        j.save = gates + (size_t)t * nh * 4;
        j.c_t = cseq + (size_t)t * nh;
        j.c_prev = s < T - 1 ? cseq + (size_t)t_from * nh : j.c_t;
    }
    if (row_tiles >= 64 && H % 32 == 0)
        hipLaunchKernelGGL((bilstm_bptt_step_kernel<2, 2>), dim3(H / 32, (row_tiles + 1) / 2, 2), dim3(256), 0, stream, jobs,
                           row_tiles, H, B.lddh, ldg, s == 0, s == T - 1);
    else
        hipLaunchKernelGGL((bilstm_bptt_step_kernel<1, 1>), dim3(H / 16, row_tiles, 2), dim3(256), 0, stream, jobs, row_tiles, H,
                           B.lddh, ldg, s == 0, s == T - 1);
    return fsn_check_launch("bilstm_bptt_step_kernel");
}

int fsn_launch_bigru_bptt_step(const FsnBiBptt& B, int s, hipStream_t stream) {
    if (bi_check(B.T, B.N, B.H, s) != FSN_OK) return FSN_ERR_ARG;
    const int row_tiles = B.N / 16, T = B.T, H = B.H;
    const size_t nh = (size_t)B.N * H;
    const long ldg = (long)6 * H;
    BiBpttJobs jobs{};
    for (int d = 0; d < 2; ++d) {
        const int t = bi_frame(d, T - 1 - s, T);
        const int t_from = d ? t + 1 : t - 1;
        const int t_next = d ? t - 1 : t + 1;
        BiBpttJob& j = jobs.j[d];
        j.dh_out = B.dh + (size_t)t * B.N * B.lddh + (size_t)d * H;
        j.dg = B.dg + (size_t)t * B.N * ldg + (size_t)d * 3 * H;
        j.dghn = B.dghn[d] + (size_t)t * nh;
        j.dg_next = s ? B.dg + (size_t)t_next * B.N * ldg + (size_t)d * 3 * H : j.dg;
        j.dghn_next = s ? B.dghn[d] + (size_t)t_next * nh : j.dghn;
        j.whhT_p = B.whhT_p[d];
        j.carry = B.carry[d];
        j.save = B.save[d] + (size_t)t * nh * 4;
        j.h_prev = B.hseq + (size_t)(s < T - 1 ? t_from : t) * B.N * B.ldh + (size_t)d * H;
    }
    if (row_tiles >= 64 && H % 32 == 0)
        hipLaunchKernelGGL((bigru_bptt_step_kernel<2, 2>), dim3(H / 32, (row_tiles + 1) / 2, 2), dim3(256), 0, stream, jobs,
                           row_tiles, H, B.lddh, ldg, B.ldh, s == 0, s == T - 1);
    else
        hipLaunchKernelGGL((bigru_bptt_step_kernel<1, 1>), dim3(H / 16, row_tiles, 2), dim3(256), 0, stream, jobs, row_tiles, H,
                           B.lddh, ldg, B.ldh, s == 0, s == T - 1);
    return fsn_check_launch("bigru_bptt_step_kernel");
}

int fsn_launch_add_rows(const float* a, const float* b, long ld, float* out, long ldo, long rows, int cols, hipStream_t stream) {
    const long total = rows * cols;
    const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(add_rows_kernel, dim3(grid), dim3(256), 0, stream, a, b, ld, out, ldo, rows, cols);
    return fsn_check_launch("add_rows_kernel");
}

int fsn_launch_time_flip(const float* src, long lds, float* dst, long ldd, int T, int N, int K, hipStream_t stream) {
    const long total = (long)T * N * K;
    const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(time_flip_kernel, dim3(grid), dim3(256), 0, stream, src, lds, dst, ldd, T, N, K);
    return fsn_check_launch("time_flip_kernel");
}
