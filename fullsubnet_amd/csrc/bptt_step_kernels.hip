// Training-step pieces of nn.LSTM (recipes/dns_interspeech_2020/fullsubnet/trainer.py:56-63 ->
// autograd through audio_zen/model/module/sequence_model.py:52-58): back-propagation through time.
//
// Per layer, with the activated gates i,f,g,o and the cell sequence c_t saved by the forward pass:
//   for t = T-1 .. 0:
//     dh      = dH_t (from the layer above) + dh_rec (from step t+1)
//     do      = dh * tanh(c_t);  dc = dc_carry + dh * o * (1 - tanh(c_t)^2)
//     di, dg, df = dc*g, dc*i, dc*c_{t-1};  dc_carry = dc * f
//     dgates_t = [di i(1-i), df f(1-f), dg (1-g^2), do o(1-o)]          (bptt_elem_kernel)
//     dh_rec  = dgates_t W_hh                                            (gemm_kernel, K = 4H)
//   dX = dgates W_ih (one GEMM over all steps);  dW_ih = dgates^T X;  dW_hh = dgates_{1..}^T H_{0..T-2};
//   db = column sums of dgates                                           (gemm_tn_kernel / colsum: gemm_tn_kernels.hip)
// First, correctness-first version: one elementwise launch + one small GEMM per step.
#include "fsn_common.h"

namespace {

__global__ __launch_bounds__(256) void bptt_elem_kernel(const float* __restrict__ dh_out,
                                                        const float* __restrict__ dh_rec, float* __restrict__ dc,
                                                        const float* __restrict__ gates,
                                                        const float* __restrict__ c_t,
                                                        const float* __restrict__ c_prev,
                                                        float* __restrict__ dgates, long n_elems, int H, int last,
                                                        int first) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_elems) return;
    const long row = idx / H;
    const int u = (int)(idx % H);
    const float* gp = gates + row * 4 * H + u;
    const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
    const float dh = dh_out[idx] + (last ? 0.f : dh_rec[idx]);
    const float tc = tanhf(c_t[idx]);
    const float d_o = dh * tc;
    const float dct = (last ? 0.f : dc[idx]) + dh * og * (1.f - tc * tc);
    const float cp = first ? 0.f : c_prev[idx];
    float* dg = dgates + row * 4 * H + u;
    dg[0] = dct * gg * ig * (1.f - ig);
    dg[H] = dct * cp * fg * (1.f - fg);
    dg[2 * H] = dct * ig * (1.f - gg * gg);
    dg[3 * H] = d_o * og * (1.f - og);
    dc[idx] = dct * fg;
}

// One BPTT step, fused: dh_rec = dgates_{t+1} W_hh for RTS 16-row tiles x CTS 16-unit groups (K = 4H,
// 4-way split-K over the waves: one dgates fragment feeds CTS MFMAs, one W_hh^T fragment RTS of them;
// partials reduced through LDS in a fixed order) followed by the cell derivative of those blocks ->
// dgates_t.  The mirror image of lstm_step_kernel; grid = (H/16/CTS, ceil(row tiles / RTS)).
template <int RTS, int CTS, int NW = 4>
__global__ __launch_bounds__(NW * 64) void bptt_step_kernel(const float* __restrict__ dh_out,
                                                        const float* __restrict__ dgates_next,
                                                        const float* __restrict__ whhT_p, float* __restrict__ dc,
                                                        const float* __restrict__ gates,
                                                        const float* __restrict__ c_t,
                                                        const float* __restrict__ c_prev,
                                                        float* __restrict__ dgates, int row_tiles, int H, int last,
                                                        int first) {
    __shared__ f32x4 red[NW][RTS][CTS][64];  // NW-way split-K (16 for the full-band model's single row tile)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug0 = blockIdx.x * CTS, rtile0 = blockIdx.y * RTS;
    const int G = 4 * H, KC = G >> 4;
    static_assert(RTS * CTS <= NW, "one finished tile per wave at most");
    // The wave that finishes tile (ert, ect) asks for everything the element-wise part reads - saved gates, dh, c_t,
    // dc, c_{t-1}: 8 cold values per element - before the K loop instead of after the barrier.
    const int ert = wave / CTS, ect = wave % CTS;
    const bool fin = wave < RTS * CTS && rtile0 + ert < row_tiles;
    float e_gate[4][4], e_dh[4], e_ct[4], e_dc[4], e_cp[4];
    if (fin) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = (long)(rtile0 + ert) * 16 + 4 * lq + i;
            const int u = (ug0 + ect) * 16 + lr;
            const float* gp = gates + row * G + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) e_gate[i][g] = gp[(long)g * H];
            e_dh[i] = dh_out[row * H + u];
            e_ct[i] = c_t[row * H + u];
            e_dc[i] = last ? 0.f : dc[row * H + u];
            e_cp[i] = first ? 0.f : c_prev[row * H + u];
        }
    }
    if (!last) {
        f32x4 acc[RTS][CTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTS; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int kc0 = wave * (KC / NW), kc1 = kc0 + KC / NW;
        const float* ap[RTS];
        const float* bp[CTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
            int rtile = rtile0 + rt;
            rtile = rtile < row_tiles ? rtile : row_tiles - 1;
            ap[rt] = dgates_next + ((long)rtile * 16 + lr) * G + 4 * lq;
        }
#pragma unroll
        for (int ct = 0; ct < CTS; ++ct) bp[ct] = whhT_p + ((long)(ug0 + ct) * KC * 64 + lane) * 4;
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
    if (fin) {
        const int rt = ert, ct = ect;
        const int rtile = rtile0 + rt;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (!last) {
            v = red[0][rt][ct][lane];
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                const f32x4 r = red[w][rt][ct][lane];
                v = f32x4{v[0] + r[0], v[1] + r[1], v[2] + r[2], v[3] + r[3]};
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = (long)rtile * 16 + 4 * lq + i;
            const int u = (ug0 + ct) * 16 + lr;
            const long idx = row * H + u;
            const float ig = e_gate[i][0], fg = e_gate[i][1], gg = e_gate[i][2], og = e_gate[i][3];
            const float dh = e_dh[i] + v[i];
            const float tc = tanhf(e_ct[i]);
            const float d_o = dh * tc;
            const float dct = e_dc[i] + dh * og * (1.f - tc * tc);
            const float cp = e_cp[i];
            float* dg = dgates + row * G + u;
            dg[0] = dct * gg * ig * (1.f - ig);
            dg[H] = dct * cp * fg * (1.f - fg);
            dg[2 * H] = dct * ig * (1.f - gg * gg);
            dg[3 * H] = d_o * og * (1.f - og);
            dc[idx] = dct * fg;
        }
    }
}

}  // namespace

// The BPTT step in the one-workgroup-per-CU shape of lstm_step_cu_kernel (lstm_step_kernels.hip), for row counts that
// fill the chip at least once (used from 192 row tiles): a workgroup = four row tiles x CTW
// column tiles of dh_rec = dgates_{t+1} W_hh, one row tile per wave, the whole K = 4H range per wave (no split-K
// exchange).  A stage is four K chunks: wave w fetches chunk w's CTW weight fragments for everybody (two-stage LDS
// buffer, one barrier per stage) and its own four A fragments; the next stage's fetch is pinned under the 16 CTW
// MFMAs of this one.  Everything the element-wise part reads (saved gates, dh, c_t, dc, c_{t-1}) is requested
// before the K loop - with one wave per SIMD there are registers to spare, and read afterwards each of the 8 CTW x 4
// values per lane would pay its own memory round trip.
template <int CTW>
__global__ __launch_bounds__(256) void bptt_step_cu_kernel(const float* __restrict__ dh_out,
                                                           const float* __restrict__ dgates_next,
                                                           const float* __restrict__ whhT_p, float* __restrict__ dc,
                                                           const float* __restrict__ gates,
                                                           const float* __restrict__ c_t, const float* c_prev,
                                                           float* __restrict__ dgates, int H, int last, int first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug0 = blockIdx.x * CTW;
    const long rtile = (long)blockIdx.y * 4 + wave;
    const int G = 4 * H, KC = G >> 4, stages = KC >> 2;
    if (first) c_prev = c_t;  // any valid address: the value is not used at t = 0
    float e_gate[CTW][4][4], e_dh[CTW][4], e_ct[CTW][4], e_dc[CTW][4], e_cp[CTW][4];
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = rtile * 16 + 4 * lq + i;
            const int u = (ug0 + ct) * 16 + lr;
            const float* gp = gates + row * G + u;
#pragma unroll
            for (int g = 0; g < 4; ++g) e_gate[ct][i][g] = gp[(long)g * H];
            e_dh[ct][i] = dh_out[row * H + u];
            e_ct[ct][i] = c_t[row * H + u];
            e_dc[ct][i] = last ? 0.f : dc[row * H + u];
            e_cp[ct][i] = c_prev[row * H + u];
        }
    f32x4 acc[CTW];
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!last) {  // uniform over the workgroup (barriers inside)
        __shared__ f32x4 bsh[2][4 * CTW][64];
        const float* ap = dgates_next + (rtile * 16 + lr) * G + 4 * lq;
        const float* bp = whhT_p + ((long)ug0 * KC * 64 + lane) * 4;
        f32x4 an[4], bn[CTW];
        auto fetch = [&](int st) {
#pragma unroll
            for (int q = 0; q < 4; ++q) an[q] = *reinterpret_cast<const f32x4*>(ap + (st * 4 + q) * 16);
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct)
                bn[ct] = *reinterpret_cast<const f32x4*>(bp + ((long)ct * KC + st * 4 + wave) * 256);
        };
        fetch(0);
#pragma unroll
        for (int ct = 0; ct < CTW; ++ct) bsh[0][wave * CTW + ct][lane] = bn[ct];
        f32x4 a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = an[q];
        __syncthreads();
        for (int st = 0; st < stages; ++st) {
            __builtin_amdgcn_sched_barrier(0);
            fetch(st + 1 < stages ? st + 1 : st);
            __builtin_amdgcn_sched_barrier(0);
            const int buf = st & 1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 b[CTW];
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) b[ct] = bsh[buf][q * CTW + ct][lane];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct) acc[ct] = mfma16(a[q][j], b[ct][j], acc[ct]);
            }
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) bsh[buf ^ 1][wave * CTW + ct][lane] = bn[ct];
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = an[q];
            __syncthreads();
        }
    }
#pragma unroll
    for (int ct = 0; ct < CTW; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = rtile * 16 + 4 * lq + i;
            const int u = (ug0 + ct) * 16 + lr;
            const long idx = row * H + u;
            const float ig = e_gate[ct][i][0], fg = e_gate[ct][i][1], gg = e_gate[ct][i][2], og = e_gate[ct][i][3];
            const float dh = e_dh[ct][i] + acc[ct][i];
            const float tc = tanhf(e_ct[ct][i]);
            const float d_o = dh * tc;
            const float dct = e_dc[ct][i] + dh * og * (1.f - tc * tc);
            const float cp = first ? 0.f : e_cp[ct][i];
            float* dg = dgates + row * G + u;
            dg[0] = dct * gg * ig * (1.f - ig);
            dg[H] = dct * cp * fg * (1.f - fg);
            dg[2 * H] = dct * ig * (1.f - gg * gg);
            dg[3 * H] = d_o * og * (1.f - og);
            dc[idx] = dct * fg;
        }
}

constexpr int BPTT_SPLIT16_TILES = 8;  // measured (round 6, 5 tiles x 512 units, Fast FullSubNet's decoder at batch 72): see DESIGN 7.4
int fsn_launch_bptt_step(const float* dh_out, const float* dgates_next, const float* whhT_p, float* dc,
                         const float* gates, const float* c_t, const float* c_prev, float* dgates, int row_tiles, int H,
                         int last, int first, hipStream_t s) {
    // measured at 129 row tiles (tools/bench_train.py): 2 x 2 72.2 ms per training step, 1 x 2 73.0, 2 x 1 75.1,
    // 1 x 1 76.3, 4 x 2 76.8, 2 x 4 77.8, 4 x 4 89.0; a no-split-K form (a wave per tile for the whole K = 4H
    // range, which pays off in the forward step) is 10 % slower here: K is four times longer
    // measured (tools/bench_train.py): 256 row tiles 103.3 -> 96.8 ms per training step; at 128 tiles (one workgroup
    // per CU, nothing left to overlap its element-wise part with) 57.9 against 57.0 for the split-K form below
    if (row_tiles >= 192 && row_tiles % 4 == 0 && H % 48 == 0) {
        hipLaunchKernelGGL(bptt_step_cu_kernel<3>, dim3(H / 48, row_tiles / 4), dim3(256), 0, s, dh_out, dgates_next,
                           whhT_p, dc, gates, c_t, c_prev, dgates, H, last, first);
        return fsn_check_launch("bptt_step_cu_kernel");
    }
    const int cfg = row_tiles >= 64 && H % 32 == 0 ? 22 : 11;
#define FSN_BPTT_CASE(R, C)                                                                                        \
    hipLaunchKernelGGL((bptt_step_kernel<R, C>), dim3(H / 16 / C, (row_tiles + R - 1) / R), dim3(256), 0, s, dh_out, \
                       dgates_next, whhT_p, dc, gates, c_t, c_prev, dgates, row_tiles, H, last, first)
    if (cfg == 22) FSN_BPTT_CASE(2, 2);
    else if (row_tiles <= BPTT_SPLIT16_TILES && (4 * H / 16) % 16 == 0)  // a handful of rows (full-band model, the sibling models' blocks): 16-way split-K
        hipLaunchKernelGGL((bptt_step_kernel<1, 1, 16>), dim3(H / 16, row_tiles), dim3(1024), 0, s, dh_out, dgates_next,
                           whhT_p, dc, gates, c_t, c_prev, dgates, row_tiles, H, last, first);
    else FSN_BPTT_CASE(1, 1);
#undef FSN_BPTT_CASE
    return fsn_check_launch("bptt_step_kernel");
}

int fsn_launch_bptt_elem(const float* dh_out, const float* dh_rec, float* dc, const float* gates, const float* c_t,
                         const float* c_prev, float* dgates, long n_elems, int H, int last, int first, hipStream_t s) {
    hipLaunchKernelGGL(bptt_elem_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, s, dh_out, dh_rec, dc,
                       gates, c_t, c_prev, dgates, n_elems, H, last, first);
    return fsn_check_launch("bptt_elem_kernel");
}
