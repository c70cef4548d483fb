// nn.LSTM's recurrence for FEW rows, one launch per time step (see lstm_rec_kernels.hip for the recurrence and the
// many-row regime): the full-band model (N = B rows), small batches of the sub-band model, the left-over row tiles
// beside a persistent kernel, and the forward pass of the training step.  h and c live in global memory (L2 resident).
//
// Which plan reaches which kernel:
//   lstm_step1_kernel             fsn_launch_lstm_step(.., beside_persistent = 1): run_recurrence's left-over tiles on the
//                                 auxiliary stream beside a resident persistent workgroup (register / LDS budget: tests/test_host_cpu.py)
//   lstm_step_kernel<1 | 2>       fsn_launch_lstm_step / fsn_launch_lstm_step_train below 64 row tiles (2 from 16 tiles on):
//                                 the step path without a persistent part, streaming layers, small training batches
//   lstm_step_rows_kernel<1>      fsn_launch_lstm_step_train from 64 row tiles on when they are not a multiple of four
//   lstm_step_cu_kernel<1 | 2 | 3>  fsn_launch_lstm_step_cu: groups of four tiles, one workgroup per CU - run_recurrence without
//                                 a persistent part (from 8 tiles on) and fsn_launch_lstm_step_train from 64 tiles on (config 3)
//   lstm_step2_kernel             fsn_launch_lstm_wavefront2(w): two layers as a wavefront of T + 1 launches - the full-band model
//                                 when the chain kernel does not take it, sub-band batches below 96 row tiles, two stacked layers
//   lstm_step2_small_kernel       the same with beside_group = 1: the tiles that do not fill a cluster, beside lstm_group_kernels.hip
#include "fsn_common.h"

namespace {

// ---------------------------------------------------------------------------------------------
// One time step.  grid = (H/16 unit groups, ceil(row tiles / RTS)); a workgroup owns RTS 16-row
// tiles x one 16-unit group x the four gates; its 4 waves split K four ways (each wave holds the
// RTS x 4 partial tiles, so one W_hh fragment load feeds RTS MFMAs) and the partials are reduced
// through LDS in a fixed order (deterministic); wave w < RTS then finishes row tile w.  RTS = 1 for
// the few-row launches of inference (full-band model, left-over tiles), larger for the training step.
template <int RTS>
__device__ __forceinline__ void lstm_step_body(const float* __restrict__ gx, const float* __restrict__ whh_p,
                                               const float* __restrict__ h_prev, float* __restrict__ h_out,
                                               const float* c_prev, float* c, float* __restrict__ gates_out,
                                               long gx_rt0, int row_tiles, int H, int first, int rtile0) {
    __shared__ f32x4 red[4][RTS][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.x;
    const int KC = H >> 4, CT = 4 * KC;
    f32x4 acc[RTS][4];
#pragma unroll
    for (int rt = 0; rt < RTS; ++rt)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[rt][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // what the finishing wave's epilogue reads (projection tiles, previous cell state) is requested before the K
    // loop: cold lines, each of which would otherwise cost a memory round trip after the barrier
    const int ftile = rtile0 + wave < row_tiles ? rtile0 + wave : row_tiles - 1;
    f32x4 addv[4];
    float c_old[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
        addv[g] = *reinterpret_cast<const f32x4*>(gx + (((gx_rt0 + ftile) * CT + g * KC + ug) * 64 + lane) * 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) c_old[i] = first ? 0.f : c_prev[((long)ftile * 16 + 4 * lq + i) * H + ug * 16 + lr];
    if (!first) {
        const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
        const float* ap[RTS];
#pragma unroll
        for (int rt = 0; rt < RTS; ++rt) {
            int rtile = rtile0 + rt;
            rtile = rtile < row_tiles ? rtile : row_tiles - 1;
            ap[rt] = h_prev + ((long)rtile * 16 + lr) * H + 4 * lq;
        }
#pragma unroll 2
        for (int kc = kc0; kc < kc1; ++kc) {
            f32x4 a[RTS], b[4];
#pragma unroll
            for (int rt = 0; rt < RTS; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(ap[rt] + kc * 16);
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = *reinterpret_cast<const f32x4*>(whh_p + (((long)(g * KC + ug) * KC + kc) * 64 + lane) * 4);
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
        const long idx = row * H + ug * 16 + lr;
        // hardware exp / rcp forms (fsn_common.h): the libm ones were ~12 % of this kernel at 129 row tiles
        const float ig = sigmoid_fast(pre[0][i]), fg = sigmoid_fast(pre[1][i]);
        const float gg = tanh_fast(pre[2][i]), og = sigmoid_fast(pre[3][i]);
        const float cn = fg * c_old[i] + ig * gg;
        c[idx] = cn;
        h_out[idx] = og * tanh_fast(cn);
        if (gates_out) {  // training: keep the activated gates for the backward pass, [row][4H]
            float* gp = gates_out + row * 4 * H + ug * 16 + lr;
            gp[0] = ig;
            gp[H] = fg;
            gp[2 * H] = gg;
            gp[3 * H] = og;
        }
    }
}

template <int RTS>
__global__ __launch_bounds__(256) void lstm_step_kernel(const float* __restrict__ gx,
                                                        const float* __restrict__ whh_p,
                                                        const float* __restrict__ h_prev,
                                                        float* __restrict__ h_out, const float* c_prev,
                                                        float* c, float* __restrict__ gates_out, long gx_rt0,
                                                        int row_tiles, int H, int first) {
    lstm_step_body<RTS>(gx, whh_p, h_prev, h_out, c_prev, c, gates_out, gx_rt0, row_tiles, H, first, blockIdx.y * RTS);
}

// The same step for several weight sets in one launch (fsn_launch_lstm_step_multi): grid.y runs over the row tiles of all
// sets, each workgroup looks up its set and is lstm_step_kernel<1>'s workgroup of that set's tile.  A row's products are
// summed in the order of lstm_step_kernel<1 | 2> (the K split over the four waves and the order of the partials do not
// depend on RTS): the same bits as one launch per set below 64 row tiles.
__global__ __launch_bounds__(256) void lstm_step_multi_kernel(const FsnStepSets sets, int H) {
    const int y = blockIdx.y;
    int j = 0;
    while (j + 1 < sets.n && y >= sets.s[j + 1].tile0) ++j;
    const FsnStepSet& q = sets.s[j];
    lstm_step_body<1>(q.gx, q.whh_p, q.h_prev, q.h_out, q.c, q.c, nullptr, q.gx_rt0, q.tiles, H, 0, y - q.tile0);
}

// Many rows (the training step's 129 row tiles and more): no split-K at all.  A workgroup takes RW * 4 row
// tiles of one unit group; every wave owns RW of them for the whole K range and finishes them itself, so there
// is no partial-sum exchange, no barrier, and the cell update runs on all four waves instead of one.  The four
// waves read the same W_hh fragments (L1 hits after the first).
template <int RW>
__global__ __launch_bounds__(256) void lstm_step_rows_kernel(const float* __restrict__ gx,
                                                             const float* __restrict__ whh_p,
                                                             const float* __restrict__ h_prev,
                                                             float* __restrict__ h_out, const float* c_prev, float* c,
                                                             float* __restrict__ gates_out, long gx_rt0, int row_tiles,
                                                             int H, int first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.x, rtile0 = (blockIdx.y * 4 + wave) * RW;
    if (rtile0 >= row_tiles) return;
    const int KC = H >> 4, CT = 4 * KC;
    f32x4 acc[RW][4];
    int rtile[RW];
#pragma unroll
    for (int rt = 0; rt < RW; ++rt) {
        rtile[rt] = rtile0 + rt < row_tiles ? rtile0 + rt : row_tiles - 1;
#pragma unroll
        for (int g = 0; g < 4; ++g)
            acc[rt][g] = *reinterpret_cast<const f32x4*>(gx + (((gx_rt0 + rtile[rt]) * CT + g * KC + ug) * 64 + lane) * 4);
    }
    // previous cell state requested before the K loop: read in the epilogue, every element would pay its own
    // memory round trip (and the wait for it also waits for the stores of the element before)
    float c_old[RW][4];
#pragma unroll
    for (int rt = 0; rt < RW; ++rt)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            c_old[rt][i] = first ? 0.f : c_prev[((long)rtile[rt] * 16 + 4 * lq + i) * H + ug * 16 + lr];
    if (!first) {
        const float* ap[RW];
#pragma unroll
        for (int rt = 0; rt < RW; ++rt) ap[rt] = h_prev + ((long)rtile[rt] * 16 + lr) * H + 4 * lq;
        const float* bp = whh_p + ((long)ug * KC * 64 + lane) * 4;
        const long gstride = (long)KC * KC * 256;
#pragma unroll 2
        for (int kc = 0; kc < KC; ++kc) {
            f32x4 a[RW], b[4];
#pragma unroll
            for (int rt = 0; rt < RW; ++rt) a[rt] = *reinterpret_cast<const f32x4*>(ap[rt] + kc * 16);
#pragma unroll
            for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const f32x4*>(bp + g * gstride + (long)kc * 256);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int rt = 0; rt < RW; ++rt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[rt][g] = mfma16(a[rt][j], b[g][j], acc[rt][g]);
        }
    }
#pragma unroll
    for (int rt = 0; rt < RW; ++rt) {
        if (rtile0 + rt >= row_tiles) break;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long row = (long)rtile[rt] * 16 + 4 * lq + i;
            const long idx = row * H + ug * 16 + lr;
            const float ig = sigmoid_fast(acc[rt][0][i]), fg = sigmoid_fast(acc[rt][1][i]);
            const float gg = tanh_fast(acc[rt][2][i]), og = sigmoid_fast(acc[rt][3][i]);
            const float cn = fg * c_old[rt][i] + ig * gg;
            c[idx] = cn;
            h_out[idx] = og * tanh_fast(cn);
            if (gates_out) {
                float* gp = gates_out + row * 4 * H + ug * 16 + lr;
                gp[0] = ig;
                gp[H] = fg;
                gp[2 * H] = gg;
                gp[3 * H] = og;
            }
        }
    }
}

// K loop of lstm_step_cu_kernel: acc[u][g] += A(16 rows x H) W_hh(u, g)^T for the
// wave's row tile, UGW unit groups and four gates.  The four waves of the workgroup need the SAME 4 UGW weight
// fragments per K chunk (they differ in the row tile only): fetched per wave that is 13 KB per wave and chunk
// against 48 MFMAs, 35 B/clk per CU on the vector memory path.  Here every wave
// fetches UGW of the fragments, parks them in LDS (two stages, one barrier per chunk) and all four read them from
// there; only the A fragment is per wave.  ap: this lane's A address for chunk 0; bp: packed W_hh at unit group
// ug0 (+ lane * 4).
template <int UGW>
__device__ __forceinline__ void cu_kloop(f32x4 (&acc)[UGW][4], const float* ap, const float* bp, int KC,
                                         f32x4 (*bsh)[UGW * 4][64]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long gstride = (long)KC * KC * 256, ustride = (long)KC * 256;
    f32x4 an, bn[UGW];
    auto fetch = [&](int kc) {
        an = *reinterpret_cast<const f32x4*>(ap + kc * 16);
#pragma unroll
        for (int k = 0; k < UGW; ++k) {
            const int f = wave * UGW + k, u = f >> 2, g = f & 3;  // fragment f = (unit group u, gate g)
            bn[k] = *reinterpret_cast<const f32x4*>(bp + g * gstride + u * ustride + (long)kc * 256);
        }
    };
    fetch(0);
#pragma unroll
    for (int k = 0; k < UGW; ++k) bsh[0][wave * UGW + k][lane] = bn[k];
    f32x4 a = an;
    __syncthreads();
    for (int kc = 0; kc < KC; ++kc) {
        __builtin_amdgcn_sched_barrier(0);  // next chunk's global fetch first, pinned under this chunk's MFMAs
        fetch(kc + 1 < KC ? kc + 1 : kc);
        __builtin_amdgcn_sched_barrier(0);
        const int buf = kc & 1;
#pragma unroll
        for (int u = 0; u < UGW; ++u) {
            f32x4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) b[g] = bsh[buf][u * 4 + g][lane];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[u][g] = mfma16(a[j], b[g][j], acc[u][g]);
        }
        // the other stage was last read in the previous iteration, which ended with the barrier below
#pragma unroll
        for (int k = 0; k < UGW; ++k) bsh[buf ^ 1][wave * UGW + k][lane] = bn[k];
        a = an;
        __syncthreads();
    }
}

// One step for a row count that fills the chip about once (2 - 9 utterances, 4 x groups of row tiles): the
// launch is shaped so that every CU gets ONE workgroup of four waves, one wave per SIMD, and every wave the same
// work - row tile w of its group x UGW hidden-unit groups x all four gates - with the operands of the next K
// chunk fetched (pinned) while the 16 UGW MFMAs of this one issue.  Against lstm_step_rows_kernel (one unit
// group per wave, 3.1 workgroups per CU at 129 tiles, loads and MFMAs of a chunk back to back): 40 -> 2x us per
// step at 128 tiles.  c_prev / c / gates_out as in lstm_step_rows_kernel (inference: c in place, no gates);
// row_tiles must be a multiple of 4.
template <int UGW>
__global__ __launch_bounds__(256) void lstm_step_cu_kernel(const float* __restrict__ gx,
                                                           const float* __restrict__ whh_p,
                                                           const float* __restrict__ h_prev,
                                                           float* __restrict__ h_out, const float* c_prev,
                                                           float* c, float* __restrict__ gates_out, long gx_rt0,
                                                           int H, int first) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug0 = blockIdx.x * UGW;
    const long rtile = (long)blockIdx.y * 4 + wave;
    if (first) c_prev = c;  // any valid address: the value is not used on the first step
    const int KC = H >> 4, CT = 4 * KC;
    f32x4 acc[UGW][4];
#pragma unroll
    for (int u = 0; u < UGW; ++u)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            acc[u][g] = *reinterpret_cast<const f32x4*>(gx + (((gx_rt0 + rtile) * CT + g * KC + ug0 + u) * 64 + lane) * 4);
    // the previous cell state is asked for now: these are cold lines, and read in the epilogue each one would
    // cost its own memory round trip (the value is unused on the first step; the buffer exists either way)
    float c_old[UGW][4];
#pragma unroll
    for (int u = 0; u < UGW; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) c_old[u][i] = c_prev[(rtile * 16 + 4 * lq + i) * H + (ug0 + u) * 16 + lr];
    if (!first) {  // uniform over the workgroup (barriers inside)
        __shared__ f32x4 bsh[2][UGW * 4][64];
        cu_kloop<UGW>(acc, h_prev + (rtile * 16 + lr) * H + 4 * lq, whh_p + ((long)ug0 * KC * 64 + lane) * 4, KC, bsh);
    }
#pragma unroll
    for (int u = 0; u < UGW; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long idx = (rtile * 16 + 4 * lq + i) * H + (ug0 + u) * 16 + lr;
            const float ig = sigmoid_fast(acc[u][0][i]), fg = sigmoid_fast(acc[u][1][i]);
            const float gg = tanh_fast(acc[u][2][i]), og = sigmoid_fast(acc[u][3][i]);
            const float cn = fg * (first ? 0.f : c_old[u][i]) + ig * gg;
            c[idx] = cn;
            h_out[idx] = og * tanh_fast(cn);
            if (gates_out) {  // training: the activated gates for the backward pass, [row][4H]
                float* gp = gates_out + (rtile * 16 + 4 * lq + i) * 4 * H + (ug0 + u) * 16 + lr;
                gp[0] = ig;
                gp[H] = fg;
                gp[2 * H] = gg;
                gp[3 * H] = og;
            }
        }
}

// The single-tile form also runs the left-over tiles of the sub-band model NEXT TO the resident
// persistent workgroups (12 waves x 152 registers = 456 of the 512 per SIMD lane for the layer-0
// kernel): it only gets a slot there if it needs <= 56 registers and <= 12 KB of LDS - hence this
// inference-only instance without the training outputs (40 + 16 registers; checked by
// tests/test_host_cpu.py on the code object).  With more it silently waits for the 32 ms persistent
// kernel to end (measured: +1.4 ms per batch).
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(24))) void lstm_step1_kernel(const float* __restrict__ gx,
                                                         const float* __restrict__ whh_p,
                                                         const float* __restrict__ h_prev,
                                                         float* __restrict__ h_out, float* __restrict__ c,
                                                         long gx_rt0, int H, int first) {
    // split-K partials meet pairwise (8 KB of LDS instead of 12): next to lstm_rec_x_kernel's 151.5 KB there is
    // room for exactly one such workgroup per CU, and this chain has ~10 x slack against the kernel it runs beside.
    // (Round 5: a grid of one slot per CU with the step's 96 tasks rotating through the slots, so that no CU pays every
    // step's matrix work, measured no different: 81.8 / 82.0 against 81.6 / 81.9 ms per batch.)
    __shared__ f32x4 red[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.x, rtile = blockIdx.y;
    const int KC = H >> 4, CT = 4 * KC;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!first) {
        const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
        const float* ap = h_prev + ((long)rtile * 16 + lr) * H + 4 * lq;
#pragma unroll 4
        for (int kc = kc0; kc < kc1; ++kc) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(ap + kc * 16);
            f32x4 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                b[g] = *reinterpret_cast<const f32x4*>(whh_p + (((long)(g * KC + ug) * KC + kc) * 64 + lane) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = mfma16(a[j], b[g][j], acc[g]);
        }
        if (wave >= 2) {
#pragma unroll
            for (int g = 0; g < 4; ++g) red[wave - 2][g][lane] = acc[g];
        }
        __syncthreads();
        if (wave >= 2) return;
#pragma unroll
        for (int g = 0; g < 4; ++g) {  // wave 0 += wave 2, wave 1 += wave 3
            const f32x4 r = red[wave][g][lane];
            acc[g] = f32x4{acc[g][0] + r[0], acc[g][1] + r[1], acc[g][2] + r[2], acc[g][3] + r[3]};
        }
        __syncthreads();
        if (wave == 1) {
#pragma unroll
            for (int g = 0; g < 4; ++g) red[0][g][lane] = acc[g];
        }
        __syncthreads();
    }
    if (wave != 0) return;
    // everything below accumulates in place: a second live copy of the 16 partial sums is what pushes the
    // templated form over the register budget
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (!first) {  // (w0 + w2) + (w1 + w3)
            const f32x4 r = red[0][g][lane];
            acc[g] = f32x4{acc[g][0] + r[0], acc[g][1] + r[1], acc[g][2] + r[2], acc[g][3] + r[3]};
        }
        const f32x4 x = *reinterpret_cast<const f32x4*>(gx + (((gx_rt0 + rtile) * CT + g * KC + ug) * 64 + lane) * 4);
        acc[g] = f32x4{acc[g][0] + x[0], acc[g][1] + x[1], acc[g][2] + x[2], acc[g][3] + x[3]};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long idx = ((long)rtile * 16 + 4 * lq + i) * H + ug * 16 + lr;
        const float c_old = first ? 0.f : c[idx];
        const float ig = sigmoid_fast(acc[0][i]), fg = sigmoid_fast(acc[1][i]);
        const float gg = tanh_fast(acc[2][i]), og = sigmoid_fast(acc[3][i]);
        const float cn = fg * c_old + ig * gg;
        c[idx] = cn;
        h_out[idx] = og * tanh_fast(cn);
    }
}

// ---------------------------------------------------------------------------------------------
// Two-layer wavefront step: ONE launch advances layer 0 by step i and layer 1 by step i - 1
// (blockIdx.z picks the job), so a two-layer LSTM over T frames is T + 1 dependent launches instead
// of 2 T.  Used where the recurrence is a chain of tiny latency-bound launches: the full-band model
// (N = B rows) and the sub-band model of small batches.  The layer-1 job has no precomputed input
// projection (its input row h0_t has only just been produced): it accumulates x W_ih^T and
// h W_hh^T in the same 4-way split-K pass and adds the bias in the epilogue.
struct FsnStepJob {
    const float* add;    // fragment-ordered tiles added to the accumulators: the layer-0 projection incl. bias
                         // (tile (add_rt0 + rtile) * CT + column tile), or the layer-1 bias tiles (add_rs = 0)
    const float* xw_p;   // layer-1 form: packed W_ih [4H/16][H/16][64][4]; NULL for the layer-0 form
    const float* x;      // layer-1 form: input rows [rows][H] (h of the layer below at this step)
    const float* whh_p;
    const float* h_prev;
    float* h_out;
    float* c;
    long add_rt0;
    int add_rs, first, active;
    int H;          // hidden units of this job's layer (row stride of h / c); the two jobs may differ
    int kx_chunks;  // layer-1 form: input width / 16 (= hidden units / 16 of the layer below)
    int x_ld;       // layer-1 form: row stride of x
    int row_tiles;  // 16-row tiles of this job (the grid is sized for the job with the most)
};
struct FsnStepJobs {
    FsnStepJob j[2];
};
template <class Jobs>
__device__ __forceinline__ void lstm_step2_body(const Jobs& jobs) {
    const FsnStepJob job = jobs.j[blockIdx.z];  // one uniform kernarg fetch, no per-member branching
    const int H = job.H;
    if (!job.active || (int)blockIdx.x * 16 >= H || (int)blockIdx.y >= job.row_tiles) return;  // grid: the widest / tallest job
    __shared__ f32x4 red[3][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int ug = blockIdx.x, rtile = blockIdx.y;
    const int KC = H >> 4, CT = 4 * KC;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the finishing wave asks for everything its epilogue needs (projection / bias tiles, previous cell
    // state) before the K loop: these are cold lines whose latency would otherwise follow the barrier
    f32x4 addv[4];
    float c_old[4];
    const long cidx = ((long)rtile * 16 + 4 * lq) * H + ug * 16 + lr;
    if (wave == 0) {
        const float* ap = job.add + (((job.add_rt0 + (long)rtile * job.add_rs) * CT + ug) * 64 + lane) * 4;
#pragma unroll
        for (int g = 0; g < 4; ++g) addv[g] = *reinterpret_cast<const f32x4*>(ap + (long)g * KC * 256);
        const float* cp = job.first ? job.add : job.c + cidx;  // first step: any valid address, value unused
        const long cs = job.first ? 0 : H;
#pragma unroll
        for (int i = 0; i < 4; ++i) c_old[i] = cp[i * cs];
    }
    const int kc0 = wave * (KC >> 2), kc1 = kc0 + (KC >> 2);
    const float* ah = job.h_prev + ((long)rtile * 16 + lr) * H + 4 * lq;
    const float* bh = job.whh_p + ((long)ug * KC * 64 + lane) * 4;
    const long gstride = (long)KC * KC * 256;  // gate g of unit group ug: column tile g KC + ug
    const int KX = job.kx_chunks;
    const long xstride = (long)KC * KX * 256;
    if (job.xw_p && !job.first && KX == KC) {
        // layer-1 job in steady state: x W_ih^T and h W_hh^T share one loop, so that the loads of both
        // products are in flight together (two back-to-back loops would pay the L2 latency twice)
        const float* ax = job.x + ((long)rtile * 16 + lr) * job.x_ld + 4 * lq;
        const float* bx = job.xw_p + ((long)ug * KC * 64 + lane) * 4;
#pragma unroll 2
        for (int kc = kc0; kc < kc1; ++kc) {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(ax + kc * 16);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(ah + kc * 16);
            f32x4 b0[4], b1[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                b0[g] = *reinterpret_cast<const f32x4*>(bx + g * gstride + (long)kc * 256);
                b1[g] = *reinterpret_cast<const f32x4*>(bh + g * gstride + (long)kc * 256);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = mfma16(a0[j], b0[g][j], acc[g]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[g] = mfma16(a1[j], b1[g][j], acc[g]);
        }
    } else {
        // the two products one after the other: layer 0 (h W_hh^T only), layer 1 at its first step
        // (x W_ih^T only), or a layer 1 whose input width differs from its own (blocks of different widths)
        if (job.xw_p) {
            const int x0 = wave * (KX >> 2), x1 = x0 + (KX >> 2);
            const float* a1p = job.x + ((long)rtile * 16 + lr) * job.x_ld + 4 * lq;
            const float* b1p = job.xw_p + ((long)ug * KX * 64 + lane) * 4;
#pragma unroll 2
            for (int kc = x0; kc < x1; ++kc) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(a1p + kc * 16);
                f32x4 b[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const f32x4*>(b1p + g * xstride + (long)kc * 256);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = mfma16(a[j], b[g][j], acc[g]);
            }
        }
        if (!job.first) {
#pragma unroll 2
            for (int kc = kc0; kc < kc1; ++kc) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(ah + kc * 16);
                f32x4 b[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) b[g] = *reinterpret_cast<const f32x4*>(bh + g * gstride + (long)kc * 256);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = mfma16(a[j], b[g][j], acc[g]);
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) red[wave - 1][g][lane] = acc[g];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const f32x4 r = red[w][g][lane];
            acc[g] = f32x4{acc[g][0] + r[0], acc[g][1] + r[1], acc[g][2] + r[2], acc[g][3] + r[3]};
        }
        acc[g] = f32x4{acc[g][0] + addv[g][0], acc[g][1] + addv[g][1], acc[g][2] + addv[g][2], acc[g][3] + addv[g][3]};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long idx = cidx + (long)i * H;
        // hardware exp / rcp forms as in the persistent kernel: the libm ones are ~2 us of this one-wave
        // epilogue, a sixth of the whole step
        const float ig = sigmoid_fast(acc[0][i]), fg = sigmoid_fast(acc[1][i]);
        const float gg = tanh_fast(acc[2][i]), og = sigmoid_fast(acc[3][i]);
        const float cn = fg * (job.first ? 0.f : c_old[i]) + ig * gg;
        job.c[idx] = cn;
        job.h_out[idx] = og * tanh_fast(cn);
    }
}

__global__ __launch_bounds__(256) void lstm_step2_kernel(const FsnStepJobs jobs) { lstm_step2_body(jobs); }

// The same step beside the group kernel of lstm_group_kernels.hip (two 216-register workgroups per CU): capped at the 80
// registers per lane that are left there; it spills a little, on a chain that has ten times the slack.
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(40))) void lstm_step2_small_kernel(const FsnStepJobs jobs) {
    lstm_step2_body(jobs);
}

}  // namespace

// One step for `row_tiles` 16-row tiles: gx tiles gx_rt0 .. gx_rt0 + row_tiles - 1 of the fragment-
// ordered projection, h_prev / h_out / c point at the first of those rows.
int fsn_launch_lstm_step(const float* gx, const float* whh_p, const float* h_prev, float* h_out, float* c,
                         long gx_rt0, int row_tiles, int H, int first, hipStream_t s, int beside_persistent) {
    fsn_trace(FSN_TR_LSTM_STEP);
    if (beside_persistent) {  // must fit next to a resident persistent workgroup, see lstm_step1_kernel
        if (H % 64 != 0) {
            fsn_set_error("lstm_step: hidden size %d must be a multiple of 64", H);
            return FSN_ERR_ARG;
        }
        hipLaunchKernelGGL(lstm_step1_kernel, dim3(H / 16, row_tiles), dim3(256), 0, s, gx, whh_p, h_prev, h_out, c,
                           gx_rt0, H, first);
        return fsn_check_launch("lstm_step1_kernel");
    }
    return fsn_launch_lstm_step_train(gx, whh_p, h_prev, h_out, c, c, nullptr, gx_rt0, row_tiles, H, first, s);
}

// One step of up to 8 independent layers of the same H, each on its own weights, rows and state: set j owns grid rows
// [tile0, tile0 + tiles) (tile0 ascending from 0, no gaps) and below 64 tiles each, the regime in which
// fsn_launch_lstm_step runs lstm_step_kernel - the launch is bit for bit that launch per set.
int fsn_launch_lstm_step_multi(const FsnStepSets& sets, int H, hipStream_t s) {
    fsn_trace(FSN_TR_LSTM_STEP);
    int next = 0;
    bool ok = H >= 64 && H % 64 == 0 && sets.n >= 1 && sets.n <= 8;
    for (int j = 0; ok && j < sets.n; ++j) {
        const FsnStepSet& q = sets.s[j];
        ok = q.gx && q.whh_p && q.h_prev && q.h_out && q.c && q.gx_rt0 >= 0 && q.tile0 == next && q.tiles >= 1 && q.tiles < 64;
        next += q.tiles;
    }
    if (!ok) {
        fsn_set_error("lstm_step_multi: 1 .. 8 sets of 1 .. 63 row tiles in order without gaps, H %d a multiple of 64", H);
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(lstm_step_multi_kernel, dim3(H / 16, next), dim3(256), 0, s, sets, H);
    return fsn_check_launch("lstm_step_multi_kernel");
}

// One step on row_tiles (a multiple of 4) tiles with the one-workgroup-per-CU kernel; picks the unit groups per
// wave that fill the chip best: cost = rounds of workgroups over the CUs x work per workgroup.
int fsn_launch_lstm_step_cu(const float* gx, const float* whh_p, const float* h_prev, float* h_out, float* c,
                            long gx_rt0, int row_tiles, int H, int first, hipStream_t s, const float* c_prev,
                            float* gates_out) {
    fsn_trace(FSN_TR_LSTM_STEP_CU);
    if (!c_prev) c_prev = c;
    if (H % 16 != 0 || row_tiles % 4 != 0 || row_tiles <= 0) {
        fsn_set_error("lstm_step_cu: H %d must be a multiple of 16 and row_tiles %d a positive multiple of 4", H, row_tiles);
        return FSN_ERR_ARG;
    }
    const int cus = plan_cus();
    const int ugs = H / 16, groups = row_tiles / 4;
    int best = 1;
    long best_cost = -1;
    for (int ugw = 1; ugw <= 3; ++ugw) {
        if (ugs % ugw) continue;
        const long wgs = (long)groups * (ugs / ugw);
        const long cost = ((wgs + cus - 1) / cus) * ugw;
        if (best_cost < 0 || cost <= best_cost) {  // ties: the wider wave tile (fewer operand loads per MFMA)
            best = ugw;
            best_cost = cost;
        }
    }
#define FSN_STEP_CU(U)                                                                                             \
    hipLaunchKernelGGL(lstm_step_cu_kernel<U>, dim3(ugs / U, groups), dim3(256), 0, s, gx, whh_p, h_prev, h_out,    \
                       c_prev, c, gates_out, gx_rt0, H, first)
    if (best == 3) FSN_STEP_CU(3);
    else if (best == 2) FSN_STEP_CU(2);
    else FSN_STEP_CU(1);
#undef FSN_STEP_CU
    return fsn_check_launch("lstm_step_cu_kernel");
}

// Training form: c_{t-1} is read from c_prev, c_t written to c_out (the saved cell sequence) and the
// activated gates i, f, g, o to gates_out [rows][4H].
int fsn_launch_lstm_step_train(const float* gx, const float* whh_p, const float* h_prev, float* h_out,
                               const float* c_prev, float* c_out, float* gates_out, long gx_rt0, int row_tiles, int H,
                               int first, hipStream_t s) {
    if (H % 64 != 0) {
        fsn_set_error("lstm_step: hidden size %d must be a multiple of 64", H);
        return FSN_ERR_ARG;
    }
    if (row_tiles >= 64 && row_tiles % 4 == 0)  // config 3: 16 x 128 bins = 128 tiles = one workgroup per CU
        return fsn_launch_lstm_step_cu(gx, whh_p, h_prev, h_out, c_out, gx_rt0, row_tiles, H, first, s, c_prev, gates_out);
    if (row_tiles >= 64) {  // measured at 129 tiles: 65.1 ms per training step against 66.3 for the split-K form
        hipLaunchKernelGGL(lstm_step_rows_kernel<1>, dim3(H / 16, (row_tiles + 3) / 4), dim3(256), 0, s, gx, whh_p, h_prev,
                           h_out, c_prev, c_out, gates_out, gx_rt0, row_tiles, H, first);
        return fsn_check_launch("lstm_step_rows_kernel");
    }
    const int rts = row_tiles >= 16 ? 2 : 1;  // measured: 2 is the best at 129 tiles, 4 no better
#define FSN_STEP_CASE(R)                                                                                         \
    hipLaunchKernelGGL(lstm_step_kernel<R>, dim3(H / 16, (row_tiles + R - 1) / R), dim3(256), 0, s, gx, whh_p, h_prev, \
                       h_out, c_prev, c_out, gates_out, gx_rt0, row_tiles, H, first)
    if (rts == 2) FSN_STEP_CASE(2);
    else
        FSN_STEP_CASE(1);
#undef FSN_STEP_CASE
    return fsn_check_launch("lstm_step_kernel");
}

// Two LSTM layers over T steps on `row_tiles` 16-row tiles, advanced in a wavefront (see lstm_step2_kernel).
// Layer 0 has H0 units, layer 1 H1 units and H0 inputs.  gx0: layer-0 projection, tile (t, i) at
// t * gx_stride + gx_off + i; wih1_p: layer-1 input weights [4 H1 / 16][H0 / 16][64][4]; bias1_frag: b_ih + b_hh
// of layer 1 as fragment tiles; hseq0 / hseq1: [T][hs_stride rows][H0 / H1] with this launch's rows starting at
// row hs_off; c0 / c1: [row_tiles * 16][H0 / H1].  state_h0 / state_h1: streaming continuation (see header).
int fsn_launch_lstm_wavefront2w(const float* gx0, long gx_stride, long gx_off, const float* whh0_p,
                                const float* wih1_p, const float* bias1_frag, const float* whh1_p, float* hseq0,
                                float* hseq1, long hs_stride, long hs_off, float* c0, float* c1, int T, int row_tiles,
                                int H0, int H1, hipStream_t s, float* state_h0, float* state_h1, int beside_group) {
    if (H0 % 64 != 0 || H1 % 64 != 0 || (state_h0 == nullptr) != (state_h1 == nullptr)) {
        fsn_set_error("lstm_wavefront2: hidden sizes %d / %d must be multiples of 64 (and both states or none)", H0, H1);
        return FSN_ERR_ARG;
    }
    const bool cont = state_h0 != nullptr;
    const size_t step0 = (size_t)hs_stride * H0, step1 = (size_t)hs_stride * H1;
    float* h0 = hseq0 + (size_t)hs_off * H0;
    float* h1 = hseq1 + (size_t)hs_off * H1;
    const int Hmax = H0 > H1 ? H0 : H1;
    for (int i = 0; i <= T; ++i) {
        FsnStepJobs jobs{};
        FsnStepJob& a = jobs.j[0];
        FsnStepJob& b = jobs.j[1];
        a.H = H0;
        b.H = H1;
        a.row_tiles = b.row_tiles = row_tiles;
        if (i < T) {
            a.active = 1;
            a.add = gx0;
            a.add_rt0 = (long)i * gx_stride + gx_off;
            a.add_rs = 1;
            a.whh_p = whh0_p;
            a.h_prev = i ? h0 + (i - 1) * step0 : (cont ? state_h0 : h0);
            a.h_out = h0 + i * step0;
            a.c = c0;
            a.first = i == 0 && !cont;
        }
        if (i >= 1) {
            const int t = i - 1;
            b.active = 1;
            b.add = bias1_frag;
            b.add_rt0 = 0;
            b.add_rs = 0;
            b.xw_p = wih1_p;
            b.x = h0 + t * step0;
            b.x_ld = H0;
            b.kx_chunks = H0 / 16;
            b.whh_p = whh1_p;
            b.h_prev = t ? h1 + (t - 1) * step1 : (cont ? state_h1 : h1);
            b.h_out = h1 + t * step1;
            b.c = c1;
            b.first = t == 0 && !cont;
        }
        // (a 16-wave split of the K range - every wave's operands in one round trip - was tried for the full-band
        // model and lost: 13.3 us per step against 10.5; dispatching and joining 16 waves costs more than it saves)
        if (beside_group) hipLaunchKernelGGL(lstm_step2_small_kernel, dim3(Hmax / 16, row_tiles, 2), dim3(256), 0, s, jobs);
        else hipLaunchKernelGGL(lstm_step2_kernel, dim3(Hmax / 16, row_tiles, 2), dim3(256), 0, s, jobs);
        FSN_TRY_LAUNCH("lstm_step2_kernel");
    }
    if (cont) {
        const size_t rows = (size_t)row_tiles * 16;
        if (hipMemcpyAsync(state_h0, h0 + (size_t)(T - 1) * step0, rows * H0 * sizeof(float), hipMemcpyDeviceToDevice,
                           s) != hipSuccess ||
            hipMemcpyAsync(state_h1, h1 + (size_t)(T - 1) * step1, rows * H1 * sizeof(float), hipMemcpyDeviceToDevice,
                           s) != hipSuccess) {
            fsn_set_error("lstm_wavefront2: state copy failed");
            return FSN_ERR_LAUNCH;
        }
    }
    return FSN_OK;
}

int fsn_launch_lstm_wavefront2(const float* gx0, long gx_stride, long gx_off, const float* whh0_p, const float* wih1_p,
                               const float* bias1_frag, const float* whh1_p, float* hseq0, float* hseq1, long hs_stride,
                               long hs_off, float* c0, float* c1, int T, int row_tiles, int H, hipStream_t s,
                               float* state_h0, float* state_h1, int beside_group) {
    fsn_trace(FSN_TR_LSTM_WAVEFRONT2);
    return fsn_launch_lstm_wavefront2w(gx0, gx_stride, gx_off, whh0_p, wih1_p, bias1_frag, whh1_p, hseq0, hseq1,
                                       hs_stride, hs_off, c0, c1, T, row_tiles, H, H, s, state_h0, state_h1, beside_group);
}
