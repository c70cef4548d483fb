// Persistent many-row LSTM / GRU layer with a WIDE INPUT PROJECTION INSIDE (K = H): a layer whose input is the hidden
// sequence of an equally wide layer below.  See lstm_rec_kernels.hip for the recurrence and the regime.
//
// Which plan reaches which instantiation (H = 384, two unit groups per wave, RT = 2 - 4 row tiles per workgroup - what
// fsn_lstm_rec_x_supported admits; at RT = 1 / 5 the caller keeps the projection GEMM + lstm_rec_kernel pair):
//   lstm_rec_x_kernel<384, RT, 2, GRU = false, HSEQ = false>  the LAST sub-band layer with the two-row output layer fused
//       (fsn_api_fullsubnet.hip: run_recurrence with x_main when CoreDims::l1x - fp32 arithmetic; BASELINE config 2), and
//       fsn_lstm_layer_fc_forward (fsn_api_layers.hip: Fast FullSubNet's second bottleneck layer + its output layer)
//   lstm_rec_x_kernel<384, RT, 2, false, HSEQ = true>         a layer inside a stack, h_t stored (fsn_lstm_layer_forward with
//       I == H, with or without left-over tiles beside it)
//   lstm_rec_x_kernel<384, RT, 2, GRU = true, HSEQ = true>    the same for nn.GRU (fsn_gru_layer_forward, fsn_api_gru.hip);
//       the GRU's output layer is a separate launch, so there is no fused GRU form
#include "lstm_cell.h"
#include "persist_sync.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Last sub-band layer with its INPUT PROJECTION INSIDE: gates = b + x_t W_ih^T + h_{t-1} W_hh^T with x_t = h_t of the
// layer below, read from that layer's hidden sequence (4.8 GB at config 2).  The separate K = 384 projection GEMM and
// its 19.2 GB fragment-ordered `gx` round trip (written once, read back once per batch) are gone; the K loop of a gate
// pass is twice as long (768), so the per-pass costs - cell update, pass boundary, barriers - weigh half as much.
//
// h_{t-1} stays in LDS as in lstm_rec_kernel (16 RT x (H + 4) floats); x_t does not fit next to it, so it streams
// through a two-stage LDS ring in K slices of SK chunks (RT x SK fragments of 1 KB per stage).  The ring is filled by
// LDS-DMA (global_load_lds_dwordx4: no registers, nothing for the waves to wait on), one fragment per instruction:
// lane (row i, quarter q) fetches the 16 bytes x[row i][16 kc + 4 q ..] so that a stage holds the A fragments in the
// lane order ds_read_b128 wants (conflict-free by construction).  A gate pass walks the four slices of x_t and then
// h_{t-1}; the four passes of a step re-stream the same 96 KB tile (L2 hits), the next slice always in flight behind
// the current one.  Slice boundaries are LDS-only barriers (the DMA a wave issued a whole slice earlier has long
// landed: it is older than a dozen weight fragments the wave has consumed since, and loads return in order).
// Output layer fused exactly as in lstm_rec_kernel (the hidden sequence of this layer is never stored).
// ---------------------------------------------------------------------------------------------
// The fragment is persist_sync.h's fsn_lds_dma (vector address) / fsn_lds_dma_s (wave-uniform base + lane offset).
// (Non-temporal / sc0 sc1 fills were measured in round 5: +0.4 .. +0.8 ms - the slices are re-read from L2 / Infinity Cache.)
#ifndef FSN_REC_VCAP
#define FSN_REC_VCAP 76  // x 2 on gfx950's unified register file = 152: three waves per SIMD + room for a step workgroup
#endif
// HSEQ: the layer is not the last one of its stack (or its output layer is not the fused two-row one): h_t is streamed
// out as whole rows to hseq_out [Tp][Npad][H], like lstm_rec_in_kernel does, and no output layer is formed - every
// stacked nn.LSTM layer of a SequenceModel (sequence_model.py:52-58) then takes its input from the layer below with
// no projection GEMM and no gx round trip (Fast FullSubNet's bottleneck: fast_fullsubnet/model.py:66-74).
template <int H, int RT, int UG, bool GRU, bool HSEQ>
__global__ __launch_bounds__((H / (16 * UG)) * 64) __attribute__((amdgpu_num_vgpr(FSN_REC_VCAP))) void lstm_rec_x_kernel(const float* __restrict__ xseq,
                                                                          const float* __restrict__ w_p,
                                                                          unsigned whh_off,
                                                                          const float* __restrict__ bias, int Tp,
                                                                          int Npad, const FsnRecFc fc) {
    // (HSEQ: the destination travels in fc.crm_r - the kernel's signature, and with it the register allocation of the
    // fused form, stays what it was)
    constexpr int NW = H / (16 * UG);
    constexpr int KC = H / 16;
    constexpr int HS = H + 4;
    constexpr int ROWS = RT * 16;
    constexpr int SK = 6;              // K chunks per x slice
    constexpr int NSL = KC / SK;       // slices per pass
    constexpr int NF = RT * SK;        // 1 KB fragments per ring stage
    static_assert(KC % SK == 0 && SK % 2 == 0 && KC % 2 == 0, "slice width must divide the K range; chunks go in pairs");
    // xs [2][NF][256] | hl [ROWS][HS] | wl [2][H].  The ring comes first: its LDS-DMA destination travels in M0,
    // and byte addresses below 64 KB are safe whatever width of M0 the DMA path honours.
    extern __shared__ __attribute__((aligned(16))) float xs[];
    float* hl = xs + 2 * NF * 256;
    float* wl = hl + ROWS * HS;

    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const long n0 = (long)blockIdx.x * ROWS;
    if (!HSEQ)
        for (int i = threadIdx.x; i < 2 * H; i += NW * 64) {  // rows 0 / 1 of the packed output weights, un-tiled
            const int c = i / H, k = i % H;
            wl[i] = fc.w_p[(((k >> 4) * 64) + ((k & 15) >> 2) * 16 + c) * 4 + (k & 3)];
        }
    // FCT: the output layer's tail without its per-step overhead - (b, f) of the workgroup's first row once
    // (rows are consecutive; the per-step form divided two 64-bit integers per thread and step), the bias from scalar
    // registers, the quad sums by DPP instead of ds_bpermute, and the two product chains kept scalar (hipcc paired them
    // into v_pk_fma_f32 at the price of three v_mov per product).  Same arithmetic, same order.
    int fc_b0 = 0, fc_f0 = 0;
    float fc_bias0 = 0.f, fc_bias1 = 0.f;
    if (!HSEQ) {
        const long ng0 = n0 + fc.row0;
        fc_b0 = (int)(ng0 / fc.F);
        fc_f0 = (int)(ng0 - (long)fc_b0 * fc.F);
        fc_bias0 = fc.bias[0];
        fc_bias1 = fc.bias[1];
    }
    // KOPT: the recurrent product's K loop without per-chunk vector instructions.  Vector instructions and fp32 MFMAs share
    // the SIMD (tools/probe_overlap.hip), and the rolled loop spent 11 of them per 64 MFMAs: the hidden state sits beyond
    // the 64 KB an LDS read's immediate offset reaches, so every row tile's address was re-derived per chunk (6 v_add), and
    // the refilled weight fragments landed in fresh registers that were then copied (4 v_mov_b64 behind a vmcnt(0)).  Now:
    // two base registers (row tiles 0-1 / 2-3) advanced once per 6 chunks, immediates inside, and the refill of a
    // fragment pinned behind the last MFMA that reads it, so that it returns into the same registers.
    static_assert(RT >= 2 && RT <= 4, "two base registers reach row tiles 0-1 / 2-3");
    // GRU: the GRU as a four-gate cell (lstm_cell.h).  Its skipped x slices (pass 1, from step 1 on) must leave the ring
    // stage of a pass' first slice where it was: a whole number of stage PAIRS per pass.
    static_assert(!GRU || NSL % 2 == 0, "the GRU form skips whole passes of the x ring: slices per pass must be even");
    // PK: gate non-linearities on pairs (v_pk_*_f32, see sigmoid_fast2); c / the staged values are accumulator-shaped vectors
    f32x4 cst[RT][UG], tmp[RT][UG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int u = 0; u < UG; ++u)
#pragma unroll
            for (int i = 0; i < 4; ++i) cst[rt][u][i] = 0.f;
    for (int i = threadIdx.x; i < ROWS * HS; i += NW * 64) hl[i] = 0.f;

    // ring stage `buf` <- slice `sl` of x_t: this wave's share of the NF fragments
    const unsigned xlane = (unsigned)(lr * H + 4 * lq);  // lane part of the source address; the rest is uniform
    const unsigned xs_lds = (unsigned)(size_t)(__attribute__((address_space(3))) float*)xs;  // LDS byte address
    auto fill = [&](int buf, int t, int sl) {
        const float* src = xseq + ((long)t * Npad + n0) * H + sl * (SK * 16);  // wave-uniform
        for (int f = wave; f < NF; f += NW) {
            const int rt = f / SK, kcl = f - rt * SK;
            fsn_lds_dma(src + (rt * 16 * H + kcl * 16) + xlane,
                        __builtin_amdgcn_readfirstlane(xs_lds + (unsigned)((buf * NF + f) * 1024)));
        }
    };
    // FSA: the fills' addresses from scalar registers - a wave's fragments of a stage are the same (row
    // tile, chunk) pairs all through the kernel, so their offsets are formed once, and the source is base + lane offset
    // (the loop form spent a 64-bit vector add, a vector add and a v_readfirstlane per fragment, inside a real loop)
    constexpr int FPW = (NF + NW - 1) / NW;  // fragments per wave and stage (the last one only in the first waves if NW does not divide NF)
    int fsa_src[FPW], fsa_lds[FPW];
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
        const int f = wave + i * NW, rt = f / SK, kcl = f - rt * SK;
        fsa_src[i] = __builtin_amdgcn_readfirstlane(rt * 16 * H + kcl * 16);
        fsa_lds[i] = __builtin_amdgcn_readfirstlane((int)xs_lds + f * 1024);
    }
    const unsigned xlane_bytes = xlane * 4u;
    auto fill_s = [&](int buf, int t, int sl) {
        const float* src = xseq + ((long)t * Npad + n0) * H + sl * (SK * 16);  // wave-uniform
#pragma unroll
        for (int i = 0; i < FPW; ++i)
            if (NF % NW == 0 || wave + i * NW < NF)
                fsn_lds_dma_s(src + fsa_src[i], xlane_bytes, (unsigned)(fsa_lds[i] + buf * (NF * 1024)));
    };
    fill(0, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // Weight fragments travel in a two-deep ring (b0 / b1, written out by hand so that no copy is needed and every
    // wait is for the older of two requests); b0 always holds - or has in flight - the first fragments the next
    // K chunk needs, across slice, pass and step boundaries (the first chunk of a pass never starts cold).
    f32x4 b0[UG], b1[UG];
    // fragment (gate g, unit group u of this wave, chunk kc): element offset from w_p (W_ih, with W_hh whh_off
    // elements behind it) = a wave-uniform part (scalar registers) + 256 kc, + this lane's 16 bytes
    // buffer loads (T8): resource descriptor + scalar byte offset + this lane's constant 16 l - no per-load VGPR
    // address arithmetic at all
    const __amdgpu_buffer_rsrc_t wrsrc = fsn_buffer_rsrc(w_p);
    const unsigned lane16 = (unsigned)lane * 16u;
    auto wofs = [&](int g, int u) { return (unsigned)((g * KC + wave * UG + u) * KC) * 256u; };
    auto wload = [&](unsigned ofs) { return fsn_buffer_load<f32x4>(wrsrc, lane16, ofs * 4u); };
    float bias_n[UG];  // the bias of the coming pass, requested a pass ahead
    {
        int g0 = 1;
        asm volatile("" : "+s"(g0));
#pragma unroll
        for (int u = 0; u < UG; ++u) {
            b0[u] = wload(wofs(g0, u));
            bias_n[u] = bias[(g0 * KC + wave * UG + u) * 16 + lr];
        }
    }
    // acc[rt][u] += A(16 rows x 16 k) B(16 k x 16 units): a = this lane's A fragment address of row tile 0
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

    // FLATE: a slice's ring fills are issued BEHIND the first row tile's MFMAs of the slice's first block
    // instead of ahead of the block: the block that follows a slice barrier - where all twelve waves stand together - opens
    // with two LDS reads and eight MFMAs, and the fills' instructions run under the other waves' MFMAs (the same gain was
    // measured with the fills left out: it is the shape of the block, not the fills' latency).
    auto mma_fill = [&](f32x4 (&acc)[RT][UG], const float* a, int a_rt_stride, const f32x4 (&b)[UG], int buf, int nt, int nsl) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + a_rt_stride);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int u = 0; u < UG; ++u) acc[0][u] = mfma16(a0[jj], b[u][jj], acc[0][u]);
        __builtin_amdgcn_sched_barrier(0);
        if (nt < Tp) fill_s(buf, nt, nsl);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int rt = 1; rt < RT; ++rt) {
            const f32x4 av = rt == 1 ? a1 : *reinterpret_cast<const f32x4*>(a + rt * a_rt_stride);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int u = 0; u < UG; ++u) acc[rt][u] = mfma16(av[jj], b[u][jj], acc[rt][u]);
        }
    };

    for (int t = 0; t < Tp; ++t) {
        // gate order of evaluation: f (1), i (0), g (2), o (3)
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            __builtin_amdgcn_sched_barrier(0);
            int g = pass == 0 ? 1 : (pass == 1 ? 0 : pass);
            int gn = pass == 0 ? 0 : (pass == 1 ? 2 : (pass == 2 ? 3 : 1));  // the gate after this one
            asm volatile("" : "+s"(g));  // opaque: see lstm_rec_kernel
            asm volatile("" : "+s"(gn));
            // GRU: the nx gate (pass 2) has no recurrent part, the nh gate (pass 1) no input part - its x slices are
            // skipped from step 1 on (at step 0 nothing else runs in that pass and the zero block keeps the ring's order)
            const bool hpart = t > 0 && !(GRU && pass == 2);
            const bool xpart = !(GRU && pass == 1 && t > 0);
            const bool prev_h = t > 0 && !(GRU && pass == 3);  // the pass before this one had a recurrent product
            f32x4 acc[RT][UG];
            unsigned wx[UG], wh[UG], wxn[UG];  // uniform offsets: W_ih / W_hh of this gate, the next pass' first fragment
#pragma unroll
            for (int u = 0; u < UG; ++u) {
                wx[u] = wofs(g, u);
                wh[u] = wx[u] + whh_off;
                wxn[u] = wofs(gn, u) + ((GRU && pass == 0 && t > 0) ? whh_off : 0u);
                const float b = bias_n[u];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][u] = f32x4{b, b, b, b};
                bias_n[u] = bias[(gn * KC + wave * UG + u) * 16 + lr];
            }
            // ---- x_t W_ih^T, slice by slice ------------------------------------------------------
#pragma unroll 1
            for (int sl = 0; sl < (xpart ? NSL : 0); ++sl) {
                const int j = pass * NSL + sl;  // slice counter of the step: ring stage j & 1
                // (the barrier that opens a pass' first slice is taken in the middle of the previous pass' recurrent product
                // instead - its fills were issued before that product began - so that no barrier follows the gate
                // non-linearities)
                if (j > 0 && !(sl == 0 && prev_h)) {
                    // this wave's fills of stage j & 1 were issued a slice ago, before UG SK weight fragments it has
                    // consumed since; at most the UG prefetched ones are still in flight
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(UG) : "memory");
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                }
                // next slice into the other stage (last read in slice j - 1, which every wave has left):
                // same x_t for the next pass, x_{t+1} after the last pass
                const int nsl = sl + 1 < NSL ? sl + 1 : 0;
                const int nt = (sl + 1 < NSL || pass < 3) ? t : t + 1;
                const float* xa = xs + ((j & 1) * NF) * 256 + lane * 4;
#pragma unroll
                for (int kk = 0; kk < SK; kk += 2) {
                    const int kc = sl * SK + kk;
#pragma unroll
                    for (int u = 0; u < UG; ++u)
                        b1[u] = wload(wx[u] + (unsigned)(kc + 1) * 256u);
                    __builtin_amdgcn_sched_barrier(0);  // requests first, pinned: hipcc otherwise sinks them to their use
                    if (kk == 0) mma_fill(acc, xa, SK * 256, b0, (j + 1) & 1, nt, nsl);
                    else mma(acc, xa + kk * 256, SK * 256, b0);
                    __builtin_amdgcn_sched_barrier(0);
                    // chunk kc + 2: W_ih, or the first chunk of W_hh, or (h_{-1} = 0: no W_hh product) of the next pass
                    const bool more_x = kc + 2 < KC;
#pragma unroll
                    for (int u = 0; u < UG; ++u) {
                        b0[u] = wload(more_x ? wx[u] + (unsigned)(kc + 2) * 256u : (hpart ? wh[u] : wxn[u]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    mma(acc, xa + (kk + 1) * 256, SK * 256, b1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // ---- h_{t-1} W_hh^T (h_{-1} = 0) -------------------------------------------------------
            if (hpart) {
                // two LDS byte addresses, opaque to the optimiser (it would fold the tile's own offset into the immediates
                // and overflow them again): row tiles 0-1 / 2-3
                typedef const __attribute__((address_space(3))) float* lds_cptr;
                unsigned hb01 = (unsigned)(size_t)(lds_cptr)(hl + lr * HS + 4 * lq), hb23 = hb01 + 32u * HS * 4u;
                asm volatile("" : "+v"(hb01));
                asm volatile("" : "+v"(hb23));
                lds_cptr ha01 = (lds_cptr)(size_t)hb01;
                lds_cptr ha23 = (lds_cptr)(size_t)hb23;
                auto mmah = [&](int kofs, const f32x4 (&b)[UG]) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const f32x4 av = *reinterpret_cast<const __attribute__((address_space(3))) f32x4*>((rt < 2 ? ha01 : ha23) + (rt & 1) * 16 * HS + kofs);
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                            for (int u = 0; u < UG; ++u) acc[rt][u] = mfma16(av[jj], b[u][jj], acc[rt][u]);
                    }
                };
#pragma unroll 1
                for (int hs = 0; hs < NSL; ++hs) {
                    if (pass < 3 && hs == NSL / 2) {  // the next pass' first slice barrier, taken here
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(UG) : "memory");
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
                        __builtin_amdgcn_s_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
                    }
#pragma unroll
                    for (int kk = 0; kk < SK; kk += 2) {
                        const int kc = hs * SK + kk;
#pragma unroll
                        for (int u = 0; u < UG; ++u) b1[u] = wload(wh[u] + (unsigned)(kc + 1) * 256u);
                        __builtin_amdgcn_sched_barrier(0);
                        mmah(kk * 16, b0);
                        __builtin_amdgcn_sched_barrier(0);  // the refill behind the last MFMA that reads b0: same registers
                        const bool more_h = kc + 2 < KC;
#pragma unroll
                        for (int u = 0; u < UG; ++u) b0[u] = wload(more_h ? wh[u] + (unsigned)(kc + 2) * 256u : wxn[u]);
                        __builtin_amdgcn_sched_barrier(0);
                        mmah((kk + 1) * 16, b1);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    ha01 += SK * 16;
                    ha23 += SK * 16;
                }
            }
            if constexpr (GRU) {  // cst = h_{t-1} (h_t after the z pass); tmp: r, r * (W_hn h + b_hn), n
                if (pass == 0) {
                    FSN_CELL_PASS2(tmp, sigmoid_fast2(a))
                } else if (pass == 1) {
                    FSN_CELL_PASS2(tmp, m * a)
                } else if (pass == 2) {
                    FSN_CELL_PASS2(tmp, tanh_fast2(a + m))
                } else {
                    FSN_CELL_PASS2(cst, m + sigmoid_fast2(a) * (c - m))
                }
            } else if (pass == 0) {
                FSN_CELL_PASS2(cst, sigmoid_fast2(a) * c)
            } else if (pass == 1) {
                FSN_CELL_PASS2(tmp, sigmoid_fast2(a))
            } else if (pass == 2) {
                FSN_CELL_PASS2(cst, c + m * tanh_fast2(a))
            } else {
                FSN_CELL_PASS2(tmp, sigmoid_fast2(a) * tanh_fast2(c))
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // every wave has finished reading h_{t-1}; the fill of the next step's first slice stays in flight
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        {
            // one base register, re-derived every step (opaque to the optimiser): hoisted out of the time loop the
            // 32 store addresses become 32 live registers that end up in scratch
            unsigned hwb = (unsigned)((4 * lq) * HS + (wave * UG) * 16 + lr);
            asm volatile("" : "+v"(hwb));
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
        if (HSEQ) {
            // stream h_t out as whole rows: hseq_out[t][n0 + row][0..H)
            float* dst = fc.crm_r + ((long)t * Npad + n0) * H;
            for (int i = threadIdx.x; i < ROWS * (H / 4); i += NW * 64) {
                const int row = i / (H / 4), c4 = i % (H / 4);
                *reinterpret_cast<f32x4*>(dst + (long)row * H + c4 * 4) =
                    *reinterpret_cast<const f32x4*>(hl + row * HS + c4 * 4);
            }
        } else {
            // output layer on the spot (nn.Linear(H, 2)): 4 threads per (row, output), a quarter of K each (FCT)
            const int tid = threadIdx.x;
            if (tid < ROWS * 8) {
                const int part = tid & 3, c = (tid >> 2) & 1, row = tid >> 3;
                const float* hp = hl + row * HS + part * (H / 4);
                const float* wp = wl + c * H + part * (H / 4);
                float a0 = 0.f, a1 = 0.f;
#pragma unroll 2
                for (int k = 0; k < H / 4; k += 8) {
                    const f32x4 h0 = *reinterpret_cast<const f32x4*>(hp + k), w0 = *reinterpret_cast<const f32x4*>(wp + k);
                    const f32x4 h1 = *reinterpret_cast<const f32x4*>(hp + k + 4),
                                w1 = *reinterpret_cast<const f32x4*>(wp + k + 4);
                    a0 = fmaf(h0[0], w0[0], a0);
                    a0 = fmaf(h0[1], w0[1], a0);
                    a0 = fmaf(h0[2], w0[2], a0);
                    a0 = fmaf(h0[3], w0[3], a0);
                    asm volatile("" : "+v"(a0));  // not a twin of the other chain any more: no pairing
                    a1 = fmaf(h1[0], w1[0], a1);
                    a1 = fmaf(h1[1], w1[1], a1);
                    a1 = fmaf(h1[2], w1[2], a1);
                    a1 = fmaf(h1[3], w1[3], a1);
                }
                float v = a0 + a1;
                v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
                v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
                if (part == 0 && t >= fc.la && (int)n0 + row < fc.N) {
                    int f = fc_f0 + row, b = fc_b0;
                    while (f >= fc.F) {
                        f -= fc.F;
                        ++b;
                    }
                    (c ? fc.crm_i : fc.crm_r)[((long)b * fc.T + (t - fc.la)) * fc.FP + f] = v + (c ? fc_bias1 : fc_bias0);
                }
            }
        }
    }
}

template <int H, int RT, bool HSEQ, int CELL = 0, int UG = 2>
int launch_rec_x(const float* xseq, const float* wih_p, const float* whh_p, const float* bias, int Tp, int Npad,
                 int main_wgs, hipStream_t s, const FsnRecFc* fc, float* hseq_out) {
    constexpr int NW = H / (16 * UG);
    const size_t lds = ((size_t)RT * 16 * (H + 4) + 2 * H + (size_t)2 * RT * 6 * 256) * sizeof(float);
    auto kern = lstm_rec_x_kernel<H, RT, UG, CELL != 0, HSEQ>;
    if (lds > 160 * 1024) {
        fsn_set_error("lstm_rec_x: cannot reserve %zu bytes of LDS", lds);
        return FSN_ERR_LAUNCH;
    }
    FSN_TRY_RESERVE_LDS("lstm_rec_x", kern, lds);
    if (whh_p < wih_p || whh_p - wih_p > 0x3fffffffL) {
        fsn_set_error("lstm_rec_x: W_hh must follow W_ih in one packed buffer");
        return FSN_ERR_ARG;
    }
    FsnRecFc a{};
    if (fc) a = *fc;
    if (HSEQ) a.crm_r = hseq_out;
    hipLaunchKernelGGL(kern, dim3((unsigned)main_wgs), dim3(NW * 64), lds, s, xseq, wih_p, (unsigned)(whh_p - wih_p), bias,
                       Tp, Npad, a);
    return fsn_check_launch("lstm_rec_x_kernel");
}

}  // namespace

// The last sub-band layer with its input projection inside (lstm_rec_x_kernel): built for H = 384 and 2 - 4 row
// tiles per workgroup (at 5 the x ring no longer fits beside the hidden state; the caller then keeps the
// projection GEMM + lstm_rec_kernel pair).
bool fsn_lstm_rec_x_supported(int H, int RT) { return H == 384 && RT >= 2 && RT <= 4; }

int fsn_launch_lstm_rec_x(const float* xseq, const float* wih_p, const float* whh_p, const float* bias, int Tp, int Npad,
                          int H, int RT, int main_wgs, hipStream_t s, const FsnRecFc* fc, float* hseq_out, int cell) {
    fsn_trace(FSN_TR_LSTM_REC_X);
    if (((!fc || !fc->w_p) && !hseq_out) || !fsn_lstm_rec_x_supported(H, RT)) {
        fsn_set_error("lstm_rec_x: needs the fused output layer or a hidden-sequence buffer, H = 384 and 2 - 4 row tiles "
                      "(got H %d, RT %d)", H, RT);
        return FSN_ERR_ARG;
    }
    if (cell) {  // GRU (lstm_cell.h)
        if (hseq_out) {
            if (RT == 2) return launch_rec_x<384, 2, true, 1>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, nullptr, hseq_out);
            if (RT == 3) return launch_rec_x<384, 3, true, 1>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, nullptr, hseq_out);
            return launch_rec_x<384, 4, true, 1>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, nullptr, hseq_out);
        }
        fsn_set_error("lstm_rec_x: the GRU cell is instantiated for the hidden-sequence form (its output layer is a separate launch)");
        return FSN_ERR_ARG;
    }
    if (hseq_out) {  // a layer inside a stack: h_t stored, no output layer
        if (RT == 2) return launch_rec_x<384, 2, true>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, nullptr, hseq_out);
        if (RT == 3) return launch_rec_x<384, 3, true>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, nullptr, hseq_out);
        return launch_rec_x<384, 4, true>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, nullptr, hseq_out);
    }
    if (RT == 2) return launch_rec_x<384, 2, false>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, fc, nullptr);
    if (RT == 3) return launch_rec_x<384, 3, false>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, fc, nullptr);
    return launch_rec_x<384, 4, false>(xseq, wih_p, whh_p, bias, Tp, Npad, main_wgs, s, fc, nullptr);
}
