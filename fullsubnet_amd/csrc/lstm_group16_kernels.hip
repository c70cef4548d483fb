// The sub-band model's two LSTM layers under the reference's OWN training arithmetic (torch.autocast: 16-bit matrix-core
// operands, fp32 accumulation; recipes/dns_interspeech_2020/fullsubnet/trainer.py:56-69, fullsubnet/train.toml:5) as
// persistent launches built for that arithmetic: forward with saves (sequence_model.py:52-58 under autograd) and
// back-propagation through time.  Same work split as lstm_group_kernels.hip / lstm_group_bptt_kernels.hip - clusters
// of 64 rows, eight members of 48 hidden units per layer, two workgroups per CU - and the same buffers in and out
// (hidden sequences, save layout, gate gradients), but a different step:
//
// With 16-bit operands the matrix work of a step is 3 - 6 us and the fp32-era kernels spend 30 - 45 us per step in a
// CHAIN of memory round trips (profiles/r03_bptt_probe_f16.md: weights through L2 / LDS with a barrier per four K
// chunks ~10 us, the partners' operand ~9, saved activations ~8, dword write-through stores ~11).  Here
//   * every product is formed TRANSPOSED, D^T[gate column or unit][batch row] = W (A operand) x activations^T (B
//     operand): a lane's four accumulator values are four CONSECUTIVE hidden units of one batch row, so everything
//     that touches memory - h, the saves, the gate gradients, the exchanged partial sums - moves as 16-byte accesses
//     (5 - 6x fewer fabric transactions than dword write-through stores);
//   * the waves of a workgroup split the WEIGHT dimension: each wave streams its own weight fragments L2 -> registers
//     through a ring that is filled BEFORE the step's hand-off wait (weights do not depend on it) - no LDS staging of
//     weights, no barrier inside a K loop; the ACTIVATIONS (what the partners handed over) are staged once per product
//     into LDS, rounded to 16 bits once on the way in, and shared by the four waves;
//   * forward: wave g forms gate g of the member's 48 units for all 64 rows; the four gates of a unit meet through one
//     LDS exchange, after which a thread owns (row, four units): cell update, one 16-byte write-through store of h per
//     (row, unit quad), the saves as 16-byte stores after the flag;
//   * BPTT splits K instead of the output: a member keeps the gate gradients of ITS 192 gate columns (it has just
//     formed them: no exchange to read them) and multiplies them by its 192 ROWS of W_hh / W_ih - a [64 x 192] x
//     [192 x 384] product whose result is a PARTIAL dh for all 384 units; the eight partials of a cluster are summed
//     in a fixed order by the member that owns the units.  Per member and step 96 KB written + 96 KB read in
//     accumulator-fragment order (16-byte, fully coalesced) instead of a 393 KB gather of everyone's gate gradients;
//     layer 1 also forms dgates1 W_ih1 (layer 0's dH) from the same LDS tile, handed over through a four-deep ring.
// Arithmetic: operands rounded to fp16 / bf16 (round to nearest even) exactly where fsn_mma_k16 rounds them - weights
// once when packed, activations when staged - products and sums in fp32, everything stored in fp32.  Results differ
// from the fp32-era kernels under the same arithmetic only by the order of the fp32 sums (tests/test_gpu_amp.py holds
// both to the exact emulation).  Flags / bounded waits / status / poison: the group family of persist_sync.h, as in lstm_group_kernels.hip.
#include "persist_sync.h"

namespace {

constexpr int QH = 384;            // hidden units (both layers)
constexpr int QG = 4 * QH;         // gate columns
constexpr int QM = 8;              // members per cluster and layer
constexpr int QU = QH / QM;        // units per member (48)
constexpr int QROWS = 64;          // rows per cluster
constexpr int QFS = 32;            // words between flag groups (one 128-byte line each)
constexpr int QD = 4;              // forward: K blocks (32 k each) of weight fragments in flight per wave
constexpr int Q_H16_OFF = QG * 2;  // FSN_ARITH_SAVES16: byte offset of the 16-bit h_t inside a row's save slot (behind the 16-bit gates)
constexpr int QDX = 4;             // BPTT: slots of the exchanged gate-gradient tiles (layer 1 may run QDX - 1 steps ahead of layer 0)
constexpr int ACT_STRIDE = QH * 2 + 16;   // bytes per row of a staged [64][384] 16-bit tile (+16: conflict-free b128 reads)
constexpr int X_STRIDE = 32 * 2 + 16;     // layer-0 input tile [64][32]
constexpr int GSH_STRIDE = QU * 4 + 16;   // bytes per row of the gate exchange [4][64][48] fp32
constexpr int DSH_STRIDE = 4 * QU * 2 + 16;  // BPTT: own gate gradients [64][192] 16-bit
constexpr int ACT_BYTES = QROWS * ACT_STRIDE, GSH_BYTES = 4 * QROWS * GSH_STRIDE;
constexpr int FWD_LDS = ACT_BYTES > GSH_BYTES ? ACT_BYTES : GSH_BYTES;

// geometry of the BPTT kernel's K blocks under arithmetic AR (see there)
template <int AR> constexpr int q_kbk() { return 32; }                               // k per block (eight 16-bit values per lane)
template <int AR> constexpr int q_nbw() { return QG / q_kbk<AR>() / 4; }             // blocks of one wave's K quarter: 12
template <int AR> constexpr int q_nbm() { return 4 * QU / q_kbk<AR>(); }             // blocks a member owns: 6
template <int AR> constexpr int q_xslot() { return QG / q_kbk<AR>() * 4 * 1024; }    // bytes of one [64 rows][1536] tile in fragment order
template <int AR>
__device__ __forceinline__ fsn_u32x2 q_round4(const f32x4 v) {
    return __builtin_bit_cast(fsn_u32x2, fsn_operand<AR>(v));
}
template <int AR>
__device__ __forceinline__ f32x4 q_mma2(const fsn_u32x4 a, const fsn_u32x4 b, f32x4 c) {  // one K block (32 k) of one tile
    // (round 5: ONE v_mfma_f32_16x16x32_{f16,bf16} - the lane's sixteen bytes ARE that instruction's operand - where
    // rounds 3 - 4 issued two K = 16 instructions, which run at half its rate on gfx950)
    return fsn_mma_k32<AR>(fsn_wfrag_operand<AR>(fsn_u32x2{a[0], a[1]}), fsn_wfrag_operand<AR>(fsn_u32x2{a[2], a[3]}),
                           fsn_wfrag_operand<AR>(fsn_u32x2{b[0], b[1]}), fsn_wfrag_operand<AR>(fsn_u32x2{b[2], b[3]}), c);
}
__device__ __forceinline__ fsn_u32x4 q_lds128(const unsigned char* p) { return *reinterpret_cast<const fsn_u32x4*>(p); }
// four 16-bit values as q_round4 packed them -> fp32 (exact)
template <int AR>
__device__ __forceinline__ f32x4 q_unpack4(const unsigned lo, const unsigned hi) {
    if constexpr (AR == FSN_ARITH_F16) {
        return __builtin_convertvector(__builtin_bit_cast(fsn_f16x4, fsn_u32x2{lo, hi}), f32x4);
    } else {
        return f32x4{__builtin_bit_cast(float, lo << 16), __builtin_bit_cast(float, lo & 0xffff0000u),
                     __builtin_bit_cast(float, hi << 16), __builtin_bit_cast(float, hi & 0xffff0000u)};
    }
}
// (With SV the forward hand-off itself travels in 16 bits: a member's h slice goes write-through into the rows' save slots
// before its flag, the partners copy the [64][H] 16-bit tile straight into LDS - half the exchanged bytes, no conversion - and
// the fp32 hidden sequence is stored after the flag, off the hand-off path.)
// Saved gates in 16 bits (SV = 1; FSN_ARITH_SAVES16): the activated gates i, f, g, o that BPTT re-reads are kept in the
// operand type of the arithmetic - what the vendor's autocast LSTM keeps in its reserve space - inside the SAME buffer: row
// r of step t still owns its 4H x 4 bytes and uses the first half as [unit quad 96][gate 4][4 units] 16-bit, so a thread's
// (row, unit quad) item is 32 contiguous bytes (two 16-byte stores forward, two LDS-DMA pieces backward) and rows that do
// not fill a cluster (step kernels beside the launch, fp32 layout) are untouched.  The cell sequence stays fp32.

// ---- packing ------------------------------------------------------------------------------------------------------
// forward: product W [4H][K] (nn.LSTM's layout, K = k_pad columns, zeros beyond k) -> [member 8][gate 4][K/32][unit
// tile 3][lane 64][8]: lane (lr, lq) of fragment (m, g, kb, j) holds W[g H + 48 m + 16 j + lr][32 kb + 8 lq .. + 7] -
// the A operand of two 16x16x16 matrix instructions whose B operand is row lr's activations at the same k.
template <int AR>
__global__ void q_pack_fwd_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int k, int k_pad) {
    const int kbn = k_pad / 32;
    const long n8 = (long)QG * k_pad / 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        long f = i >> 6;
        const int j = (int)(f % 3);
        f /= 3;
        const int kb = (int)(f % kbn);
        f /= kbn;
        const int g = (int)(f & 3), m = (int)(f >> 2);
        const int row = g * QH + QU * m + 16 * j + (lane & 15), k0 = 32 * kb + 8 * (lane >> 4);
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = k0 + e < k ? w[(long)row * k + k0 + e] : 0.f;
            hi[e] = k0 + 4 + e < k ? w[(long)row * k + k0 + 4 + e] : 0.f;
        }
        const fsn_u32x2 a = q_round4<AR>(lo), b = q_round4<AR>(hi);
        reinterpret_cast<fsn_u32x4*>(out)[i] = fsn_u32x4{a[0], a[1], b[0], b[1]};
    }
}
// BPTT: product W [4H][H] -> [member 8][wave 4][kbl 12][j 3][lane 64][8]: lane (lr, lq) of fragment (m, w, kbl, j) holds
// W[gamma(k')][48 m + 16 j + lr] for k' = 32 (12 w + kbl) + 8 lq + e, e = 0..7, where k' = 192 m' + 48 gate + unit is the K
// position of the exchanged gate gradients (member m' owns a contiguous run) and gamma(k') = gate H + 48 m' + unit the
// gate column behind it; 48 m + 16 j + lr is the output unit (a hidden unit of the step before / of the layer below).
template <int AR>
__global__ void q_pack_bptt_kernel(const float* __restrict__ w, void* __restrict__ out) {
    constexpr int NBW = q_nbw<AR>(), KBK = q_kbk<AR>();
    const long nf = (long)QM * 4 * NBW * 3 * 64;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        long f = i >> 6;
        const int j = (int)(f % 3);
        f /= 3;
        const int kbl = (int)(f % NBW);
        f /= NBW;
        const int wv = (int)(f & 3), m = (int)(f >> 2);
        const int unit = QU * m + 16 * j + (lane & 15), k0 = KBK * (NBW * wv + kbl) + 8 * (lane >> 4);
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int kk = k0 + e, mm = kk / (4 * QU), kl = kk % (4 * QU), col = (kl / QU) * QH + QU * mm + kl % QU;
            v[e] = w[(long)col * QH + unit];
        }
        const fsn_u32x2 a = q_round4<AR>(f32x4{v[0], v[1], v[2], v[3]}), b = q_round4<AR>(f32x4{v[4], v[5], v[6], v[7]});
        reinterpret_cast<fsn_u32x4*>(out)[i] = fsn_u32x4{a[0], a[1], b[0], b[1]};
    }
}

// ---- forward with saves -------------------------------------------------------------------------------------------
// (Tried in round 4 and dropped, profiles/r04_g16_probe_fwd_v2.txt: layer 0 forming layer 1's input projection from its
// own staged tile + a 16-bit h exchange - balanced workgroups, a third of the hand-off bytes, and no faster: 23.2 us per
// step against 22.0.  What bounds the step is the weight stream - 454 KB per CU and step from the Infinity Cache, which
// the 4 MB L2s cannot keep beside the streaming saves - at the bytes a wave can keep in flight in registers.)
struct G16FwdArgs {
    const float* x;        // layer-0 input [Tp][x_step][32] (zero-padded columns)
    long x_step;
    const unsigned short* w16;
    unsigned o_ih0, o_hh0, o_ih1, o_hh1;  // byte offsets of the packed products
    const float *bias0, *bias1;           // b_ih + b_hh [4H]
    float *hseq0, *hseq1;                 // [Tp][Nrows][H]: outputs AND exchange buffers
    float *gates0, *cseq0, *gates1, *cseq1;
    unsigned* flags;                      // [clusters][2][QFS]
    unsigned* status;
    unsigned long long spin_ticks;
    int Tp, Nrows;
};

// XS: the cache policy (scope) of the exchanged payload, FSN_CP_SC1 or - all workgroups of the cluster on one XCD - FSN_CP_SC0
template <int LAYER, int AR, int XS, int SV>
__device__ __forceinline__ void g16_fwd_body(const G16FwdArgs& a, int cluster, int member, unsigned char* act, unsigned char* xsm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int Tp = a.Tp;
    const size_t N = (size_t)a.Nrows;
    unsigned* fl0 = a.flags + ((size_t)cluster * 2 + 0) * QFS;
    unsigned* fl1 = a.flags + ((size_t)cluster * 2 + 1) * QFS;
    const __amdgpu_buffer_rsrc_t wrsrc = fsn_buffer_rsrc(a.w16);
    // this wave's weight stream of a product: fragments (kb, j) at wbase + kb * 3072 + j * 1024 + lane * 16
    auto wbase = [&](unsigned o, int kbn) { return o + (unsigned)((member * 4 + wave) * kbn) * 3072u; };
    const unsigned w_rec = wbase(LAYER ? a.o_hh1 : a.o_hh0, 12), w_in = LAYER ? wbase(a.o_ih1, 12) : wbase(a.o_ih0, 1);
    auto wload = [&](unsigned base, int kb, int j) {
        return fsn_buffer_load<fsn_u32x4>(wrsrc, (unsigned)lane * 16u, base + (unsigned)kb * 3072u + (unsigned)j * 1024u);
    };
    // the cluster's [64][H] tile of step t of a hidden sequence / cell sequence, its [64][4H] tile of a gate buffer
    auto tileh = [&](float* p, int t) { return fsn_buffer_rsrc(p + ((size_t)t * N + (size_t)cluster * QROWS) * QH, QROWS * QH * 4); };
    auto tileg = [&](float* p, int t) { return fsn_buffer_rsrc(p + ((size_t)t * N + (size_t)cluster * QROWS) * QG, QROWS * QG * 4); };

    // bias of this wave's gate for the member's three unit tiles: accumulator row 4 lq + i of tile j = unit 16 j + 4 lq + i
    f32x4 bias[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        bias[j] = *reinterpret_cast<const f32x4*>((LAYER ? a.bias1 : a.bias0) + wave * QH + QU * member + 16 * j + 4 * lq);

    // stage the cluster's [64][H] fp32 tile behind `src` (written through by the partners: sc1 loads) into `act` as 16-bit
    // rows: item q = tid + 256 i is (row q / 48, eight consecutive k)
    auto stage = [&](const __amdgpu_buffer_rsrc_t src) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f32x4 v[12];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int q = tid + 256 * (half * 6 + i), row = q / 48, k8 = q % 48;
                const unsigned go = (unsigned)((row * QH + k8 * 8) * 4);
                v[2 * i] = fsn_buffer_load<f32x4, XS>(src, go, 0);
                v[2 * i + 1] = fsn_buffer_load<f32x4, XS>(src, go, 16);
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int q = tid + 256 * (half * 6 + i), row = q / 48, k8 = q % 48;
                const fsn_u32x2 lo = q_round4<AR>(v[2 * i]), hi = q_round4<AR>(v[2 * i + 1]);
                *reinterpret_cast<fsn_u32x4*>(act + row * ACT_STRIDE + k8 * 16) = fsn_u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
        }
    };
    // SV: the hand-off travels in 16 bits - a member writes its h slice through (same scope) into the second half of the rows'
    // save slots BEFORE its flag; the partners copy [64][H] 16-bit values (half the bytes, no conversion) straight into `act`.
    // `g` = the layer's gate-save buffer, step t.  (Rounded at the producer or at the consumer's matrix input: the same number.)
    auto stage16 = [&](float* g, int t) {
        const __amdgpu_buffer_rsrc_t src = fsn_buffer_rsrc(g + ((size_t)t * N + (size_t)cluster * QROWS) * QG, QROWS * QG * 4);
        fsn_u32x4 v[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int q = tid + 256 * i, row = q / 48, k8 = q % 48;
            v[i] = fsn_buffer_load<fsn_u32x4, XS>(src, (unsigned)(row * QG * 4 + Q_H16_OFF + k8 * 16), 0);
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int q = tid + 256 * i, row = q / 48, k8 = q % 48;
            *reinterpret_cast<fsn_u32x4*>(act + row * ACT_STRIDE + k8 * 16) = v[i];
        }
    };
    // acc += W(gate `wave` of the member's 48 units x K) act^T: twelve K blocks, the wave's own weight stream through a
    // ring of QD blocks whose first turn `ring` was requested by the caller (before the hand-off wait)
    auto kloop12 = [&](f32x4 (&acc)[3][4], fsn_u32x4 (&ring)[QD][3], unsigned base) {
#pragma unroll
        for (int kb0 = 0; kb0 < 12; kb0 += QD) {
#pragma unroll
            for (int d = 0; d < QD; ++d) {
                const int kb = kb0 + d;
                fsn_u32x4 wf[3], af[4];
#pragma unroll
                for (int j = 0; j < 3; ++j) wf[j] = ring[d][j];
                if (kb + QD < 12) {
                    __builtin_amdgcn_sched_barrier(0);  // the refill goes out before this block's matrix work
#pragma unroll
                    for (int j = 0; j < 3; ++j) ring[d][j] = wload(base, kb + QD, j);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) af[r] = q_lds128(act + (16 * r + lr) * ACT_STRIDE + kb * 64 + lq * 16);
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[j][r] = q_mma2<AR>(wf[j], af[r], acc[j][r]);
            }
        }
    };
    auto ring_start = [&](fsn_u32x4 (&ring)[QD][3], unsigned base) {
#pragma unroll
        for (int d = 0; d < QD; ++d)
#pragma unroll
            for (int j = 0; j < 3; ++j) ring[d][j] = wload(base, d, j);
    };

    // elementwise items of this thread: q = tid + 256 e -> (row q / 12, unit quad q % 12); cell state in registers
    f32x4 c[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) c[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    float* const hseq = LAYER ? a.hseq1 : a.hseq0;
    float* const gates = LAYER ? a.gates1 : a.gates0;
    float* const cseq = LAYER ? a.cseq1 : a.cseq0;
    unsigned* const myflag = (LAYER ? fl1 : fl0) + member;

    for (int t = 0; t < Tp; ++t) {
        f32x4 acc[3][4];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = bias[j];
        fsn_u32x4 ring[QD][3];
        if (LAYER == 0) {
            // x_t (64 rows x 32 columns, the caller's tensor: plain loads) -> xsm; its three weight fragments
            fsn_u32x4 wx[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) wx[j] = wload(w_in, 0, j);
            if (t > 0) ring_start(ring, w_rec);
            {
                const int row = tid >> 2, k8 = tid & 3;
                const float* xp = a.x + ((size_t)t * a.x_step + (size_t)cluster * QROWS + row) * 32 + k8 * 8;
                const fsn_u32x2 lo = q_round4<AR>(*reinterpret_cast<const f32x4*>(xp));
                const fsn_u32x2 hi = q_round4<AR>(*reinterpret_cast<const f32x4*>(xp + 4));
                *reinterpret_cast<fsn_u32x4*>(xsm + row * X_STRIDE + k8 * 16) = fsn_u32x4{lo[0], lo[1], hi[0], hi[1]};
            }
            if (t > 0) {
                fsn_group_wait<QM>(fl0, (unsigned)t, a.status, a.spin_ticks);  // h0_{t-1} of all members
                if constexpr (SV != 0) stage16(a.gates0, t - 1);
                else stage(tileh(a.hseq0, t - 1));
            }
            __syncthreads();
            {
                fsn_u32x4 af[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) af[r] = q_lds128(xsm + (16 * r + lr) * X_STRIDE + lq * 16);
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[j][r] = q_mma2<AR>(wx[j], af[r], acc[j][r]);
            }
            if (t > 0) kloop12(acc, ring, w_rec);
        } else {
            // x_t W_ih1^T first: it needs h0_t, which layer 0 published long ago; then h1_{t-1} W_hh1^T
            ring_start(ring, w_in);
            fsn_group_wait<QM>(fl0, (unsigned)t + 1, a.status, a.spin_ticks);
            if constexpr (SV != 0) stage16(a.gates0, t);
            else stage(tileh(a.hseq0, t));
            __syncthreads();
            kloop12(acc, ring, w_in);
            if (t > 0) {
                ring_start(ring, w_rec);
                fsn_group_wait<QM>(fl1, (unsigned)t, a.status, a.spin_ticks);  // h1_{t-1} of all members; also: everyone has left `act`
                if constexpr (SV != 0) stage16(a.gates1, t - 1);
                else stage(tileh(a.hseq1, t - 1));
                __syncthreads();
                kloop12(acc, ring, w_rec);
            }
        }
        __syncthreads();  // every wave has left `act`: the gate exchange takes its place
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<f32x4*>(act + (wave * QROWS + 16 * r + lr) * GSH_STRIDE + (16 * j + 4 * lq) * 4) = acc[j][r];
        __syncthreads();
        f32x4 sg[3][4];  // activated gates of this thread's items, kept for the saves
        const __amdgpu_buffer_rsrc_t rh = tileh(hseq, t), rg = tileg(gates, t);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int q = tid + 256 * e, row = q / 12, quad = q % 12;
            f32x4 pre[4], hv;
#pragma unroll
            for (int g = 0; g < 4; ++g) pre[g] = *reinterpret_cast<const f32x4*>(act + (g * QROWS + row) * GSH_STRIDE + quad * 16);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ig = sigmoid_fast(pre[0][i]), fg = sigmoid_fast(pre[1][i]);
                const float gg = tanh_fast(pre[2][i]), og = sigmoid_fast(pre[3][i]);
                const float cn = fg * c[e][i] + ig * gg;
                c[e][i] = cn;
                hv[i] = og * tanh_fast(cn);
                sg[e][0][i] = ig, sg[e][1][i] = fg, sg[e][2][i] = gg, sg[e][3][i] = og;
            }
            if constexpr (SV != 0)
                fsn_buffer_store<XS>(rg, (unsigned)(row * QG * 4 + Q_H16_OFF + (QU * member + quad * 4) * 2), 0, q_round4<AR>(hv));
            else fsn_buffer_store<XS>(rh, (unsigned)((row * QH + QU * member + quad * 4) * 4), 0, hv);
        }
        fsn_publish(myflag, (unsigned)t + 1);  // its barrier also closes the reads of the gate exchange
        // the saves of the step, AFTER the hand-off (only h belongs to it)
        const __amdgpu_buffer_rsrc_t rc = tileh(cseq, t);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int q = tid + 256 * e, row = q / 12, quad = q % 12;
            const unsigned go = (unsigned)((row * QG + QU * member + quad * 4) * 4);
            if constexpr (SV != 0) {
                const unsigned so = (unsigned)(row * QG * 4 + (12 * member + quad) * 32);
                const fsn_u32x2 pi = q_round4<AR>(sg[e][0]), pf = q_round4<AR>(sg[e][1]);
                const fsn_u32x2 pg = q_round4<AR>(sg[e][2]), po = q_round4<AR>(sg[e][3]);
                fsn_buffer_store(rg, so, 0, fsn_u32x4{pi[0], pi[1], pf[0], pf[1]});
                fsn_buffer_store(rg, so, 16, fsn_u32x4{pg[0], pg[1], po[0], po[1]});
                // (h_t in 16 bits sits behind them, second half of the row's slot, [H] values: the hand-off above - and the B
                // operand of two weight-gradient products, which need no conversion pass over the hidden sequence.)  The
                // fp32 hidden sequence, off the hand-off path: recomputed from o and c, the very value that was rounded
                f32x4 hv;
#pragma unroll
                for (int i = 0; i < 4; ++i) hv[i] = sg[e][3][i] * tanh_fast(c[e][i]);
                fsn_buffer_store(rh, (unsigned)((row * QH + QU * member + quad * 4) * 4), 0, hv);
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) fsn_buffer_store(rg, go, (unsigned)(g * QH * 4), sg[e][g]);
            }
            fsn_buffer_store(rc, (unsigned)((row * QH + QU * member + quad * 4) * 4), 0, c[e]);
        }
    }
}

template <int AR, int SV = 0>
__global__ __launch_bounds__(256, 2) void lstm2_g16_fwd_kernel(const G16FwdArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char act[FWD_LDS];
    __shared__ __attribute__((aligned(16))) unsigned char xsm[QROWS * X_STRIDE];
    // first half of the grid: layer 0, second half: layer 1 - blocks are handed out in order, one per CU before any CU
    // gets its second, so a CU ends up with one workgroup of each layer; the members of a cluster on one XCD (block b
    // runs on XCD b % 8, observed) when the cluster count allows it.  Speed only.
    const int half = gridDim.x >> 1;
    const int layer = (int)blockIdx.x >= half ? 1 : 0;
    const int bid = (int)blockIdx.x - layer * half;
    const int nclusters = half / QM;
    int cluster, member;
    if (nclusters % 8 == 0) {
        const int xcd = bid & 7, j = bid >> 3;
        cluster = xcd * (nclusters / 8) + j / QM;
        member = j % QM;
    } else {
        cluster = bid / QM;
        member = bid % QM;
    }
    // Placement check: every workgroup reports the XCD it runs on (HW_REG_XCC_ID) and reads its cluster's sixteen reports;
    // only when all agree is the payload exchanged at XCD scope (XS = FSN_CP_SC0: 9 % of the launch, the partners' tiles come from
    // the shared L2 instead of through the fabric).  Any other placement - or a timeout - takes the device-scope path:
    // results never depend on where the workgroups run.
    bool same_xcd = false;
    {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc = (xcc & 0xfu) + 1u;
        unsigned* reports = a.flags + (size_t)nclusters * 2 * QFS + (size_t)cluster * QFS;  // [layer][member], zeroed by the host
        unsigned* agree = reinterpret_cast<unsigned*>(xsm);
        if (threadIdx.x == 0) __hip_atomic_store(reports + layer * QM + member, xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((threadIdx.x >> 6) == 0) {
            const int lane = threadIdx.x & 63;
            unsigned long long t0 = 0;
            unsigned v = xcc;
            for (unsigned spins = 0;; ++spins) {
                if (lane < 2 * QM) v = __hip_atomic_load(reports + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (__all((int)(v != 0u))) break;
                if ((spins & 255u) == 255u && fsn_wait_give_up(a.status, spins, t0, a.spin_ticks, 0x7000u)) {
                    v = 0u;
                    break;
                }
                __builtin_amdgcn_s_sleep(1);
            }
            const bool ok = __all((int)(v == xcc));
            if (lane == 0) *agree = ok ? 1u : 0u;
        }
        __syncthreads();
        same_xcd = *agree != 0u;
        __syncthreads();  // (xsm is the layer-0 input tile afterwards)
    }
    if (same_xcd) {
        if (layer == 0) g16_fwd_body<0, AR, FSN_CP_SC0, SV>(a, cluster, member, act, xsm);
        else g16_fwd_body<1, AR, FSN_CP_SC0, SV>(a, cluster, member, act, xsm);
    } else {
        if (layer == 0) g16_fwd_body<0, AR, FSN_CP_SC1, SV>(a, cluster, member, act, xsm);
        else g16_fwd_body<1, AR, FSN_CP_SC1, SV>(a, cluster, member, act, xsm);
    }
}

// ---- back-propagation through time --------------------------------------------------------------------------------
// Per step t = T-1 .. 0 (formulas: bptt_step_kernels.hip):
//   layer 1: dh1_t = dH1_t + dgates1_{t+1} W_hh1;   layer 0: dh0_t = dgates1_t W_ih1 + dgates0_{t+1} W_hh0
// Member m owns the 48 units [48 m, 48 m + 48) of dh for the cluster's 64 rows, transposed: D^T[unit][row] = sum over ALL
// 1536 gate columns.  The gate gradients travel between members as a 16-BIT copy in matrix-operand FRAGMENT order -
// X[cluster][slot][K block 48][row tile 4][lane 64][8 values], K position k' = 192 m' + 48 gate + unit: member m' owns
// blocks 6 m' .. 6 m' + 5 and writes them as six fully coalesced 16-byte write-through stores per thread; rounding to 16
// bits at the producer or at the consumer's matrix input is the same number - so a consumer wave's operand load is ONE
// contiguous 1 KB line group, straight into registers: no LDS staging, no conversion, and the eight members of a cluster
// (one XCD when the grid allows it) share each tile through that XCD's L2 (196 KB per cluster, layer and step through the
// fabric, where per-member partial sums cost 1.5 MB - measured: profiles/r04_g16_probe_v1.txt).  The four waves split K
// (twelve blocks each, own weight stream, own operand stream) and meet once per step in a fixed-order LDS reduction.
// Layer 0 forms dgates1_t W_ih1 itself, from layer 1's tile (published well ahead: off its recurrent chain).
// (An fp32 instantiation of this kernel - 16 k per block, the tile exchanged in fp32 - was built and measured in round 4:
// 69 us per step against the fp32-era kernel's 72: with fp32 operands the step is bound by the fabric either way, 0.5 GB
// of tiles and weight fragments per step that the 4 MB L2s cannot hold, so the fp32 arithmetic stays on
// lstm_group_bptt_kernels.hip; profiles/r04_g16_probe_bptt_f32.txt.)
constexpr int QAD = 4;                  // operand blocks in flight per wave (4 fragments each)
constexpr int QWD = 4;                  // weight blocks in flight per wave (3 fragments each)
template <int AR>
__device__ __forceinline__ f32x4 q_mma_blk(const fsn_u32x4 a, const fsn_u32x4 b, f32x4 c) { return q_mma2<AR>(a, b, c); }

struct G16BwdArgs {
    const float* dh1;      // [Tp][N][H]  d loss / d hseq1
    const void* w16;       // packed 16-bit weights
    unsigned o_hh1, o_ih1, o_hh0;  // byte offsets of the packed products (q_pack_bptt_kernel)
    const float *gates0, *cseq0, *gates1, *cseq1;
    float *dg0, *dg1;      // [Tp][N][4H] gate gradients (outputs)
    void *x1, *x0;         // [clusters][QDX][q_xslot bytes]: the gate gradients of the last steps, fragment order
    unsigned short *dg16_0, *dg16_1;  // [Tp][N][4H] 16-bit gate gradients, row-major: operands of the weight-gradient products
    float* dbp;            // [2 layers][clusters][4H]: column sums of this launch's gate gradients (fp32 values): the bias gradients
    int dg1_f32;           // 0: layer 1's fp32 gate gradients are not stored (nothing reads them: the products take dg16_1)
    int dg0_f32;           // 0: nor layer 0's (dx and dW_ih0 take dg16_0 too: gemm_dx16_kernel, gemm_tn16n_kernel)
    unsigned* flags;       // [clusters][2][QFS]: steps published by (layer 1 | layer 0, member)
    unsigned* status;
    unsigned long long spin_ticks;
    int Tp, Nrows;
};

template <int LAYER, int AR, int SV>
__device__ __forceinline__ void g16_bwd_body(const G16BwdArgs& a, int cluster, int member, unsigned char* red, unsigned char* dsh,
                                             float (*dbs)[4 * QU]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int Tp = a.Tp;
    const size_t N = (size_t)a.Nrows;
    unsigned* fl1 = a.flags + ((size_t)cluster * 2 + 0) * QFS;
    unsigned* fl0 = a.flags + ((size_t)cluster * 2 + 1) * QFS;
    const __amdgpu_buffer_rsrc_t wrsrc = fsn_buffer_rsrc(a.w16);
    // this wave's weight stream of a product: fragments (kbl, j) at base + kbl * 3072 + j * 1024 + lane * 16
    constexpr int NBW = q_nbw<AR>(), NBM = q_nbm<AR>(), XSLOT = q_xslot<AR>();
    auto wbase = [&](unsigned o) { return o + (unsigned)((member * 4 + wave) * NBW) * 3072u; };
    auto wload = [&](unsigned base, int kbl, int j) {
        return fsn_buffer_load<fsn_u32x4>(wrsrc, (unsigned)lane * 16u, base + (unsigned)kbl * 3072u + (unsigned)j * 1024u);
    };
    auto wait = [&](unsigned* f8, unsigned epoch) { fsn_group_wait<QM>(f8, epoch, a.status, a.spin_ticks); };
    auto tileh = [&](const float* p, int t) { return fsn_buffer_rsrc(p + ((size_t)t * N + (size_t)cluster * QROWS) * QH, QROWS * QH * 4); };
    auto tileg = [&](const float* p, int t) { return fsn_buffer_rsrc(p + ((size_t)t * N + (size_t)cluster * QROWS) * QG, QROWS * QG * 4); };
    const __amdgpu_buffer_rsrc_t rx1 = fsn_buffer_rsrc(reinterpret_cast<const unsigned char*>(a.x1) + (size_t)cluster * QDX * XSLOT, (unsigned)QDX * XSLOT);
    const __amdgpu_buffer_rsrc_t rx0 = fsn_buffer_rsrc(reinterpret_cast<const unsigned char*>(a.x0) + (size_t)cluster * QDX * XSLOT, (unsigned)QDX * XSLOT);
    const __amdgpu_buffer_rsrc_t rxo = LAYER ? rx1 : rx0;
    // elementwise mapping = accumulator layout of the transposed product after the reduction: wave = row tile, lane (lr, lq)
    // = row 16 w + lr, for unit tile j = 0..2 of this member the four units 48 m + 16 j + 4 lq .. + 3
    const unsigned eo_h = (unsigned)((((wave * 16 + lr) * QH) + QU * member + 4 * lq) * 4);  // + j * 64
    const unsigned eo_g = (unsigned)((((wave * 16 + lr) * QG) + QU * member + 4 * lq) * 4);  // + g * H * 4 + j * 64

    // acc += W^T(this member's 48 units x this wave's twelve K blocks) x (the tile behind `rx`, slot offset `xo`)^T.  The
    // first QWD blocks of weight fragments were requested by the caller (before the hand-off wait); the operand ring
    // starts here, after it.
    auto kloop = [&](f32x4 (&acc)[3][4], fsn_u32x4 (&wring)[QWD][3], unsigned wb, const __amdgpu_buffer_rsrc_t rx, unsigned xo) {
        auto xload = [&](int kbl, int r) {
            return fsn_buffer_load<fsn_u32x4, FSN_CP_SC1>(rx, (unsigned)lane * 16u, xo + (unsigned)(((wave * NBW + kbl) * 4 + r) * 1024));
        };
        fsn_u32x4 aring[QAD][4];
#pragma unroll
        for (int d = 0; d < QAD; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) aring[d][r] = xload(d, r);
#pragma unroll
        for (int kb0 = 0; kb0 < NBW; kb0 += QAD) {
#pragma unroll
            for (int d = 0; d < QAD; ++d) {
                const int kbl = kb0 + d;
                fsn_u32x4 wf[3], af[4];
#pragma unroll
                for (int j = 0; j < 3; ++j) wf[j] = wring[d][j];
#pragma unroll
                for (int r = 0; r < 4; ++r) af[r] = aring[d][r];
                if (kbl + QAD < NBW) {
                    __builtin_amdgcn_sched_barrier(0);  // the refills go out before this block's matrix work
#pragma unroll
                    for (int j = 0; j < 3; ++j) wring[d][j] = wload(wb, kbl + QWD, j);
#pragma unroll
                    for (int r = 0; r < 4; ++r) aring[d][r] = xload(kbl + QAD, r);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[j][r] = q_mma_blk<AR>(wf[j], af[r], acc[j][r]);
            }
        }
    };
    static_assert(QAD == QWD && NBW % QAD == 0, "the two rings turn together, in whole turns");
    auto wring_start = [&](fsn_u32x4 (&wring)[QWD][3], unsigned wb) {
#pragma unroll
        for (int d = 0; d < QWD; ++d)
#pragma unroll
            for (int j = 0; j < 3; ++j) wring[d][j] = wload(wb, d, j);
    };

    const float* const gates = LAYER ? a.gates1 : a.gates0;
    const float* const cseq = LAYER ? a.cseq1 : a.cseq0;
    float* const dgout = LAYER ? a.dg1 : a.dg0;
    unsigned* const myfl = LAYER ? fl1 : fl0;
    const unsigned w_hh = wbase(LAYER ? a.o_hh1 : a.o_hh0), w_ih = wbase(a.o_ih1);
    unsigned short* const dg16 = LAYER ? a.dg16_1 : a.dg16_0;
    for (int i = threadIdx.x; i < 4 * 4 * QU; i += 256) dbs[0][i] = 0.f;  // [wave][gate 48 + unit]: this member's bias-gradient sums
    f32x4 dc[3], c_t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) dc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
        const __amdgpu_buffer_rsrc_t rc = tileh(cseq, Tp - 1);
#pragma unroll
        for (int j = 0; j < 3; ++j) c_t[j] = fsn_buffer_load<f32x4>(rc, eo_h, (unsigned)(j * 64));
    }

    for (int t = Tp - 1; t >= 0; --t) {
        const unsigned done = (unsigned)(Tp - 1 - t);  // steps every member has completed when step t + 1 is
        f32x4 acc[3][4];
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = f32x4{0.f, 0.f, 0.f, 0.f};
        // The saved activations of step t do not depend on any hand-off: requested FIRST.  The gates (12 fragments per
        // lane) by LDS-DMA into this wave's own 12 KB of `red` - no registers while the K loops run; they are read back
        // after the loops and before the wave's partial sums take their place - c_{t-1} and (layer 1) dH1_t into registers.
        const unsigned red_w = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)red + (unsigned)wave * 12u * 1024u;  // LDS byte address of this wave's region
        f32x4 sg[3][4], c_p[3], dh[3];
        {
            const float* gp = gates + ((size_t)t * N + (size_t)cluster * QROWS + wave * 16 + lr) * QG + QU * member + 4 * lq;
            if constexpr (SV != 0) {  // 16-bit saves: a lane's (row, unit quad) item = 32 bytes = two pieces
                const unsigned char* gp16 = reinterpret_cast<const unsigned char*>(gates) +
                                            ((size_t)t * N + (size_t)cluster * QROWS + wave * 16 + lr) * (QG * 4) + (12 * member + lq) * 32;
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int p = 0; p < 2; ++p)
                        fsn_lds_dma(gp16 + j * 128 + p * 16, red_w + (unsigned)((j * 2 + p) * 1024));
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) fsn_lds_dma(gp + g * QH + 16 * j, red_w + (unsigned)((j * 4 + g) * 1024));
            }
            const __amdgpu_buffer_rsrc_t rp = tileh(cseq, t > 0 ? t - 1 : 0), rd = tileh(LAYER ? a.dh1 : cseq, t);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                c_p[j] = t > 0 ? fsn_buffer_load<f32x4>(rp, eo_h, (unsigned)(j * 64)) : f32x4{0.f, 0.f, 0.f, 0.f};
                dh[j] = LAYER ? fsn_buffer_load<f32x4>(rd, eo_h, (unsigned)(j * 64)) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        fsn_u32x4 wring[QWD][3];
        if (LAYER == 0) {  // dgates1_t W_ih1: layer 1 published step t as its flag value done + 1
            wring_start(wring, w_ih);
            wait(fl1, done + 1);
            kloop(acc, wring, w_ih, rx1, (unsigned)((t % QDX) * XSLOT));
        }
        if (t < Tp - 1) {  // dgates_{t+1} W_hh of the own layer
            wring_start(wring, w_hh);
            wait(myfl, done);
            kloop(acc, wring, w_hh, rxo, (unsigned)(((t + 1) % QDX) * XSLOT));
        }
        // the gates have landed long ago (the DMA is older than every load the K loops consumed); say so, read them back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (SV != 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const fsn_u32x4 v0 = q_lds128(red + (wave * 12 + j * 2) * 1024 + lane * 16);
                const fsn_u32x4 v1 = q_lds128(red + (wave * 12 + j * 2 + 1) * 1024 + lane * 16);
                sg[j][0] = q_unpack4<AR>(v0[0], v0[1]), sg[j][1] = q_unpack4<AR>(v0[2], v0[3]);
                sg[j][2] = q_unpack4<AR>(v1[0], v1[1]), sg[j][3] = q_unpack4<AR>(v1[2], v1[3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) sg[j][g] = *reinterpret_cast<const f32x4*>(red + (wave * 12 + j * 4 + g) * 1024 + lane * 16);
        }
        // the four waves' K quarters meet: wave w' takes row tile w', sums the sources in a fixed order
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) *reinterpret_cast<f32x4*>(red + ((wave * 12 + j * 4 + r) * 64 + lane) * 16) = acc[j][r];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int src = 0; src < 4; ++src) dh[j] += *reinterpret_cast<const f32x4*>(red + ((src * 12 + j * 4 + wave) * 64 + lane) * 16);
        // cell derivative of this thread's 3 x 4 elements -> gate gradients of step t: fp32 to memory (the weight-gradient
        // products read them afterwards) and, rounded to 16 bits, into this member's [64][192] tile for the exchange
        const __amdgpu_buffer_rsrc_t ro = tileg(dgout, t);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            f32x4 d_i, d_f, d_g, d_o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float ig = sg[j][0][i], fg = sg[j][1][i], gg = sg[j][2][i], og = sg[j][3][i];
                const float tc = tanhf(c_t[j][i]);
                const float dhv = dh[j][i];
                const float dct = dc[j][i] + dhv * og * (1.f - tc * tc);
                d_i[i] = dct * gg * ig * (1.f - ig);
                d_f[i] = dct * c_p[j][i] * fg * (1.f - fg);
                d_g[i] = dct * ig * (1.f - gg * gg);
                d_o[i] = dhv * tc * og * (1.f - og);
                dc[j][i] = dct * fg;
            }
            sg[j][0] = d_i, sg[j][1] = d_f, sg[j][2] = d_g, sg[j][3] = d_o;  // kept for the fp32 stores after the hand-off
            unsigned char* dp = dsh + (wave * 16 + lr) * DSH_STRIDE + (16 * j + 4 * lq) * 2;
            *reinterpret_cast<fsn_u32x2*>(dp) = q_round4<AR>(d_i);
            *reinterpret_cast<fsn_u32x2*>(dp + QU * 2) = q_round4<AR>(d_f);
            *reinterpret_cast<fsn_u32x2*>(dp + 2 * QU * 2) = q_round4<AR>(d_g);
            *reinterpret_cast<fsn_u32x2*>(dp + 3 * QU * 2) = q_round4<AR>(d_o);
            c_t[j] = c_p[j];  // c_{t-1} is the next iteration's c_t
        }
        // exchange: this member's K blocks x four row tiles of step t's tile, one 1 KB fragment per wave and store.
        // Layer 1's slot still holds step t + QDX until every layer-0 member has read it, i.e. completed that step
        __syncthreads();
        if (LAYER && done >= (unsigned)QDX) wait(fl0, done - QDX + 1);
#pragma unroll
        for (int kbl = 0; kbl < NBM; ++kbl) {
            const fsn_u32x4 v = q_lds128(dsh + (wave * 16 + lr) * DSH_STRIDE + kbl * 64 + lq * 16);
            fsn_buffer_store<FSN_CP_SC1>(rxo, (unsigned)lane * 16u, (unsigned)((t % QDX) * XSLOT + ((NBM * member + kbl) * 4 + wave) * 1024), v);
        }
        fsn_publish(myfl + member, done + 1);  // its barrier also closes this step's use of `red` and `dsh`
        // AFTER the hand-off (only the fragment-order tile belongs to it): the gate gradients for the products that follow
        // the launch - 16-bit row-major copies [t][row][4H] (the weight-gradient products' operand: rounding here or at their
        // matrix input is the same number), fp32 for layer 0 (its input gradient is an fp32 product) - and their column sums
        // (the bias gradients, from the fp32 values): the 16 rows of a wave summed by DPP, one lane per unit quad adds to LDS
        const __amdgpu_buffer_rsrc_t r16 = fsn_buffer_rsrc(dg16 + ((size_t)t * N + (size_t)cluster * QROWS) * QG, QROWS * QG * 2);
        const unsigned eo_16 = (unsigned)((((wave * 16 + lr) * QG) + QU * member + 4 * lq) * 2);
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (LAYER ? a.dg1_f32 : a.dg0_f32) fsn_buffer_store(ro, eo_g, (unsigned)(g * QH * 4 + j * 64), sg[j][g]);
                fsn_buffer_store(r16, eo_16, (unsigned)((g * QH + j * 16) * 2), q_round4<AR>(sg[j][g]));
                fsn_hold_store_data(sg[j][g]);  // the sums below may be formed in the store's data registers
                f32x4 v = sg[j][g];
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // sum over the 16 lanes lr of this lane's group: quad xor 1, xor 2, half mirror, mirror
                    float x = v[i];
                    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, true));
                    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, true));
                    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x141, 0xF, 0xF, true));
                    x += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0x140, 0xF, 0xF, true));
                    v[i] = x;
                }
                if (lr == 0) {
                    f32x4* d = reinterpret_cast<f32x4*>(&dbs[wave][g * QU + 16 * j + 4 * lq]);
                    *d += v;
                }
            }
    }
    // the member's bias-gradient sums: the four waves' (row tiles') accumulators in a fixed order
    __syncthreads();
    if (threadIdx.x < 4 * QU) {
        const int k = threadIdx.x;
        const float v = ((dbs[0][k] + dbs[1][k]) + dbs[2][k]) + dbs[3][k];
        a.dbp[((size_t)LAYER * (gridDim.x / (2 * QM)) + cluster) * QG + (k / QU) * QH + QU * member + k % QU] = v;
    }
}

template <int AR, int SV = 0>
__global__ __launch_bounds__(256, 2) void lstm2_g16_bwd_kernel(const G16BwdArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char red[4 * 12 * 1024];
    __shared__ __attribute__((aligned(16))) unsigned char dsh[QROWS * DSH_STRIDE];
    __shared__ __attribute__((aligned(16))) float dbs[4][4 * QU];
    // first half of the grid: layer 1 (the leading chain), second half: layer 0; cluster members on one XCD when the
    // cluster count allows it (speed only: they then share the exchanged tiles through that XCD's L2)
    const int half = gridDim.x >> 1;
    const int second = (int)blockIdx.x >= half ? 1 : 0;
    const int bid = (int)blockIdx.x - second * half;
    const int nclusters = half / QM;
    int cluster, member;
    if (nclusters % 8 == 0) {
        const int xcd = bid & 7, j = bid >> 3;
        cluster = xcd * (nclusters / 8) + j / QM;
        member = j % QM;
    } else {
        cluster = bid / QM;
        member = bid % QM;
    }
    if (!second) g16_bwd_body<1, AR, SV>(a, cluster, member, red, dsh, dbs);
    else g16_bwd_body<0, AR, SV>(a, cluster, member, red, dsh, dbs);
}

// After the launch: the rows that did not fill a cluster (computed step by step beside it, fp32) need their 16-bit copies ...
template <int AR>
__global__ void g16_left_to16_kernel(const float* __restrict__ dg, unsigned short* __restrict__ dg16, int T, long N, long row0, int left) {
    const long per_t = (long)left * QG / 4, n4 = (long)T * per_t;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const long t = i / per_t, o = ((t * N + row0) * QG) + (i % per_t) * 4;
        *reinterpret_cast<fsn_u32x2*>(dg16 + o) = q_round4<AR>(*reinterpret_cast<const f32x4*>(dg + o));
    }
}
// ... and the bias gradient is the clusters' sums (fixed order) plus those rows' fp32 gate gradients
__global__ void g16_db_kernel(const float* __restrict__ dbp, int clusters, const float* __restrict__ dg, int T, long N, long row0,
                              int left, float* __restrict__ db) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= QG) return;
    float acc = 0.f;
    for (int c = 0; c < clusters; ++c) acc += dbp[(size_t)c * QG + col];
    for (int t = 0; t < T; ++t)
        for (int r = 0; r < left; ++r) acc += dg[((long)t * N + row0 + r) * QG + col];
    db[col] = acc;
}

}  // namespace

// ---- host side ------------------------------------------------------------------------------------------------------
// clusters these kernels can take for `tiles` 16-row tiles: whole 64-row clusters, one per eight CUs at most, two
// workgroups per CU by the compiled kernels' occupancy (residency contract)
int fsn_lstm2_g16_clusters(int tiles) {
    int cus = 0, dev = 0;
    if (!fsn_persistent_allowed() || hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    for (const void* k : {(const void*)lstm2_g16_fwd_kernel<FSN_ARITH_F16>, (const void*)lstm2_g16_fwd_kernel<FSN_ARITH_BF16>,
                          (const void*)lstm2_g16_bwd_kernel<FSN_ARITH_F16>, (const void*)lstm2_g16_bwd_kernel<FSN_ARITH_BF16>,
                          (const void*)lstm2_g16_fwd_kernel<FSN_ARITH_F16, 1>, (const void*)lstm2_g16_fwd_kernel<FSN_ARITH_BF16, 1>,
                          (const void*)lstm2_g16_bwd_kernel<FSN_ARITH_F16, 1>, (const void*)lstm2_g16_bwd_kernel<FSN_ARITH_BF16, 1>})
        if (!fsn_grid_fits(k, 256, 2u * (unsigned)cus)) return 0;
    const int cap = cus / QM, c = tiles / 4;
    return c < cap ? c : cap;
}
size_t fsn_lstm2_g16_flag_words(int clusters) { return (size_t)clusters * 3 * QFS + 16; }
size_t fsn_lstm2_g16_status_word(int clusters) { return (size_t)clusters * 3 * QFS; }
// the two rings of exchanged gate-gradient tiles (floats of scratch), the packed weights (bytes of scratch)
size_t fsn_lstm2_g16_partial_floats(int clusters) { return (size_t)clusters * 2 * QDX * (q_xslot<FSN_ARITH_F16>() / 4); }
size_t fsn_lstm2_g16_bwd_weight_bytes() { return (size_t)3 * QG * QH * 2; }
size_t fsn_lstm2_g16_fwd_weight_halves(int Ipad) { return (size_t)QG * Ipad + (size_t)3 * QG * QH; }

template <int AR>
static int g16_pack_fwd(const float* w, unsigned short* out, int k, int k_pad, hipStream_t s) {
    const long n8 = (long)QG * k_pad / 8;
    hipLaunchKernelGGL(q_pack_fwd_kernel<AR>, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, w, out, k, k_pad);
    return fsn_check_launch("q_pack_fwd_kernel");
}
template <int AR>
static int g16_pack_bptt(const float* w, void* out, hipStream_t s) {
    const long nf = (long)QM * 4 * q_nbw<AR>() * 3 * 64;
    hipLaunchKernelGGL(q_pack_bptt_kernel<AR>, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, w, out);
    return fsn_check_launch("q_pack_bptt_kernel");
}
template <int AR>
static int g16_launch_bptt(G16BwdArgs a, const float* w_hh1, const float* w_ih1, const float* w_hh0, void* wbuf, float* exchange,
                           int clusters, hipStream_t s, bool saves16) {
    const size_t wb = (size_t)QG * QH * 2;
    unsigned char* p = static_cast<unsigned char*>(wbuf);
    int rc;
    if ((rc = g16_pack_bptt<AR>(w_hh1, p, s)) || (rc = g16_pack_bptt<AR>(w_ih1, p + wb, s)) || (rc = g16_pack_bptt<AR>(w_hh0, p + 2 * wb, s)))
        return rc;
    a.w16 = p;
    a.o_hh1 = 0;
    a.o_ih1 = (unsigned)wb;
    a.o_hh0 = (unsigned)(2 * wb);
    a.x1 = exchange;
    a.x0 = reinterpret_cast<unsigned char*>(exchange) + (size_t)clusters * QDX * q_xslot<AR>();
    const dim3 grid((unsigned)clusters * QM * 2), block(256);
    if (saves16) FSN_PERSIST_LAUNCH((lstm2_g16_bwd_kernel<AR, 1>), grid, block, s, a);
    else FSN_PERSIST_LAUNCH(lstm2_g16_bwd_kernel<AR>, grid, block, s, a);
    return fsn_check_launch("lstm2_g16_bwd_kernel");
}

// Rows [0, 64 clusters) of two stacked LSTM layers, forward with saves, 16-bit operands.  x [Tp][Nrows][32] (zero-padded
// columns beyond I); w_* the UNPACKED nn.LSTM tensors; bias0 / bias1 = b_ih + b_hh [4H]; w16: scratch of
// fsn_lstm2_g16_fwd_weight_halves(32) 16-bit words; flags: fsn_lstm2_g16_flag_words(clusters) words.
int fsn_launch_lstm2_g16_train(const float* x, int I, int Nrows, const float* w_ih0, const float* w_hh0, const float* w_ih1,
                               const float* w_hh1, const float* bias0, const float* bias1, float* hseq0, float* hseq1,
                               float* save0, float* save1, unsigned* flags, void* w16, int Tp, int clusters, int H,
                               hipStream_t s, int arith) {
    const bool saves16 = (arith & FSN_ARITH_SAVES16) != 0;  // the activated gates saved in the 16-bit type (include/fsn_hip.h)
    arith &= ~FSN_ARITH_SAVES16;
    if (H != QH || I < 1 || I > 32 || clusters < 1 || clusters > fsn_lstm2_g16_clusters(Nrows / 16) ||
        (arith != FSN_ARITH_F16 && arith != FSN_ARITH_BF16)) {
        fsn_set_error("lstm2_g16 (forward): H = 384, up to 32 input columns, 16-bit arithmetic, clusters * 64 <= rows, one cluster per eight CUs at most");
        return FSN_ERR_ARG;
    }
    if (fsn_launch_zero_words(flags, fsn_lstm2_g16_flag_words(clusters), s) != FSN_OK) return FSN_ERR_LAUNCH;
    unsigned short* p = static_cast<unsigned short*>(w16);
    unsigned short *p_ih0 = p, *p_hh0 = p_ih0 + (size_t)QG * 32, *p_ih1 = p_hh0 + (size_t)QG * QH, *p_hh1 = p_ih1 + (size_t)QG * QH;
    int rc;
    if (arith == FSN_ARITH_F16) {
        if ((rc = g16_pack_fwd<FSN_ARITH_F16>(w_ih0, p_ih0, I, 32, s)) || (rc = g16_pack_fwd<FSN_ARITH_F16>(w_hh0, p_hh0, QH, QH, s)) ||
            (rc = g16_pack_fwd<FSN_ARITH_F16>(w_ih1, p_ih1, QH, QH, s)) || (rc = g16_pack_fwd<FSN_ARITH_F16>(w_hh1, p_hh1, QH, QH, s)))
            return rc;
    } else {
        if ((rc = g16_pack_fwd<FSN_ARITH_BF16>(w_ih0, p_ih0, I, 32, s)) || (rc = g16_pack_fwd<FSN_ARITH_BF16>(w_hh0, p_hh0, QH, QH, s)) ||
            (rc = g16_pack_fwd<FSN_ARITH_BF16>(w_ih1, p_ih1, QH, QH, s)) || (rc = g16_pack_fwd<FSN_ARITH_BF16>(w_hh1, p_hh1, QH, QH, s)))
            return rc;
    }
    G16FwdArgs a{};
    a.x = x;
    a.x_step = Nrows;
    a.w16 = p;
    a.o_ih0 = 0;
    a.o_hh0 = (unsigned)((p_hh0 - p) * 2);
    a.o_ih1 = (unsigned)((p_ih1 - p) * 2);
    a.o_hh1 = (unsigned)((p_hh1 - p) * 2);
    a.bias0 = bias0;
    a.bias1 = bias1;
    a.hseq0 = hseq0;
    a.hseq1 = hseq1;
    a.gates0 = save0;
    a.cseq0 = save0 + (size_t)Tp * Nrows * QG;
    a.gates1 = save1;
    a.cseq1 = save1 + (size_t)Tp * Nrows * QG;
    a.flags = flags;
    a.status = flags + fsn_lstm2_g16_status_word(clusters);
    a.spin_ticks = fsn_spin_ticks();
    a.Tp = Tp;
    a.Nrows = Nrows;
    const dim3 grid((unsigned)clusters * QM * 2), block(256);
    if (saves16) {
        if (arith == FSN_ARITH_F16) FSN_PERSIST_LAUNCH((lstm2_g16_fwd_kernel<FSN_ARITH_F16, 1>), grid, block, s, a);
        else FSN_PERSIST_LAUNCH((lstm2_g16_fwd_kernel<FSN_ARITH_BF16, 1>), grid, block, s, a);
    } else {
        if (arith == FSN_ARITH_F16) FSN_PERSIST_LAUNCH(lstm2_g16_fwd_kernel<FSN_ARITH_F16>, grid, block, s, a);
        else FSN_PERSIST_LAUNCH(lstm2_g16_fwd_kernel<FSN_ARITH_BF16>, grid, block, s, a);
    }
    return fsn_check_launch("lstm2_g16_fwd_kernel");
}

// Rows [0, 64 clusters) of the two layers' back-propagation through time, 16-bit operands (FSN_ARITH_F16 / _BF16).  w_*
// UNPACKED; save0 / save1 in fsn_lstm_layer_forward's layout; dg0 / dg1 [Tp][Nrows][4H] out; exchange:
// fsn_lstm2_g16_partial_floats(clusters) floats of scratch; wbuf: fsn_lstm2_g16_bwd_weight_bytes() bytes.
int fsn_launch_lstm2_g16_bptt(const float* dh1, const float* w_hh1, const float* w_ih1, const float* w_hh0, const float* save0,
                              const float* save1, float* dg0, float* dg1, float* exchange, unsigned* flags, void* wbuf, int Tp,
                              int Nrows, int clusters, int H, hipStream_t s, int arith, void* dg16_0, void* dg16_1, float* dbp,
                              int dg1_f32, int dg0_f32) {
    const bool saves16 = (arith & FSN_ARITH_SAVES16) != 0;
    arith &= ~FSN_ARITH_SAVES16;
    if (H != QH || clusters < 1 || clusters > fsn_lstm2_g16_clusters(Nrows / 16) || (arith != FSN_ARITH_F16 && arith != FSN_ARITH_BF16)) {
        fsn_set_error("lstm2_g16 (bptt): H = 384, 16-bit arithmetic, clusters * 64 <= rows, one cluster per eight CUs at most");
        return FSN_ERR_ARG;
    }
    if (fsn_launch_zero_words(flags, fsn_lstm2_g16_flag_words(clusters), s) != FSN_OK) return FSN_ERR_LAUNCH;
    G16BwdArgs a{};
    a.dh1 = dh1;
    a.gates0 = save0;
    a.cseq0 = save0 + (size_t)Tp * Nrows * QG;
    a.gates1 = save1;
    a.cseq1 = save1 + (size_t)Tp * Nrows * QG;
    a.dg0 = dg0;
    a.dg1 = dg1;
    a.dg16_0 = static_cast<unsigned short*>(dg16_0);
    a.dg16_1 = static_cast<unsigned short*>(dg16_1);
    a.dbp = dbp;
    a.dg1_f32 = dg1_f32;
    a.dg0_f32 = dg0_f32;
    if (!dg16_0 || !dg16_1 || !dbp) {
        fsn_set_error("lstm2_g16 (bptt): NULL 16-bit gate-gradient / bias-gradient buffer");
        return FSN_ERR_ARG;
    }
    a.flags = flags;
    a.status = flags + fsn_lstm2_g16_status_word(clusters);
    a.spin_ticks = fsn_spin_ticks();
    a.Tp = Tp;
    a.Nrows = Nrows;
    if (arith == FSN_ARITH_F16) return g16_launch_bptt<FSN_ARITH_F16>(a, w_hh1, w_ih1, w_hh0, wbuf, exchange, clusters, s, saves16);
    return g16_launch_bptt<FSN_ARITH_BF16>(a, w_hh1, w_ih1, w_hh0, wbuf, exchange, clusters, s, saves16);
}

// 16-bit copies of the step-by-step rows' gate gradients of ONE layer (rows [row0, row0 + left) of every step)
int fsn_launch_g16_left_to16(const float* dg, void* dg16, int Tp, int Nrows, long row0, int left, hipStream_t s, int arith) {
    if (left <= 0) return FSN_OK;
    const long n4 = (long)Tp * left * QG / 4;
    const unsigned blocks = (unsigned)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
    if (arith == FSN_ARITH_F16)
        hipLaunchKernelGGL(g16_left_to16_kernel<FSN_ARITH_F16>, dim3(blocks), dim3(256), 0, s, dg, static_cast<unsigned short*>(dg16), Tp, (long)Nrows, row0, left);
    else
        hipLaunchKernelGGL(g16_left_to16_kernel<FSN_ARITH_BF16>, dim3(blocks), dim3(256), 0, s, dg, static_cast<unsigned short*>(dg16), Tp, (long)Nrows, row0, left);
    return fsn_check_launch("g16_left_to16_kernel");
}
// After fsn_launch_lstm2_g16_bptt AND the step-by-step rows beside it: 16-bit copies of those rows' gate gradients (rows
// [row0, row0 + left) of every step, both layers: dg = dg1 | dg0 adjacent, dg16 likewise) and the bias gradients
// db1 / db0 [4H] = the launch's cluster sums (dbp) + those rows.
int fsn_launch_lstm2_g16_finish(const float* dg1, const float* dg0, void* dg16_1, void* dg16_0, const float* dbp, int clusters, int Tp,
                                int Nrows, int left, float* db1, float* db0, hipStream_t s, int arith) {
    const long row0 = (long)clusters * QROWS;
    if (left > 0) {
        const long n4 = (long)Tp * left * QG / 4;
        const unsigned blocks = (unsigned)((n4 + 255) / 256 < 1024 ? (n4 + 255) / 256 : 1024);
        for (int layer = 0; layer < 2; ++layer) {
            const float* src = layer ? dg1 : dg0;
            unsigned short* dst = static_cast<unsigned short*>(layer ? dg16_1 : dg16_0);
            if (arith == FSN_ARITH_F16)
                hipLaunchKernelGGL(g16_left_to16_kernel<FSN_ARITH_F16>, dim3(blocks), dim3(256), 0, s, src, dst, Tp, (long)Nrows, row0, left);
            else
                hipLaunchKernelGGL(g16_left_to16_kernel<FSN_ARITH_BF16>, dim3(blocks), dim3(256), 0, s, src, dst, Tp, (long)Nrows, row0, left);
            FSN_TRY_LAUNCH("g16_left_to16_kernel");
        }
    }
    hipLaunchKernelGGL(g16_db_kernel, dim3(QG / 256), dim3(256), 0, s, dbp + (size_t)clusters * QG, clusters, dg1, Tp, (long)Nrows, row0, left, db1);
    FSN_TRY_LAUNCH("g16_db_kernel");
    hipLaunchKernelGGL(g16_db_kernel, dim3(QG / 256), dim3(256), 0, s, dbp, clusters, dg0, Tp, (long)Nrows, row0, left, db0);
    return fsn_check_launch("g16_db_kernel");
}
