// C = A^T B (and layer 0's dx) with the operands 16-bit IN MEMORY: the weight-gradient products of the 16-bit training
// arithmetic.  The fp32-memory forms and the split-K plan these share (fsn_tn_plan) are in gemm_tn_kernels.hip.
#include "persist_sync.h"

namespace {

// gemm_tn16_kernel's product (gemm_tn_kernels.hip) with the operands ALREADY in 16 bits in memory (the BPTT kernel writes
// the 16-bit gate gradients it forms for the
// exchange anyway; the hidden sequences are converted once): half the HBM bytes, and no conversion pass - so the slabs go
// global -> LDS by LDS-DMA (no registers: four chunks of 24 KB in flight per CU instead of the two that fit the
// architectural registers), each DMA instruction building two [16 k][16 columns] subtiles of the image
// ds_read_b64_tr_b16 wants (lane l fetches row (l & 31) >> 1, half l & 1 of subtile l >> 5).  K in chunks of 32 (the
// caller passes K rounded down to 32; the reduce kernel adds the tail rows from the same 16-bit operands).
constexpr int TH_STAGES = 4;             // (6 stages = 5 chunks in flight measured SLOWER, 0.76 against 0.66 ms: the LDS-DMA path lands ~29 GB/s per CU whatever is in flight)
// WN: waves along the N side - 2: 192 x 192 tile, four waves (the square plan); 4: 192 x 384 tile, eight waves - a weight
// gradient's whole 384-column side in one workgroup, so that the [k][1536] gate-gradient rows are fetched once per 192 of
// their columns instead of twice (the launch is bound by the bytes its DMAs land: 36 KB per chunk for 192 x 384 outputs
// against 2 x 24 KB)
template <int WN>
constexpr int th_stage_bytes() { return 2 * (12 + 6 * WN) * 512; }  // (A 12 + B 6 WN column tiles) x 2 k steps x 512 B
template <int AR, int WN>
__global__ __launch_bounds__(WN * 128) void gemm_tn16h_kernel(const unsigned short* __restrict__ A, long lda,
                                                              const unsigned short* __restrict__ B, long ldb,
                                                              float* __restrict__ part, int M, int Nc, long K, long k_per_split,
                                                              int m_blocks, int n_blocks) {
    constexpr int TH_STAGE = th_stage_bytes<WN>();
    constexpr int NTB = 6 * WN;        // B column tiles of the workgroup
    constexpr int B0 = 12 * 1024;      // byte offset of the B block inside a stage (A: 2 k steps x 6 KB)
    extern __shared__ __attribute__((aligned(16))) unsigned char th_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    const int tiles = m_blocks * n_blocks, xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    const int tile = jb % tiles, split = xcd * ((int)(gridDim.x >> 3) / tiles) + jb / tiles;
    const int mb = tile / n_blocks, nb = tile % n_blocks;
    const int m0 = mb * 192, n0 = nb * (96 * WN);
    const long k_begin = (long)split * k_per_split;
    long k_end = k_begin + k_per_split;
    k_end = k_end < K ? k_end : K;
    const int chunks = (int)((k_end - k_begin) >> 5);  // whole chunks of 32 (K and k_per_split are multiples of 32)
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)th_lds;

    // staging roles (six DMA instructions per chunk each, one per pair of column tiles): role 0, 1 = A, k step 0 / 1;
    // role 2 + 2 h + ks = B columns [192 h, 192 h + 192), k step ks.  Wave w takes role w (2 + WN roles: with eight waves the
    // last two stage nothing).  Lane l -> row 16 ks + ((l & 31) >> 1), columns 16 (2 p + (l >> 5)) + 8 (l & 1) .. + 7
    const bool loader = wave < 2 + WN;
    const int s_op = wave >= 2 ? 1 : 0, s_ks = wave & 1, s_half = wave >= 2 ? (wave - 2) >> 1 : 0;
    const long s_ld = s_op ? ldb : lda;
    const unsigned short* sp = (s_op ? B + n0 + 192 * s_half : A + m0) + (k_begin + 16 * s_ks + ((lane & 31) >> 1)) * s_ld +
                               16 * (lane >> 5) + 8 * (lane & 1);
    const unsigned s_dst = s_op ? (unsigned)(B0 + (s_ks * (NTB / 2) + s_half * 6) * 1024) : (unsigned)(s_ks * 6 * 1024);
    auto issue = [&](int c) {  // chunk c into stage c % TH_STAGES
        if (!loader) return;
        const unsigned dst = lds0 + (unsigned)((c % TH_STAGES) * TH_STAGE) + s_dst;
#pragma unroll
        for (int p = 0; p < 6; ++p) fsn_lds_dma(sp + (long)c * 32 * s_ld + 32 * p, dst + (unsigned)(p * 1024));
    };
    f32x4 acc[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lane_off = (4 * lq + (lr >> 2)) * 32 + (lr & 3) * 8;
    auto tr = [&](const unsigned char* p) {
        return __builtin_bit_cast(typename FsnOperand<AR>::type,
                                  __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fsn_s16x4*)p));
    };
    auto compute = [&](int stage) {
        typename FsnOperand<AR>::type a[2][6], b[2][6];
        const unsigned char* base = th_lds + stage * TH_STAGE + lane_off;  // column tile i of an operand block at + i * 512
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                a[ks][i] = tr(base + ks * 6 * 1024 + (wm * 6 + i) * 512);
                b[ks][i] = tr(base + B0 + ks * (NTB / 2) * 1024 + (wn * 6 + i) * 512);
            }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[i][j] = fsn_mma_k32<AR>(a[0][i], a[1][i], b[0][j], b[1][j], acc[i][j]);
    };
    // TH_STAGES - 1 chunks in flight; the DMAs are invisible to the compiler's counter, so the waits are stated here: a
    // staging wave issues 6 per chunk, in order, and nothing else that counts
#pragma unroll
    for (int c = 0; c < TH_STAGES - 1; ++c)
        if (c < chunks) issue(c);
    for (int c = 0; c < chunks; ++c) {
        static_assert(TH_STAGES == 4, "the counted wait below: TH_STAGES - 2 younger chunks x 6 DMAs per wave");
        if (c + TH_STAGES - 1 <= chunks) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");  // two younger chunks may still be in flight
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // chunk c of every wave has landed; everyone has left stage (c - 1) % TH_STAGES
        if (c + TH_STAGES - 1 < chunks) issue(c + TH_STAGES - 1);
        compute(c % TH_STAGES);
    }
    float* out = part + (long)split * M * Nc;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * 6 + i) * 16 + 4 * lq + r, n = n0 + (wn * 6 + j) * 16 + lr;
                out[(long)m * Nc + n] = acc[i][j][r];
            }
}
// its epilogue: sum of the split partials (fixed order) + the tail rows (K % 32) from the same 16-bit operands
template <int AR>
__global__ void tn16h_reduce_kernel(const float* __restrict__ part, float* __restrict__ C, long ldc, int M, int Nc, int splits,
                                    const unsigned short* __restrict__ A, long lda, const unsigned short* __restrict__ B,
                                    long ldb, long k_tail0, long K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * Nc) return;
    const int m = (int)(i / Nc), n = (int)(i % Nc);
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += part[(long)s * M * Nc + i];
    for (long k = k_tail0; k < K; ++k) {
        float a, b;
        if constexpr (AR == FSN_ARITH_F16) {
            a = (float)__builtin_bit_cast(_Float16, A[k * lda + m]);
            b = (float)__builtin_bit_cast(_Float16, B[k * ldb + n]);
        } else {
            a = __builtin_bit_cast(float, (unsigned)A[k * lda + m] << 16);
            b = __builtin_bit_cast(float, (unsigned)B[k * ldb + n] << 16);
        }
        acc = fmaf(a, b, acc);
    }
    C[(long)m * ldc + n] = acc;
}

// ---- layer 0's INPUT-side products from the 16-bit gate gradients (round 6) -------------------------------------------------
// With these two the BPTT launch of the 16-bit arithmetic stores no fp32 gate gradients at all (2.45 GB less written per
// step at config 3's shape, 2 x 2.45 GB less read): dW_ih0 = dgates0^T x and dx = dgates0 W_ih0 take the row-major 16-bit
// copies the launch writes for the large products anyway - both operands of both products rounded to 16 bits, as every other
// product of the autocast arithmetic (dx used to be an fp32 product of the fp32 gradients: wider than the reference's own).
//
// (1) dW_ih0 [M = 4H][<= 32] = A^T B: gemm_tn16h_kernel's staging (LDS-DMA into the image ds_read_b64_tr_b16 wants, four stages)
// on a 384 x 32 tile: four waves x 96 gate columns, B = the 32 input columns.  A chunk of 32 k: A 2 k steps x 24 column
// tiles x 512 B, B 2 x 2 x 512 B.  Wave w stages A's k step w & 1, column pairs 6 (w >> 1) .. + 5; waves 0, 1 also B's k step w.
constexpr int TNN_STAGE = 2 * (24 + 2) * 512;
template <int AR>
__global__ __launch_bounds__(256) void gemm_tn16n_kernel(const unsigned short* __restrict__ A, long lda,
                                                         const unsigned short* __restrict__ B, long ldb, float* __restrict__ part,
                                                         int M, long K, long k_per_split, int m_blocks) {
    constexpr int B0 = 2 * 24 * 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char th_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int mb = (int)blockIdx.x % m_blocks, split = (int)blockIdx.x / m_blocks;
    const int m0 = mb * 384;
    const long k_begin = (long)split * k_per_split;
    long k_end = k_begin + k_per_split;
    k_end = k_end < K ? k_end : K;
    const int chunks = k_end > k_begin ? (int)((k_end - k_begin) >> 5) : 0;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)th_lds;
    const int s_ks = wave & 1, s_half = wave >> 1;
    const long s_row = k_begin + 16 * s_ks + ((lane & 31) >> 1);
    const int s_col = 16 * (lane >> 5) + 8 * (lane & 1);
    const unsigned short* spa = A + m0 + 192 * s_half + s_row * lda + s_col;
    const unsigned short* spb = B + s_row * ldb + s_col;
    const unsigned dst_a = (unsigned)(s_ks * 24 * 512 + s_half * 6 * 1024), dst_b = (unsigned)(B0 + s_ks * 2 * 512);
    auto issue = [&](int c) {
        const unsigned st = lds0 + (unsigned)((c % TH_STAGES) * TNN_STAGE);
#pragma unroll
        for (int p = 0; p < 6; ++p) fsn_lds_dma(spa + (long)c * 32 * lda + 32 * p, st + dst_a + (unsigned)(p * 1024));
        if (wave < 2) fsn_lds_dma(spb + (long)c * 32 * ldb, st + dst_b);
    };
    f32x4 acc[6][2];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int lane_off = (4 * lq + (lr >> 2)) * 32 + (lr & 3) * 8;
    auto tr = [&](const unsigned char* p) {
        return __builtin_bit_cast(typename FsnOperand<AR>::type,
                                  __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) fsn_s16x4*)p));
    };
#pragma unroll
    for (int c = 0; c < TH_STAGES - 1; ++c)
        if (c < chunks) issue(c);
    for (int c = 0; c < chunks; ++c) {
        static_assert(TH_STAGES == 4, "the counted waits below: two younger chunks of 7 (waves 0, 1) / 6 DMAs per wave");
        if (c + TH_STAGES - 1 <= chunks) {
            if (wave < 2) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();  // chunk c of every wave has landed; everyone has left stage (c - 1) % TH_STAGES
        if (c + TH_STAGES - 1 < chunks) issue(c + TH_STAGES - 1);
        const unsigned char* base = th_lds + (c % TH_STAGES) * TNN_STAGE + lane_off;
        typename FsnOperand<AR>::type a[2][6], b[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < 6; ++i) a[ks][i] = tr(base + ks * 24 * 512 + (wave * 6 + i) * 512);
#pragma unroll
            for (int j = 0; j < 2; ++j) b[ks][j] = tr(base + B0 + ks * 2 * 512 + j * 512);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = fsn_mma_k32<AR>(a[0][i], a[1][i], b[0][j], b[1][j], acc[i][j]);
    }
    float* out = part + (long)split * M * 32;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(long)(m0 + (wave * 6 + i) * 16 + 4 * lq + r) * 32 + j * 16 + lr] = acc[i][j][r];
}
// its epilogue: the split partials [split][M][32] (fixed order) + the K % 32 tail rows, the first Nc <= 32 columns out
template <int AR>
__global__ void tn16n_reduce_kernel(const float* __restrict__ part, float* __restrict__ C, long ldc, int M, int Nc, int splits,
                                    const unsigned short* __restrict__ A, long lda, const unsigned short* __restrict__ B,
                                    long ldb, long k_tail0, long K) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * Nc) return;
    const int m = (int)(i / Nc), n = (int)(i % Nc);
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += part[((long)s * M + m) * 32 + n];
    for (long k = k_tail0; k < K; ++k) {
        float a, b;
        if constexpr (AR == FSN_ARITH_F16) {
            a = (float)__builtin_bit_cast(_Float16, A[k * lda + m]);
            b = (float)__builtin_bit_cast(_Float16, B[k * ldb + n]);
        } else {
            a = __builtin_bit_cast(float, (unsigned)A[k * lda + m] << 16);
            b = __builtin_bit_cast(float, (unsigned)B[k * ldb + n] << 16);
        }
        acc = fmaf(a, b, acc);
    }
    C[(long)m * ldc + n] = acc;
}

// (2) dx [rows][I <= 32] = dg16 [rows][G] W [G][I], formed transposed like every product of the 16-bit kernels:
// D^T[input column][row] = W^T (A operand: fragments packed once, resident in LDS) x dg16^T (B operand: a lane's eight
// consecutive gate columns of one row = one 16-byte load straight from the row-major copy), so a lane ends up with four
// consecutive input columns of one row: 16-byte stores.  A wave walks 16-row tiles; its operand loads run twelve K blocks
// ahead.  HBM-bound: 2 G bytes per row in, 128 out.
constexpr int DX16_DEPTH = 12;
template <int AR>
__global__ void dx16_pack_kernel(const float* __restrict__ w, unsigned short* __restrict__ out, int G, int I) {
    // fragment (kb, j): lane (lr, lq) holds W[32 kb + 8 lq + e][16 j + lr], e = 0..7 (zero beyond I)
    const long n = (long)(G / 32) * 2 * 64;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63), j = (int)((i >> 6) & 1), kb = (int)(i >> 7);
        const int col = 16 * j + (lane & 15), k0 = 32 * kb + 8 * (lane >> 4);
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            lo[e] = col < I ? w[(long)(k0 + e) * I + col] : 0.f;
            hi[e] = col < I ? w[(long)(k0 + 4 + e) * I + col] : 0.f;
        }
        const fsn_u32x2 a = __builtin_bit_cast(fsn_u32x2, fsn_operand<AR>(lo)), b = __builtin_bit_cast(fsn_u32x2, fsn_operand<AR>(hi));
        reinterpret_cast<fsn_u32x4*>(out)[i] = fsn_u32x4{a[0], a[1], b[0], b[1]};
    }
}
template <int AR>
__global__ __launch_bounds__(256) void gemm_dx16_kernel(const unsigned short* __restrict__ dg16, long ld16,
                                                        const unsigned short* __restrict__ wfrag, float* __restrict__ dx, long lddx,
                                                        long tiles, int I, int KB) {
    extern __shared__ __attribute__((aligned(16))) unsigned char wl[];  // [KB][2][64 lanes][16 B]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lq = lane >> 4;
    for (int i = tid; i < KB * 2 * 64; i += 256) reinterpret_cast<fsn_u32x4*>(wl)[i] = reinterpret_cast<const fsn_u32x4*>(wfrag)[i];
    __syncthreads();
    auto opnd = [](const fsn_u32x4 v, int h) {
        return fsn_wfrag_operand<AR>(fsn_u32x2{v[2 * h], v[2 * h + 1]});
    };
    for (long tile = (long)blockIdx.x * 4 + wave; tile < tiles; tile += (long)gridDim.x * 4) {
        const unsigned short* p = dg16 + (tile * 16 + lr) * ld16 + lq * 8;
        fsn_u32x4 ring[DX16_DEPTH];
#pragma unroll
        for (int d = 0; d < DX16_DEPTH; ++d) ring[d] = *reinterpret_cast<const fsn_u32x4*>(p + d * 32);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        for (int kb0 = 0; kb0 < KB; kb0 += DX16_DEPTH) {
#pragma unroll
            for (int d = 0; d < DX16_DEPTH; ++d) {
                const int kb = kb0 + d;
                const fsn_u32x4 b = ring[d];
                if (kb + DX16_DEPTH < KB) ring[d] = *reinterpret_cast<const fsn_u32x4*>(p + (kb + DX16_DEPTH) * 32);
                const fsn_u32x4 a0 = reinterpret_cast<const fsn_u32x4*>(wl)[(kb * 2 + 0) * 64 + lane];
                const fsn_u32x4 a1 = reinterpret_cast<const fsn_u32x4*>(wl)[(kb * 2 + 1) * 64 + lane];
                acc0 = fsn_mma_k32<AR>(opnd(a0, 0), opnd(a0, 1), opnd(b, 0), opnd(b, 1), acc0);
                acc1 = fsn_mma_k32<AR>(opnd(a1, 0), opnd(a1, 1), opnd(b, 0), opnd(b, 1), acc1);
            }
        }
        float* o = dx + (tile * 16 + lr) * lddx + 4 * lq;
        if (I == 32) {
            *reinterpret_cast<f32x4*>(o) = acc0;
            *reinterpret_cast<f32x4*>(o + 16) = acc1;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (4 * lq + r < I) o[r] = acc0[r];
                if (16 + 4 * lq + r < I) o[16 + r] = acc1[r];
            }
        }
    }
}

}  // namespace

// C [M][Nc] = sum_k A[k][m] B[k][n] with BOTH operands 16-bit in memory (fp16 / bf16 per `arith`), fp32 accumulation:
// M and Nc multiples of 192, one workgroup per CU over the 192 x 192 tiles with every K split's tiles on one XCD (the
// plan of fsn_launch_gemm_tn's square form); false when the shape has no such plan.  workspace: fsn_gemm_tn_workspace_bytes.
static int g_tn16h_wide = 1;  // fsn_tn16h_wide(0): the 192 x 192 tiles also where the 192 x 384 form applies (A/B measurements, tests)
void fsn_tn16h_wide(int on) { g_tn16h_wide = on; }
// the 192 x 384 form: Nc a multiple of 384, whole K splits per XCD with one (eight-wave) workgroup per CU
static bool tn16h_wide_plan(int M, int Nc, long K32, FsnTnPlan* out) {
    const int cus = plan_cus();
    if (!g_tn16h_wide || M % 192 || Nc % 384 || cus % 8) return false;
    const int tiles = (M / 192) * (Nc / 384);
    if ((cus / 8) % tiles) return false;
    const long s = cus / tiles;
    const long kps = ((K32 + s - 1) / s + 31) / 32 * 32;
    if (kps < 128 || (K32 + kps - 1) / kps != s || s > fsn_tn_max_splits(M, Nc)) return false;
    if (out) {
        out->square = 1;
        out->narrow = 0;
        out->m_blocks = M / 192;
        out->n_blocks = Nc / 384;
        out->splits = (int)s;
        out->k_per_split = kps;
    }
    return true;
}
// which form a product takes and its K splits: 0 none, 1 the 192 x 192 form, 2 the 192 x 384 form.  ONE rule for the
// launcher, for fsn_gemm_tn16h_supported and for the test query: the square form splits K in whole chunks of 32 rows where
// fsn_tn_plan counts in 16, and a plan whose splits come out fewer that way is no plan (fsn_gemm_tn16h_supported used to say
// yes from fsn_tn_plan alone; fsn_lstm2_backward then failed with "gemm_tn16h: no plan", e.g. at T = 4, N = 1552 on 256 CUs)
static int tn16h_pick(int M, int Nc, long K, FsnTnPlan* p) {
    const long K32 = K & ~31L;
    if (K32 <= 0) return 0;
    if (tn16h_wide_plan(M, Nc, K32, p)) return 2;
    *p = fsn_tn_plan(M, Nc, K32, FSN_ARITH_F16);
    if (!p->square) return 0;
    p->k_per_split = (p->k_per_split + 31) / 32 * 32;  // whole chunks; the last split takes what is left (K32 is a multiple of 32)
    return (K32 + p->k_per_split - 1) / p->k_per_split == p->splits && p->splits <= fsn_tn_max_splits(M, Nc) ? 1 : 0;
}
bool fsn_gemm_tn16h_supported(int M, int Nc, long K) {
    FsnTnPlan p{};
    return tn16h_pick(M, Nc, K, &p) != 0;
}
int fsn_gemm_tn16h_form(int M, int Nc, long K, int* splits) {
    FsnTnPlan p{};
    const int form = tn16h_pick(M, Nc, K, &p);
    if (splits) *splits = form ? p.splits : 0;
    return form;
}
// the two launches of a planned product under arithmetic AR: the split partials, then their sum + the K % 32 tail rows
template <int AR>
static int tn16h_run(const unsigned short* a, long lda, const unsigned short* b, long ldb, float* C, long ldc, int M, int Nc,
                     long K, float* part, hipStream_t s, const FsnTnPlan& p, bool wide) {
    const long K32 = K & ~31L;
    const dim3 grid((unsigned)(p.m_blocks * p.n_blocks * p.splits));
    if (wide) {
        constexpr size_t kLdsW = (size_t)TH_STAGES * th_stage_bytes<4>();  // 144 KB: one workgroup per CU by itself
        FSN_TRY_RESERVE_LDS("gemm_tn16h", (gemm_tn16h_kernel<AR, 4>), kLdsW);
        hipLaunchKernelGGL((gemm_tn16h_kernel<AR, 4>), grid, dim3(512), kLdsW, s, a, lda, b, ldb, part, M, Nc, K32, p.k_per_split,
                           p.m_blocks, p.n_blocks);
    } else {
        constexpr size_t kLds = kFsnTnOnePerCu;  // 4 stages of 24 KB = the reservation that keeps one workgroup per CU
        static_assert(TH_STAGES * th_stage_bytes<2>() <= (int)kFsnTnOnePerCu, "the stages fit it");
        FSN_TRY_RESERVE_LDS("gemm_tn16h", (gemm_tn16h_kernel<AR, 2>), kLds);
        hipLaunchKernelGGL((gemm_tn16h_kernel<AR, 2>), grid, dim3(256), kLds, s, a, lda, b, ldb, part, M, Nc, K32, p.k_per_split,
                           p.m_blocks, p.n_blocks);
    }
    FSN_TRY_LAUNCH("gemm_tn16h_kernel");
    const long n = (long)M * Nc;
    hipLaunchKernelGGL(tn16h_reduce_kernel<AR>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, C, ldc, M, Nc, p.splits,
                       a, lda, b, ldb, K32, K);
    return fsn_check_launch("tn16h_reduce_kernel");
}
int fsn_launch_gemm_tn16h(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                          void* workspace, hipStream_t s, int arith) {
    if ((arith != FSN_ARITH_F16 && arith != FSN_ARITH_BF16) || !fsn_gemm_tn16h_supported(M, Nc, K) || lda % 8 || ldb % 8 ||
        ((size_t)A16 & 15) || ((size_t)B16 & 15)) {
        fsn_set_error("gemm_tn16h: 16-bit arithmetic, M and Nc multiples of 192 with a one-workgroup-per-CU plan, 16-byte aligned rows");
        return FSN_ERR_ARG;
    }
    FsnTnPlan p{};
    const int form = tn16h_pick(M, Nc, K, &p);
    if (!form) {
        fsn_set_error("gemm_tn16h: no plan for %d x %d, K = %ld", M, Nc, K);
        return FSN_ERR_ARG;
    }
    const bool wide = form == 2;
    float* part = static_cast<float*>(workspace);
    const unsigned short *a = static_cast<const unsigned short*>(A16), *b = static_cast<const unsigned short*>(B16);
    return arith == FSN_ARITH_F16 ? tn16h_run<FSN_ARITH_F16>(a, lda, b, ldb, C, ldc, M, Nc, K, part, s, p, wide)
                                  : tn16h_run<FSN_ARITH_BF16>(a, lda, b, ldb, C, ldc, M, Nc, K, part, s, p, wide);
}


// dW [M][Nc <= 32] = A16^T B16 over K rows, both operands 16-bit row-major in memory (A [K][lda >= M], B [K][ldb >= 32], its
// columns beyond Nc zero); M a multiple of 384.  workspace: fsn_gemm_tn_workspace_bytes(M, Nc, K).
bool fsn_gemm_tn16n_supported(int M, int Nc, long K) { return M % 384 == 0 && Nc >= 1 && Nc <= 32 && (K & ~31L) >= 32 * 64; }
template <int AR>
static int tn16n_run(const unsigned short* a, long lda, const unsigned short* b, long ldb, float* C, long ldc, int M, int Nc,
                     long K, float* part, hipStream_t s, int m_blocks, int splits, long kps) {
    const long K32 = K & ~31L;
    constexpr size_t kLds = (size_t)TH_STAGES * TNN_STAGE;  // 104 KB: one workgroup per CU by itself
    FSN_TRY_RESERVE_LDS("gemm_tn16n", gemm_tn16n_kernel<AR>, kLds);
    hipLaunchKernelGGL(gemm_tn16n_kernel<AR>, dim3((unsigned)(m_blocks * splits)), dim3(256), kLds, s, a, lda, b, ldb, part, M, K32,
                       kps, m_blocks);
    FSN_TRY_LAUNCH("gemm_tn16n_kernel");
    const long n = (long)M * Nc;
    hipLaunchKernelGGL(tn16n_reduce_kernel<AR>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, C, ldc, M, Nc, splits, a,
                       lda, b, ldb, K32, K);
    return fsn_check_launch("tn16n_reduce_kernel");
}
// its K splits (one workgroup per CU, as many as the workspace holds) and the rows of each; 0: not even one partial fits
static long tn16n_splits(int M, int Nc, long K, long* kps_out) {
    const int cus = plan_cus();
    const long K32 = K & ~31L;
    const int m_blocks = M / 384;
    long splits = cus / m_blocks > 1 ? cus / m_blocks : 1;
    // the partials take 32 columns per split whatever Nc is, while the workspace query counts Nc + 1: with a small Nc on a
    // device of few CUs not even one partial fits
    const long bound = (long)(fsn_gemm_tn_workspace_bytes(M, Nc, K) / ((size_t)M * 32 * sizeof(float)));
    if (bound < 1) return 0;
    splits = splits < bound ? splits : bound;
    const long kps = ((K32 + splits - 1) / splits + 31) / 32 * 32;
    if (kps_out) *kps_out = kps;
    return (K32 + kps - 1) / kps;
}
int fsn_gemm_tn16n_splits(int M, int Nc, long K) { return fsn_gemm_tn16n_supported(M, Nc, K) ? (int)tn16n_splits(M, Nc, K, nullptr) : 0; }
int fsn_launch_gemm_tn16n(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                          void* workspace, hipStream_t s, int arith) {
    if ((arith != FSN_ARITH_F16 && arith != FSN_ARITH_BF16) || !fsn_gemm_tn16n_supported(M, Nc, K) || lda % 8 || ldb % 8 || ldb < 32 ||
        ((size_t)A16 & 15) || ((size_t)B16 & 15)) {
        fsn_set_error("gemm_tn16n: 16-bit arithmetic, M a multiple of 384, Nc <= 32 in rows of >= 32 16-bit columns, 16-byte aligned rows");
        return FSN_ERR_ARG;
    }
    const int m_blocks = M / 384;
    long kps = 0;
    const long splits = tn16n_splits(M, Nc, K, &kps);
    if (splits < 1) {
        fsn_set_error("gemm_tn16n: the workspace of a %d x %d product holds no %d x 32 partial", M, Nc, M);
        return FSN_ERR_WORKSPACE;
    }
    float* part = static_cast<float*>(workspace);
    const unsigned short *a = static_cast<const unsigned short*>(A16), *b = static_cast<const unsigned short*>(B16);
    return arith == FSN_ARITH_F16 ? tn16n_run<FSN_ARITH_F16>(a, lda, b, ldb, C, ldc, M, Nc, K, part, s, m_blocks, (int)splits, kps)
                                  : tn16n_run<FSN_ARITH_BF16>(a, lda, b, ldb, C, ldc, M, Nc, K, part, s, m_blocks, (int)splits, kps);
}

// dx [rows][I <= 32] (row stride lddx) = dg16 [rows][G] W [G][I] with both operands rounded to 16 bits; rows a multiple of 16,
// G a multiple of 32 up to 2048; wfrag: G * 32 16-bit words of scratch for the packed weight (written here).
bool fsn_gemm_dx16_supported(long rows, int G, int I) {
    return rows > 0 && rows % 16 == 0 && G % (32 * DX16_DEPTH) == 0 && G <= 2048 && I >= 1 && I <= 32;
}
// the two launches under arithmetic AR: the weight packed into fragments, then the product
template <int AR>
static int dx16_run(const unsigned short* dg16, long ld16, const float* w, unsigned short* wf, float* dx, long lddx, long rows,
                    int G, int I, hipStream_t s) {
    const int KB = G / 32;
    const size_t lds = (size_t)KB * 2 * 1024;
    const int cus = plan_cus();
    const long tiles = rows / 16;
    const unsigned grid = (unsigned)((tiles + 3) / 4 < cus ? (tiles + 3) / 4 : cus);
    hipLaunchKernelGGL(dx16_pack_kernel<AR>, dim3((unsigned)((KB * 128 + 255) / 256)), dim3(256), 0, s, w, wf, G, I);
    FSN_TRY_LAUNCH("dx16_pack_kernel");
    FSN_TRY_RESERVE_LDS("gemm_dx16", gemm_dx16_kernel<AR>, 128 * 1024);  // G <= 2048: at most 128 KB of fragments
    hipLaunchKernelGGL(gemm_dx16_kernel<AR>, dim3(grid), dim3(256), lds, s, dg16, ld16, wf, dx, lddx, tiles, I, KB);
    return fsn_check_launch("gemm_dx16_kernel");
}
int fsn_launch_gemm_dx16(const void* dg16, long ld16, const float* w, void* wfrag, float* dx, long lddx, long rows, int G, int I,
                         hipStream_t s, int arith) {
    if ((arith != FSN_ARITH_F16 && arith != FSN_ARITH_BF16) || !fsn_gemm_dx16_supported(rows, G, I) || ld16 % 8 || lddx % 4 ||
        ((size_t)dg16 & 15) || ((size_t)dx & 15) || ((size_t)wfrag & 15)) {
        fsn_set_error("gemm_dx16: 16-bit arithmetic, rows %% 16 == 0, G %% 384 == 0 (<= 2048), I <= 32, 16-byte aligned rows");
        return FSN_ERR_ARG;
    }
    return arith == FSN_ARITH_F16
               ? dx16_run<FSN_ARITH_F16>(static_cast<const unsigned short*>(dg16), ld16, w, static_cast<unsigned short*>(wfrag), dx, lddx, rows, G, I, s)
               : dx16_run<FSN_ARITH_BF16>(static_cast<const unsigned short*>(dg16), ld16, w, static_cast<unsigned short*>(wfrag), dx, lddx, rows, G, I, s);
}
