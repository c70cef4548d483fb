// C = A^T B with both operands fp32 row-major over k: the weight gradient of every nn.Linear and LSTM / GRU layer
// (dW = dY^T X), the column sums that are its bias gradient, and the split-K plan that the 16-bit-operand forms of
// gemm_tn16_kernels.hip share.
#include "fsn_common.h"

namespace {

// C[M][Nc] (partial, per K split) = sum_k A[k][m] * B[k][n]; A, B row-major over k (K % 16 == 0).
// Same execution shape as the forward GEMM (gemm_kernels.hip): ONE 4-wave workgroup per CU, one
// wave per SIMD with a large accumulator tile (RTW x CTW MFMA tiles) and a 2-deep register ring of
// operand chunks whose refills are pinned right behind the MFMAs that free them.  Lane (r = l&15,
// q = l>>4) feeds A[k0 + 4q + j][m0 + r] / B[k0 + 4q + j][n0 + r] to the j-th MFMA of a 16-deep
// chunk: 16 lanes read 64 contiguous bytes of one k row, the row base is wave-uniform (SGPR) and
// the lane part a fixed 32-bit offset.  Out-of-range columns are clamped on load and never stored.
// AR: arithmetic of the products (fsn_mma_k16): the lane's four k of a chunk ARE the 16-bit instruction's operand.
template <int RTW, int CTW, int WM, int WN, int AR = FSN_ARITH_F32, int PF = 2>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const float* __restrict__ A, long lda,
                                                      const float* __restrict__ B, long ldb,
                                                      float* __restrict__ part, int M, int Nc, long K, long k_per_split,
                                                      int m_blocks, int n_blocks, float* __restrict__ asum_part,
                                                      int xcd_grouped) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;  // PF: operand chunks in flight (register ring)
    const int lr = lane & 15, lq = lane >> 4;
    const int wm = wave / WN, wn = wave % WN;
    int tile = blockIdx.x % (m_blocks * n_blocks), split = blockIdx.x / (m_blocks * n_blocks);
    if (xcd_grouped) {
        // all tiles of a K split on ONE XCD (block b runs on XCD b % 8: observed, speed only): the split's A rows are
        // read by n_blocks workgroups and its B rows by m_blocks - from that XCD's L2 after the first touch instead of
        // once each from HBM (the 16-bit forms are bandwidth-bound: 11 GB per GEMM at config 3's shape otherwise)
        const int tiles = m_blocks * n_blocks, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        tile = j % tiles;
        split = xcd * ((int)(gridDim.x >> 3) / tiles) + j / tiles;
    }
    const int mb = tile / n_blocks, nb = tile % n_blocks;
    const int m0 = (mb * WM + wm) * RTW * 16, n0 = (nb * WN + wn) * CTW * 16;
    const long k_begin = (long)split * k_per_split;
    long k_end = k_begin + k_per_split;
    k_end = k_end < K ? k_end : K;
    const int chunks = (int)((k_end - k_begin) >> 4), last = chunks - 1;

    int aoff[RTW], boff[CTW];
#pragma unroll
    for (int i = 0; i < RTW; ++i) {
        const int m = m0 + i * 16 + lr;
        aoff[i] = 4 * lq * (int)lda + (m < M ? m : M - 1);
    }
#pragma unroll
    for (int i = 0; i < CTW; ++i) {
        const int n = n0 + i * 16 + lr;
        boff[i] = 4 * lq * (int)ldb + (n < Nc ? n : Nc - 1);
    }
    const float* a0 = A + k_begin * lda;
    const float* b0 = B + k_begin * ldb;

    f32x4 acc[RTW][CTW];
#pragma unroll
    for (int i = 0; i < RTW; ++i)
#pragma unroll
        for (int j = 0; j < CTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // column sums of A over k (= the bias gradient when A is dgates) ride along for free: the A fragments are in
    // registers anyway; 8 adds per chunk next to 128 MFMAs.  Written by the n-block-0 / wave-column-0 waves only.
    float asum[RTW];
#pragma unroll
    for (int i = 0; i < RTW; ++i) asum[i] = 0.f;
    float abuf[PF][RTW][4], bbuf[PF][CTW][4];
    auto fetch = [&](int p, int kc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* ar = a0 + ((long)kc * 16 + j) * lda;  // wave-uniform row bases
            const float* br = b0 + ((long)kc * 16 + j) * ldb;
#pragma unroll
            for (int i = 0; i < RTW; ++i) abuf[p][i][j] = ar[aoff[i]];
#pragma unroll
            for (int i = 0; i < CTW; ++i) bbuf[p][i][j] = br[boff[i]];
        }
    };
    auto consume = [&](int p) {
        if constexpr (AR == FSN_ARITH_F32) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < RTW; ++i)
#pragma unroll
                    for (int jj = 0; jj < CTW; ++jj) acc[i][jj] = mfma16(abuf[p][i][j], bbuf[p][jj][j], acc[i][jj]);
        } else {
            typename FsnOperand<AR>::type ao[RTW], bo[CTW];
#pragma unroll
            for (int i = 0; i < RTW; ++i)
                ao[i] = fsn_operand<AR>(f32x4{abuf[p][i][0], abuf[p][i][1], abuf[p][i][2], abuf[p][i][3]});
#pragma unroll
            for (int jj = 0; jj < CTW; ++jj)
                bo[jj] = fsn_operand<AR>(f32x4{bbuf[p][jj][0], bbuf[p][jj][1], bbuf[p][jj][2], bbuf[p][jj][3]});
#pragma unroll
            for (int i = 0; i < RTW; ++i)
#pragma unroll
                for (int jj = 0; jj < CTW; ++jj) acc[i][jj] = fsn_mma_k16<AR>(ao[i], bo[jj], acc[i][jj]);
        }
#pragma unroll
        for (int i = 0; i < RTW; ++i) asum[i] += (abuf[p][i][0] + abuf[p][i][1]) + (abuf[p][i][2] + abuf[p][i][3]);
    };
#pragma unroll
    for (int p = 0; p < PF; ++p) fetch(p, p < last ? p : last);
    const int k_main = (chunks / PF) * PF;
    for (int kc0 = 0; kc0 < k_main; kc0 += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            consume(p);
            __builtin_amdgcn_sched_barrier(0);
            const int kn = kc0 + p + PF;
            fetch(p, kn < last ? kn : last);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int p = 0; p < PF - 1; ++p)  // the left-over chunks (fewer than PF) are already in slots 0 ..
        if (k_main + p < chunks) consume(p);

    float* out = part + (long)split * M * Nc;
#pragma unroll
    for (int i = 0; i < RTW; ++i)
#pragma unroll
        for (int jj = 0; jj < CTW; ++jj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + i * 16 + 4 * lq + r, n = n0 + jj * 16 + lr;
                if (m < M && n < Nc) out[(long)m * Nc + n] = acc[i][jj][r];
            }
    if (asum_part && nb == 0 && wn == 0) {
#pragma unroll
        for (int i = 0; i < RTW; ++i) {
            float v = asum[i];  // lanes r, r + 16, r + 32, r + 48 hold the four k phases of column m0 + 16 i + r
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            const int m = m0 + i * 16 + lr;
            if (lq == 0 && m < M) asum_part[(long)split * M + m] = v;
        }
    }
}

// The same product under the 16-bit training arithmetic, built for it (round 4).  With 16-bit operands the matrix work of
// a 192 x 192 tile is 36 instructions of 8 cycles per 16 k, and gemm_tn_kernel feeds them with 48 DWORD loads per lane
// (a lane's operand is four k of one column: four rows of a K-major matrix) - it ran at 14 % of the 16-bit peak, bound
// by its load instructions.  Here both operand slabs of a 32-k chunk are fetched as 16-BYTE row pieces (12 per thread
// instead of 96 dword loads), rounded to 16 bits once on the way into LDS - [k step][column tile][16 k][16 columns], k
// rows of 32 bytes - and every wave reads its operands with ds_read_b64_tr_b16 (gfx950's transposing LDS read: lane (lr,
// lq) of a 16-lane group addresses row lr / 4, column quad lr % 4 of a [4 k][16 columns] block and receives column lr of
// the four rows = the matrix instruction's operand A[m = lr][k = 4 lq + j]; measured, tools/probe_tr16.hip).  Two LDS
// stages, one barrier per chunk, the next chunk's loads in flight under the current chunk's matrix work.  Same products
// (operands rounded exactly as fsn_mma_k16 rounds them), same k order, same K splits: bit-identical partial sums.  The
// column sums of A (the bias gradient) ride on the staging threads' fp32 values.
constexpr int TQ_TS = 544;             // bytes per [16 k][16 columns] 16-bit subtile (512 + 32: spreads the staging writes over banks)
constexpr int TQ_OP = 2 * 12 * TQ_TS;  // one operand of one chunk: 2 k steps x 12 column tiles
constexpr int TQ_STAGE = 2 * TQ_OP;    // A then B
constexpr int TQ_LDS = 2 * TQ_STAGE + 4 * 48 * 16;
constexpr int TQ_PF = 2;               // chunks of operand rows in flight per staging thread
template <int AR>
__global__ __launch_bounds__(256) void gemm_tn16_kernel(const float* __restrict__ A, long lda, const float* __restrict__ B,
                                                        long ldb, float* __restrict__ part, int M, int Nc, long K,
                                                        long k_per_split, int m_blocks, int n_blocks,
                                                        float* __restrict__ asum_part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tq_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, lq = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    // all tiles of a K split on ONE XCD (block b runs on XCD b % 8: observed, speed only), as gemm_tn_kernel's grouped form
    const int tiles = m_blocks * n_blocks, xcd = blockIdx.x & 7, jb = blockIdx.x >> 3;
    const int tile = jb % tiles, split = xcd * ((int)(gridDim.x >> 3) / tiles) + jb / tiles;
    const int mb = tile / n_blocks, nb = tile % n_blocks;
    const int m0 = mb * 192, n0 = nb * 192;
    const long k_begin = (long)split * k_per_split;
    long k_end = k_begin + k_per_split;
    k_end = k_end < K ? k_end : K;
    const int chunks = (int)((k_end - k_begin + 31) >> 5);

    // staging: thread t < 192 owns the 16-byte piece q = t % 48 of the 192 columns for the k rows 8 (t / 48) + i, i < 8
    const bool stager = tid < 192;
    const int q = tid % 48, kp = (tid / 48) & 3;
    const float* ap = A + (k_begin + kp * 8) * lda + m0 + 4 * q;
    const float* bp = B + (k_begin + kp * 8) * ldb + n0 + 4 * q;
    // TQ_PF chunks of operand rows in flight per staging thread (register sets, statically indexed): the slabs come from
    // HBM (3 GB per product, each element read once: PMC FETCH_SIZE = 3.4 GB), and a chunk's matrix work is ~0.25 us - one
    // chunk ahead left the kernel at 2.3 TB/s, latency-bound; two: 2.65.  Three do not fit the 256 architectural
    // registers a load can target beside the operands (the accumulators live in the other half of the file).
    f32x4 va[TQ_PF][8], vb[TQ_PF][8], asum = {0.f, 0.f, 0.f, 0.f};
    auto load = [&](int set, int c) {
        if (!stager) return;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long k = k_begin + (long)c * 32 + kp * 8 + i;
            const bool ok = k < k_end;
            va[set][i] = ok ? *reinterpret_cast<const f32x4*>(ap + ((long)c * 32 + i) * lda) : f32x4{0.f, 0.f, 0.f, 0.f};
            vb[set][i] = ok ? *reinterpret_cast<const f32x4*>(bp + ((long)c * 32 + i) * ldb) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store = [&](int set, int stage) {
        if (!stager) return;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int kk = kp * 8 + i;
            unsigned char* d = tq_lds + stage * TQ_STAGE + ((kk >> 4) * 12 + (q >> 2)) * TQ_TS + (kk & 15) * 32 + (q & 3) * 8;
            *reinterpret_cast<fsn_u32x2*>(d) = __builtin_bit_cast(fsn_u32x2, fsn_operand<AR>(va[set][i]));
            *reinterpret_cast<fsn_u32x2*>(d + TQ_OP) = __builtin_bit_cast(fsn_u32x2, fsn_operand<AR>(vb[set][i]));
            asum += va[set][i];
        }
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
        // both k steps of the chunk as ONE K = 32 matrix instruction per tile (fsn_mma_k32: round 5)
        typename FsnOperand<AR>::type a[2][6], b[2][6];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const unsigned char* base = tq_lds + stage * TQ_STAGE + ks * 12 * TQ_TS + lane_off;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                a[ks][i] = tr(base + (wm * 6 + i) * TQ_TS);
                b[ks][i] = tr(base + TQ_OP + (wn * 6 + i) * TQ_TS);
            }
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) acc[i][j] = fsn_mma_k32<AR>(a[0][i], a[1][i], b[0][j], b[1][j], acc[i][j]);
    };
    // chunk c lives in register set c % TQ_PF and LDS stage c & 1; rows beyond k_end (and whole chunks beyond the last) load zeros
#pragma unroll
    for (int d = 0; d < TQ_PF; ++d) load(d, d);
    store(0, 0);
    __syncthreads();
    for (int c0 = 0; c0 < chunks; c0 += 2 * TQ_PF) {  // 2 TQ_PF: both the register set and the LDS stage of a chunk are static
#pragma unroll
        for (int d = 0; d < 2 * TQ_PF; ++d) {
            const int c = c0 + d;
            if (c < chunks) {  // uniform
                load(d % TQ_PF, c + TQ_PF);           // set of chunk c (already in LDS) is free: chunk c + TQ_PF takes it
                compute(d & 1);
                store((d + 1) % TQ_PF, (d + 1) & 1);  // chunk c + 1 (zeros beyond the end) into the other stage
                __syncthreads();
            }
        }
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
    if (asum_part && nb == 0) {  // the four k phases of a column quad meet in a fixed order
        f32x4* red = reinterpret_cast<f32x4*>(tq_lds + 2 * TQ_STAGE);
        if (stager) red[kp * 48 + q] = asum;
        __syncthreads();
        if (tid < 48) {
            f32x4 v = red[tid];
#pragma unroll
            for (int k = 1; k < 4; ++k) v += red[k * 48 + tid];
            *reinterpret_cast<f32x4*>(asum_part + (long)split * M + m0 + 4 * tid) = v;
        }
    }
}

// column sums riding on gemm_tn: sum of the split partials (fixed order) + the K % 16 tail rows
__global__ void tn_colsum_reduce_kernel(const float* __restrict__ asum_part, float* __restrict__ out, int M, int splits,
                                        const float* __restrict__ A, long lda, long k_tail0, long K, int accumulate) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += asum_part[(long)s * M + m];
    for (long k = k_tail0; k < K; ++k) acc += A[k * lda + m];
    out[m] = accumulate ? out[m] + acc : acc;  // a later K segment: onto the sum of the earlier ones
}

// out[i] = sum_s part[s][i] in a fixed order
__global__ void reduce_splits_kernel(const float* __restrict__ part, float* __restrict__ C, long ldc, int M, int Nc,
                                     int splits) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * Nc) return;
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += part[(long)s * M * Nc + i];
    C[(i / Nc) * ldc + (i % Nc)] = acc;
}

// gemm_tn epilogue: sum of the split partials (fixed order) + the K % 16 tail rows the MFMA kernel
// does not cover; `transposed`: the partials hold C^T ([Nc][M], operands were swapped).
// Under a 16-bit arithmetic the tail rows' operands are rounded like those of the matrix instructions (they used to enter
// in fp32: at K = 2069 the product stood at 8.4 u rms against 0.14 u of the fp32 product of the rounded operands,
// tests/test_gpu_amp_sweep.py; the training step's K = T N are multiples of 16 and have no tail).
template <int AR>
__device__ __forceinline__ float tn_tail_term(float a, float b) {
    if constexpr (AR == FSN_ARITH_F16) {
        const fsn_f16x4 v = fsn_operand<AR>(f32x4{a, b, 0.f, 0.f});
        return (float)v[0] * (float)v[1];
    } else {
        const fsn_u32x2 v = __builtin_bit_cast(fsn_u32x2, fsn_operand<AR>(f32x4{a, b, 0.f, 0.f}));
        return __builtin_bit_cast(float, v[0] << 16) * __builtin_bit_cast(float, v[0] & 0xffff0000u);
    }
}
__global__ void tn_reduce_kernel(const float* __restrict__ part, float* __restrict__ C, long ldc, int M, int Nc,
                                 int splits, int transposed, const float* __restrict__ A, long lda,
                                 const float* __restrict__ B, long ldb, long k_tail0, long K, int accumulate, int arith) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * Nc) return;
    const int m = (int)(i / Nc), n = (int)(i % Nc);
    const long pi = transposed ? (long)n * M + m : i;
    float acc = 0.f;
    for (int s = 0; s < splits; ++s) acc += part[(long)s * M * Nc + pi];
    if (arith == FSN_ARITH_F16)
        for (long k = k_tail0; k < K; ++k) acc += tn_tail_term<FSN_ARITH_F16>(A[k * lda + m], B[k * ldb + n]);
    else if (arith == FSN_ARITH_BF16)
        for (long k = k_tail0; k < K; ++k) acc += tn_tail_term<FSN_ARITH_BF16>(A[k * lda + m], B[k * ldb + n]);
    else
        for (long k = k_tail0; k < K; ++k) acc += A[k * lda + m] * B[k * ldb + n];
    C[(long)m * ldc + n] = accumulate ? C[(long)m * ldc + n] + acc : acc;  // a later K segment (fsn_launch_gemm_tn)
}

// partial column sums over blocks of rows: part[rb][c] = sum_{r in block rb} A[r][c]
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ A, long lda,
                                                             float* __restrict__ part, int cols, long rows,
                                                             long rows_per_block) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    r1 = r1 < rows ? r1 : rows;
    // two levels, chains of 64 rows: one chain of 2048 made the sum of 2^20 rows four times less accurate than a blocked
    // CPU sum (tests/test_gpu_linear_sweep.py); up to 64 rows per block (every shipped shape) the bits are the same
    float acc = 0.f;
    for (long rc = r0; rc < r1; rc += 64) {
        const long re = rc + 64 < r1 ? rc + 64 : r1;
        float a = 0.f;
        for (long r = rc; r < re; ++r) a += A[r * lda + c];
        acc += a;
    }
    part[(long)blockIdx.y * cols + c] = acc;
}

// the same for at most 16 columns (the 2-wide output layer): 16 row groups x 16 columns per block instead of two
// busy threads; the row groups are combined in a fixed order
__global__ __launch_bounds__(256) void colsum_narrow_kernel(const float* __restrict__ A, long lda,
                                                            float* __restrict__ part, int cols, long rows,
                                                            long rows_per_block) {
    __shared__ float red[16][17];
    const int c = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const long r0 = (long)blockIdx.x * rows_per_block;
    long r1 = r0 + rows_per_block;
    r1 = r1 < rows ? r1 : rows;
    float acc = 0.f;
    if (c < cols)
        for (long r = r0 + rg; r < r1; r += 16) acc += A[r * lda + c];
    red[rg][c] = acc;
    __syncthreads();
    if (threadIdx.x < 16 && c < cols) {
        float t = 0.f;
        for (int g = 0; g < 16; ++g) t += red[g][c];
        part[(long)blockIdx.x * cols + c] = t;
    }
}

constexpr int TN_PF32 = 2;  // operand chunks in flight of the fp32 192 x 192 form (measured r04: 2 -> 3.76 ms, 3 -> 3.72: not latency-bound)
// (r04, tools/probe_tn.hip, profiles/r04_tn_probe.txt: without its operand loads this kernel's matrix stream runs at 0.98 of
// the fp32 peak, 3.03 ms, with them at 0.80, 3.67.  Three LDS-staged forms of the same product - 16-byte row pieces through
// registers with one / two chunks in flight, and by LDS-DMA with software-pipelined ds_read_b32 operands - measured 4.6 /
// 4.2 / 3.67 ms: the staged form only reaches the register ring's time (its DMA costs 0.3 ms, its LDS reads 0.2, its
// barrier 0.15), so the ring stays.)

constexpr long kColsumRows = 2048;
// rows per block of a column-sum launch: 2048, or fewer when that would leave most of the chip idle - the full-band
// output layer's 257 columns x 3120 rows ran on 4 workgroups walking 2048 rows each (0.46 ms; 49 blocks of 64: ~0.02)
static long colsum_rows_per_block(int cols, long rows) {
    long r = kColsumRows;
    const long col_blocks = cols <= 16 ? 1 : (cols + 255) / 256;
    while (r > 64 && ((rows + r - 1) / r) * col_blocks < 256) r >>= 1;
    return r;
}

}  // namespace

// Workgroup tile 256 x 128 (wave tile 8 x 4, waves 2 x 2) or, for narrow outputs (the K = 2nb+2
// input projection), 512 x 32 (wave tile 8 x 2, waves 4 x 1).  K is split so that the grid is one
// workgroup per CU (or as close below it as the tile count allows).
FsnTnPlan fsn_tn_plan(int M, int Nc, long K, int arith, bool allow_square) {
    FsnTnPlan p;
    const int cus = plan_cus();
    p.narrow = Nc <= 32;
    p.square = 0;
    (void)arith;  // every arithmetic: in fp32 the square plan is worth 0.3 ms of a 42 ms step, under the 16-bit one 1 ms per GEMM
    if (allow_square && M % 192 == 0 && Nc % 192 == 0 && cus % 8 == 0 && (cus / 8) % ((M / 192) * (Nc / 192)) == 0 &&
        K >= (long)(cus / ((M / 192) * (Nc / 192))) * 128) {
        const long s = cus / ((M / 192) * (Nc / 192));  // whole splits per XCD, one workgroup per CU
        const long kps = ((K + s - 1) / s + 15) / 16 * 16;
        if ((K + kps - 1) / kps == s) {  // every split non-empty (the kernel's grid is fixed by the XCD mapping)
            p.square = 1;
            p.m_blocks = M / 192;
            p.n_blocks = Nc / 192;
            p.k_per_split = kps;
            p.splits = (int)s;
            return p;
        }
    }
    p.m_blocks = p.narrow ? (M + 511) / 512 : (M + 255) / 256;
    p.n_blocks = p.narrow ? (Nc + 31) / 32 : (Nc + 127) / 128;
    const long tiles = (long)p.m_blocks * p.n_blocks;
    long s = cus / tiles;
    const long max_s = (K + 127) / 128;  // at least 8 chunks per split
    s = s < max_s ? s : max_s;
    s = s < 1 ? 1 : s;
    p.k_per_split = ((K + s - 1) / s + 15) / 16 * 16;
    p.splits = (int)((K + p.k_per_split - 1) / p.k_per_split);
    return p;
}

// The most K splits ANY plan of this (M, Nc) can take, whatever K: callers size one scratch buffer for several products
// of the same shape and slightly different K ((T - 1) N against T N rows), and the two plans split K differently (one
// workgroup per CU over 256 x 128 tiles, or over 192 x 192 tiles).  fsn_launch_gemm_tn refuses a plan beyond it.
long fsn_tn_max_splits(int M, int Nc) {
    const bool swap = M <= 32 && Nc > 32;
    const int cus = plan_cus();
    const int m = swap ? Nc : M, n = swap ? M : Nc;
    const bool narrow = n <= 32;
    const long tiles = narrow ? (long)((m + 511) / 512) * ((n + 31) / 32) : (long)((m + 255) / 256) * ((n + 127) / 128);
    long splits = cus / tiles > 1 ? cus / tiles : 1;
    if (!swap && M % 192 == 0 && Nc % 192 == 0) {
        const long sq = cus / ((long)(M / 192) * (Nc / 192));
        splits = sq > splits ? sq : splits;
    }
    if (!swap && M % 192 == 0 && Nc % 384 == 0) {  // the 192 x 384 form of the 16-bit-operand products: half as many tiles
        const long wq = cus / ((long)(M / 192) * (Nc / 384));
        splits = wq > splits ? wq : splits;
    }
    return splits;
}
// test hook (fsn_debug_tn_plan): the K splits of the product's plan and the bound its scratch is sized by.  A product that
// fsn_launch_gemm_tn forms in K segments (kTnLongChain) launches each segment with its own plan of at most that bound
void fsn_tn_plan_splits(int M, int Nc, long K, int arith, int* splits, long* bound) {
    const bool swap = M <= 32 && Nc > 32;
    const long K16 = K & ~15L;
    const FsnTnPlan p = K16 <= 0 ? FsnTnPlan{} : swap ? fsn_tn_plan(Nc, M, K16, arith, false) : fsn_tn_plan(M, Nc, K16, arith);
    if (splits) *splits = K16 <= 0 ? 1 : p.splits;
    if (bound) *bound = fsn_tn_max_splits(M, Nc);
}
size_t fsn_gemm_tn_workspace_bytes(int M, int Nc, long K) {
    if ((K & ~15L) <= 0) return (size_t)M * (Nc + 1) * sizeof(float);
    return (size_t)fsn_tn_max_splits(M, Nc) * M * (Nc + 1) * sizeof(float);  // + one column-sum row per split
}

constexpr long kTnLongChain = 4096;  // rows per K split from which fsn_launch_gemm_tn forms the product in K segments ...
constexpr long kTnSegChain = 2048;   // ... of this many rows per split
// One K segment of fsn_launch_gemm_tn: rows [0, K16) of A / B (K16 a multiple of 16, may be 0) through the MFMA kernel, the split
// partials summed into C (`accumulate`: onto an earlier segment's sum) together with rows [k_tail0, K_all) of A_all / B_all.
static int gemm_tn_segment(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int Nc, long K16,
                           float* part, hipStream_t s, float* colsum_out, int arith, bool swap, bool accumulate,
                           const float* A_all, const float* B_all, long k_tail0, long K_all) {
    float* asum_part = nullptr;
    int splits = 0;
    if (K16 > 0) {
        const FsnTnPlan p = swap ? fsn_tn_plan(Nc, M, K16, arith, false) : fsn_tn_plan(M, Nc, K16, arith);
        if (p.splits > fsn_tn_max_splits(M, Nc)) {  // the scratch buffer is sized by that bound
            fsn_set_error("gemm_tn: plan of %d splits for %d x %d exceeds the workspace bound", p.splits, M, Nc);
            return FSN_ERR_WORKSPACE;
        }
        if (colsum_out) asum_part = part + (size_t)p.splits * M * Nc;
        auto wide = arith == FSN_ARITH_F16    ? gemm_tn_kernel<8, 4, 2, 2, FSN_ARITH_F16>
                    : arith == FSN_ARITH_BF16 ? gemm_tn_kernel<8, 4, 2, 2, FSN_ARITH_BF16>
                                              : gemm_tn_kernel<8, 4, 2, 2>;
        auto narrow = arith == FSN_ARITH_F16    ? gemm_tn_kernel<8, 2, 4, 1, FSN_ARITH_F16>
                      : arith == FSN_ARITH_BF16 ? gemm_tn_kernel<8, 2, 4, 1, FSN_ARITH_BF16>
                                                : gemm_tn_kernel<8, 2, 4, 1>;
        const dim3 grid((unsigned)(p.m_blocks * p.n_blocks * p.splits));
        if (p.square && arith != FSN_ARITH_F32 && lda % 4 == 0 && ldb % 4 == 0 && ((size_t)A & 15) == 0 && ((size_t)B & 15) == 0) {
            // the 16-bit arithmetic's own kernel: 16-byte operand loads, transposing LDS reads
            auto k16 = arith == FSN_ARITH_F16 ? gemm_tn16_kernel<FSN_ARITH_F16> : gemm_tn16_kernel<FSN_ARITH_BF16>;
            FSN_TRY_RESERVE_LDS("gemm_tn", k16, kFsnTnOnePerCu);
            static_assert(TQ_LDS <= (int)kFsnTnOnePerCu, "the reservation that keeps one workgroup per CU holds the stages");
            hipLaunchKernelGGL(k16, grid, dim3(256), kFsnTnOnePerCu, s, A, lda, B, ldb, part, M, Nc, K16, p.k_per_split, p.m_blocks,
                               p.n_blocks, asum_part);
        } else if (p.square) {
            auto square = arith == FSN_ARITH_F16    ? gemm_tn_kernel<6, 6, 2, 2, FSN_ARITH_F16>
                          : arith == FSN_ARITH_BF16 ? gemm_tn_kernel<6, 6, 2, 2, FSN_ARITH_BF16>
                                                    : gemm_tn_kernel<6, 6, 2, 2, FSN_ARITH_F32, TN_PF32>;
            FSN_TRY_RESERVE_LDS("gemm_tn", square, kFsnTnOnePerCu);
            hipLaunchKernelGGL(square, grid, dim3(256), kFsnTnOnePerCu, s, A, lda, B, ldb, part, M, Nc, K16, p.k_per_split,
                               p.m_blocks, p.n_blocks, asum_part, 1);
        } else {
            auto kern = p.narrow ? narrow : wide;
            FSN_TRY_RESERVE_LDS("gemm_tn", kern, kFsnTnOnePerCu);
            if (swap)
                hipLaunchKernelGGL(kern, grid, dim3(256), kFsnTnOnePerCu, s, B, ldb, A, lda, part, Nc, M, K16, p.k_per_split,
                                   p.m_blocks, p.n_blocks, (float*)nullptr, 0);
            else
                hipLaunchKernelGGL(kern, grid, dim3(256), kFsnTnOnePerCu, s, A, lda, B, ldb, part, M, Nc, K16, p.k_per_split,
                                   p.m_blocks, p.n_blocks, asum_part, 0);
        }
        FSN_TRY_LAUNCH("gemm_tn_kernel");
        splits = p.splits;
    }
    const long n = (long)M * Nc;
    hipLaunchKernelGGL(tn_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, C, ldc, M, Nc, splits,
                       swap ? 1 : 0, A_all, lda, B_all, ldb, k_tail0, K_all, accumulate ? 1 : 0, arith);
    FSN_TRY_LAUNCH("tn_reduce_kernel");
    if (colsum_out) {
        hipLaunchKernelGGL(tn_colsum_reduce_kernel, dim3((M + 255) / 256), dim3(256), 0, s, asum_part, colsum_out, M,
                           splits, A_all, lda, k_tail0, K_all, accumulate ? 1 : 0);
        return fsn_check_launch("tn_colsum_reduce_kernel");
    }
    return FSN_OK;
}


// colsum_out (may be NULL): also out[m] = sum_k A[k][m], from the same pass over A (not with a narrow M)
int fsn_launch_gemm_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int Nc, long K,
                       void* workspace, hipStream_t s, float* colsum_out, int arith) {
    if (arith != FSN_ARITH_F32 && arith != FSN_ARITH_F16 && arith != FSN_ARITH_BF16) {
        fsn_set_error("gemm_tn: arithmetic %d unknown", arith);
        return FSN_ERR_ARG;
    }
    if (K <= 0 || lda * 16 > 0x7fffffffL || ldb * 16 > 0x7fffffffL) {
        fsn_set_error("gemm_tn: bad K = %ld or leading dimension", K);
        return FSN_ERR_ARG;
    }
    // a narrow M (the 2-row dW of the sub-band output layer) goes on the narrow side of the tile
    const bool swap = M <= 32 && Nc > 32;
    if (swap && colsum_out) {
        fsn_set_error("gemm_tn: fused column sums are not available for M <= 32");
        return FSN_ERR_ARG;
    }
    const long K16 = K & ~15L;
    float* part = static_cast<float*>(workspace);
    // K in SEGMENTS when one split's chain would be long.  A split is one fp32 accumulation chain; one workgroup per CU fixes
    // the split count, so the chain grows with K: 18 240 rows per split at K = 190 x 1536 (dW_hh of the sub-band pair) put the
    // product at 2.3e-6 of fp64 in relative Frobenius norm, 5 - 6 x torch's blocked fp32 sum
    // (tests/test_gpu_recurrent_sweep.py).  From kTnLongChain rows per split on, the product is formed in segments of
    // splits x kTnSegChain rows, each summed over its splits and added to C in a fixed order: three levels instead of two.
    // Cost: nseg launches of the product and of the reduction instead of one (9 at that K) and splits x M x Nc partials read
    // per segment (38 MB each there, against the 2.2 GB the product reads anyway); the training step's time with it has not been
    // measured.  fp32 only: the 16-bit arithmetics (this entry and gemm_tn16h / gemm_tn16n) keep one chain per split - their
    // operands are rounded to 8 - 11 bits, against which the chain's fp32 rounding does not show (tests/test_gpu_amp.py).
    long seg = K16 > 0 ? K16 : 0;
    int nseg = 1;
    if (K16 > 0) {
        const FsnTnPlan p0 = swap ? fsn_tn_plan(Nc, M, K16, arith, false) : fsn_tn_plan(M, Nc, K16, arith);
        if (arith == FSN_ARITH_F32 && p0.k_per_split > kTnLongChain) {
            nseg = (int)((K16 + (long)p0.splits * kTnSegChain - 1) / ((long)p0.splits * kTnSegChain));
            seg = ((K16 + nseg - 1) / nseg + 15) / 16 * 16;
            nseg = (int)((K16 + seg - 1) / seg);
        }
    }
    for (int sg = 0; sg < nseg; ++sg) {
        const long k0 = (long)sg * seg, Kc = K16 - k0 < seg ? K16 - k0 : seg;
        const bool last_seg = sg == nseg - 1;
        const int rc = gemm_tn_segment(A + k0 * lda, lda, B + k0 * ldb, ldb, C, ldc, M, Nc, Kc, part, s, colsum_out, arith, swap,
                                       sg > 0, A, B, last_seg ? K16 : K, K);
        if (rc != FSN_OK) return rc;
    }
    return FSN_OK;
}

size_t fsn_colsum_workspace_bytes(int cols, long rows) {
    const long r = colsum_rows_per_block(cols, rows);
    return (size_t)((rows + r - 1) / r) * cols * sizeof(float);
}

int fsn_launch_colsum(const float* A, long lda, float* out, int cols, long rows, void* workspace, hipStream_t s) {
    const long rpb = colsum_rows_per_block(cols, rows);
    const int rb = (int)((rows + rpb - 1) / rpb);
    float* part = static_cast<float*>(workspace);
    if (cols <= 16)
        hipLaunchKernelGGL(colsum_narrow_kernel, dim3(rb), dim3(256), 0, s, A, lda, part, cols, rows, rpb);
    else
        hipLaunchKernelGGL(colsum_partial_kernel, dim3((cols + 255) / 256, rb), dim3(256), 0, s, A, lda, part, cols, rows,
                           rpb);
    FSN_TRY_LAUNCH("colsum_partial_kernel");
    hipLaunchKernelGGL(reduce_splits_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, part, out, (long)cols, 1, cols,
                       rb);
    return fsn_check_launch("reduce_splits_kernel");
}
