// EXPERIMENT (not part of libfsn_hip.so): the sub-band layer-1 input projection, C[M][N] = A[M][K] W[N][K]^T with
// K = 384, N = 1536, as a split-precision GEMM: fp32 operands are split into two fp16 halves (a = a_hi + a_lo),
// three v_mfma_f32_16x16x32_f16 per product block (a_hi w_hi + a_hi w_lo + a_lo w_hi), fp32 accumulation.
// Same execution shape as the shipped fp32 GEMM (one 4-wave workgroup per CU, persistent over an XCD-partitioned
// tile list, operands straight from global / L2 into registers, pinned 1-deep prefetch); W is pre-split and
// pre-tiled, A is split on the fly (2 cvt + 1 sub per element, amortised over the 8 column tiles of a wave).
// Prints max error against an fp64 reference on a sample of rows and the sustained fp32-equivalent TFLOP/s.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

#ifndef PROBE_SKIP
#define PROBE_SKIP 0  // probe-only ablations: 1 = no C store, 2 = A fragments loaded once per tile (no A traffic in the K loop)
#endif
constexpr int K = 384, N = 1536, KC = K / 32;  // 12 chunks of 32
constexpr float SA = 64.f, SW = 256.f;          // power-of-two pre-scales keep the low halves out of fp16 subnormals

#define CK(x)                                                                     \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

// W [N][K] fp32 -> whi / wlo in B-fragment order [N/16][KC][64 lanes][8 halves]:
// lane l of tile (ct, kc) holds W[16 ct + (l & 15)][32 kc + 8 (l >> 4) .. + 7]
__global__ void pack_split_kernel(const float* __restrict__ w, _Float16* __restrict__ whi, _Float16* __restrict__ wlo) {
    const long total = (long)(N / 16) * KC * 64 * 8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
        const long blk = i >> 9;
        const int kc = (int)(blk % KC), ct = (int)(blk / KC);
        const float v = w[(long)(ct * 16 + (lane & 15)) * K + kc * 32 + 8 * (lane >> 4) + j] * SW;
        const _Float16 h = (_Float16)v;
        whi[i] = h;
        wlo[i] = (_Float16)(v - (float)h);
    }
}

__device__ __forceinline__ void split8(const f32x4 x0, const f32x4 x1, f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float v = (j < 4 ? x0[j] : x1[j - 4]) * SA;
        const _Float16 h = (_Float16)v;
        hi[j] = h;
        lo[j] = (_Float16)(v - (float)h);
    }
}

template <int RTW, int CTW>  // wave tile in 16 x 16 tiles; workgroup = 2 x 2 waves
__global__ __launch_bounds__(256) void gemm_f16x3_kernel(const float* __restrict__ A, const f16x8* __restrict__ whi,
                                                         const f16x8* __restrict__ wlo, float* __restrict__ C,
                                                         long M) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const long row_tiles = M / 16;
    const unsigned ncb = (N / 16) / (2 * CTW);
    const unsigned nrb = (unsigned)((row_tiles + 2 * RTW - 1) / (2 * RTW));
    const unsigned ntiles = nrb * ncb;
    // XCD x owns a contiguous range of the tile list (block b runs on XCD b % 8 - speed only)
    const unsigned xcd = blockIdx.x & 7u, lid = blockIdx.x >> 3, lstride = (gridDim.x + 7u - xcd) >> 3;
    const unsigned tq = ntiles >> 3, tr = ntiles & 7u;
    const unsigned tbeg = xcd < tr ? xcd * (tq + 1) : tr * (tq + 1) + (xcd - tr) * tq;
    const unsigned tcnt = tq + (xcd < tr ? 1u : 0u);
    for (unsigned ti = lid; ti < tcnt; ti += lstride) {
        const unsigned v = tbeg + ti;
        const unsigned rb = v / ncb, cb = v % ncb;
        const long rtile0 = ((long)rb * 2 + wr) * RTW;
        const int ctile0 = ((int)cb * 2 + wc) * CTW;
        const float* arow[RTW];
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt) {
            long row = (rtile0 + rt) * 16 + (lane & 15);
            row = row < M ? row : M - 1;
            arow[rt] = A + row * K + 8 * (lane >> 4);
        }
        f32x4 acc[RTW][CTW];
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        // operand rings: A (fp32, from HBM) is requested APF chunks ahead, the L2-resident W halves one chunk ahead
        constexpr int APF = 2;
        f32x4 araw[APF][RTW][2];
        f16x8 bh[CTW], bl[CTW];
        auto fetch_a = [&](int slot, int kc) {
#pragma unroll
            for (int rt = 0; rt < RTW; ++rt) {
                if (PROBE_SKIP == 2 && kc >= APF) continue;
                araw[slot][rt][0] = *reinterpret_cast<const f32x4*>(arow[rt] + kc * 32);
                araw[slot][rt][1] = *reinterpret_cast<const f32x4*>(arow[rt] + kc * 32 + 4);
            }
        };
        auto fetch_b = [&](int kc) {
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct) {
                const long o = ((long)(ctile0 + ct) * KC + kc) * 64 + lane;
                bh[ct] = whi[o];
                bl[ct] = wlo[o];
            }
        };
#pragma unroll
        for (int p = 0; p < APF; ++p) fetch_a(p, p);
        fetch_b(0);
        static_assert(KC % APF == 0, "ring slots are compile-time indices");
        // the split of chunk k + 1 (VALU) is issued together with the MFMAs of chunk k, so that the two pipes overlap
        f16x8 ah[RTW], al[RTW];
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt) split8(araw[0][rt][0], araw[0][rt][1], ah[rt], al[rt]);
        for (int kc0 = 0; kc0 < KC; kc0 += APF) {
#pragma unroll
            for (int p = 0; p < APF; ++p) {
                const int kc = kc0 + p;
                f16x8 ch[CTW], cl[CTW], ahn[RTW], aln[RTW];
#pragma unroll
                for (int ct = 0; ct < CTW; ++ct) {
                    ch[ct] = bh[ct];
                    cl[ct] = bl[ct];
                }
                // slot p's raw chunk was converted during the previous iteration: refill it (clamped at the end)
                __builtin_amdgcn_sched_barrier(0);
                fetch_a(p, kc + APF < KC ? kc + APF : KC - 1);
                fetch_b(kc + 1 < KC ? kc + 1 : kc);
                __builtin_amdgcn_sched_barrier(0);
                constexpr int pn = (APF == 1) ? 0 : 1;  // next chunk sits in the other slot (APF == 2)
                // the three terms of a tile go to the same accumulator: issue them a whole tile sweep apart, never
                // back to back (a dependent MFMA waits out the full latency of its predecessor)
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) {
                    split8(araw[(p + pn) % APF][rt][0], araw[(p + pn) % APF][rt][1], ahn[rt], aln[rt]);
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], ch[ct], acc[rt][ct], 0, 0, 0);
                }
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], cl[ct], acc[rt][ct], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
                    for (int ct = 0; ct < CTW; ++ct)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt], ch[ct], acc[rt][ct], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RTW; ++rt) {
                    ah[rt] = ahn[rt];
                    al[rt] = aln[rt];
                }
            }
        }
        // acc register i of lane l is C[16 rtile + 4 (l >> 4) + i][16 ctile + (l & 15)]
        const float unscale = 1.0f / (SA * SW);
        // stored like the product's gx: accumulator-fragment order, tile (rtile, ctile) = one 1 KB block [lane][4]
#pragma unroll
        for (int rt = 0; rt < RTW; ++rt)
#pragma unroll
            for (int ct = 0; ct < CTW; ++ct)
                if (rtile0 + rt < row_tiles && (PROBE_SKIP != 1 || acc[rt][ct][0] == 12345.678f)) {
                    const f32x4 a = acc[rt][ct];
                    *reinterpret_cast<f32x4*>(C + (((rtile0 + rt) * (N / 16) + ctile0 + ct) * 64 + lane) * 4) =
                        f32x4{a[0] * unscale, a[1] * unscale, a[2] * unscale, a[3] * unscale};
                }
    }
}

__global__ void fill_kernel(float* p, size_t n, unsigned seed, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned x = (unsigned)i * 747796405u + seed;
        x ^= x >> 16;
        x *= 2246822519u;
        x ^= x >> 13;
        p[i] = ((x & 0xffff) / 32768.0f - 1.0f) * scale;
    }
}

int main(int argc, char** argv) {
    const long M = argc > 1 ? atol(argv[1]) : 790400;  // rows: 16 utterances x 190 frames x 260 (as probe_gemm.hip)
    float *A, *W, *C;
    _Float16 *whi, *wlo;
    CK(hipMalloc(&A, (size_t)M * K * 4));
    CK(hipMalloc(&W, (size_t)N * K * 4));
    CK(hipMalloc(&C, (size_t)M * N * 4));
    CK(hipMalloc(&whi, (size_t)N * K * 2));
    CK(hipMalloc(&wlo, (size_t)N * K * 2));
    fill_kernel<<<4096, 256>>>(A, (size_t)M * K, 1, 1.0f);    // hidden states live in (-1, 1)
    fill_kernel<<<256, 256>>>(W, (size_t)N * K, 2, 0.05f);    // U(-1/sqrt(H), 1/sqrt(H))
    pack_split_kernel<<<1024, 256>>>(W, whi, wlo);
    CK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    // one workgroup per CU, like the shipped GEMM (96 KB LDS reservation it never touches)
    auto kern = gemm_f16x3_kernel<4, 8>;
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    float best = 1e30f;
    for (int it = 0; it < 4; ++it) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(kern, dim3(256), dim3(256), 96 * 1024, 0, A, reinterpret_cast<const f16x8*>(whi),
                           reinterpret_cast<const f16x8*>(wlo), C, M);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (it > 0 && ms < best) best = ms;
    }
    const double flops = 2.0 * M * K * N;
    // accuracy on a sample of rows against fp64
    const int SR = 64;
    std::vector<float> hA((size_t)SR * K), hW((size_t)N * K), hC((size_t)SR * N);
    const long r0 = M / 3 / 16 * 16;
    CK(hipMemcpy(hA.data(), A + r0 * K, hA.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hW.data(), W, hW.size() * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hC.data(), C + r0 * N, hC.size() * 4, hipMemcpyDeviceToHost));
    double max_err = 0, max_ref = 0, max_err32 = 0;
    for (int r = 0; r < SR; ++r)
        for (int n = 0; n < N; ++n) {
            double ref = 0;
            float f32 = 0.f;
            for (int k = 0; k < K; ++k) {
                ref += (double)hA[(size_t)r * K + k] * hW[(size_t)n * K + k];
                f32 = fmaf(hA[(size_t)r * K + k], hW[(size_t)n * K + k], f32);
            }
            const size_t fo = (((size_t)(r / 16) * (N / 16) + n / 16) * 64 + (n % 16) + 16 * ((r % 16) / 4)) * 4 + r % 4;
            max_err = fmax(max_err, fabs(hC[fo] - ref));
            max_err32 = fmax(max_err32, fabs((double)f32 - ref));
            max_ref = fmax(max_ref, fabs(ref));
        }
    printf("f16x3 GEMM %ld x %d x %d: %.3f ms = %.1f fp32-equivalent TFLOP/s; max |err| vs fp64 %.3e (plain fp32 "
           "fma chain: %.3e), max |C| %.3f\n", M, K, N, best, flops / best / 1e9, max_err, max_err32, max_ref);
    return 0;
}
