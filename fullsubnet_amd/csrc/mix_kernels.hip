// Training pairs mixed on the device (fsn_conv_rows / fsn_mix_pairs, include/fsn_hip.h): the per-item arithmetic of
// recipes/dns_interspeech_2020/dataset_train.py:137-195 (Dataset.snr_mix) for gfx950.
//
//   mix_gather_kernel     clean crop + zero pad, noise row from its segments                    slabs -> c0, nz
//   conv_cols_fwd_kernel  z = x + i h, column transforms of the four-step FFT + step twiddle     x, h  -> Z
//   conv_rows_kernel      row transforms, Hermitian split and product, inverse row transforms    Z     -> Z
//   conv_cols_inv_kernel  inverse column transforms, real part, first L samples                  Z     -> y
//   mix_level_kernel      the five reductions, the scalars of snr_mix, the clip branch, the write c, nz -> noisy, clean
//   rir_shorten_kernel    arg-max of |h|, window, product (reverberation_time_shortening)         h     -> shortened h
//
// The FFT convolution (circular length N = N1 N2 = 2^k): the signal goes into the real part and the response into the
// imaginary part of ONE complex transform; with n = N2 n1 + n2 and k = k1 + N1 k2
//     Z[k1 + N1 k2] = sum_n2 W_N2^(n2 k2) W_N^(n2 k1) sum_n1 z[N2 n1 + n2] W_N1^(n1 k1),
// columns (over n1, stride N2) first, rows (over n2, contiguous) second.  The sub-transforms are radix-2 in LDS, decimation
// in frequency forwards (natural in, bit-reversed out) and decimation in time backwards (bit-reversed in, natural out), so
// nothing is ever reordered: matrix row p holds k1 = bitrev(p), LDS slot q of a row holds k2 = bitrev(q).  X H follows
// from Z through the Hermitian split, Y[k] = (Z[k]^2 - conj(Z[N - k])^2) / 4i; the partner of (k1, k2) sits in row N1 - k1,
// so one workgroup takes both rows, forms the product in LDS and runs the inverse row transforms at once: Z is written once
// by the first kernel, read and written once by the second, read once by the third.  Everything is fp64 (twiddles from
// sincospi of exact arguments): the result is the fp32 rounding of the exact convolution of the fp32 inputs, and the
// transforms stay a small part of the call (profiles/mix_pairs.md).
#include "fsn_common.h"

namespace {

#include "fft64_lds.h"  // cd, cadd / csub / cmul, bitrev, fill_twiddles, lds_fft

__device__ __forceinline__ float slab_sample(const void* slab, int fmt, long i) {
    return fmt == FSN_SLAB_I16 ? (float)static_cast<const short*>(slab)[i] * (1.0f / 32768.0f)
                               : static_cast<const float*>(slab)[i];
}

constexpr int kThreads = kFftThreads;
constexpr int kMaxSub = 512;  // longest sub-transform: N <= 2^18 = 512 x 512
constexpr int kCols = 4;      // columns of the N1 x N2 matrix per workgroup of the column kernels

// e^(-+ 2 pi i m / N) for 0 <= m < N (forward: minus)
template <bool INV>
__device__ __forceinline__ cd step_twiddle(int m, int N) {
    double s, c;
    sincospi((INV ? 2.0 : -2.0) * (double)m / (double)N, &s, &c);
    return cd{c, s};
}

// Offsets and lengths of the rows' responses: two arrays (fsn_conv_rows) or fields of the item table (fsn_mix_pairs)
struct Taps {
    const char* off;
    const char* len;
    int off_stride, len_stride;
    __device__ __forceinline__ long offset(int b) const { return *reinterpret_cast<const long*>(off + (long)b * off_stride); }
    __device__ __forceinline__ int length(int b) const { return *reinterpret_cast<const int*>(len + (long)b * len_stride); }
};

struct ConvGeom {
    int L, N, N1, N2, log1, log2;
    int planned;  // 0: the workspace holds no transform (sized for max_h_len = 0); N1 x N2 only indexes the row
};

// The taps of row b that take part (0: the row is copied; -1: more than the transform carries, the row becomes NaN).
__device__ __forceinline__ int row_taps(const Taps& t, int b, const ConvGeom& g) {
    int hl = t.length(b);
    if (hl <= 0) return 0;
    hl = hl < g.L ? hl : g.L;
    return g.planned && g.L + hl - 1 <= g.N ? hl : -1;
}

// grid (ceil(N2 / kCols), B)
__global__ __launch_bounds__(kThreads) void conv_cols_fwd_kernel(const float* __restrict__ x, const void* __restrict__ h_slab,
                                                                 int fmt, Taps taps, cd* __restrict__ Z,
                                                                 int* __restrict__ live, ConvGeom g) {
    __shared__ cd a[kCols * kMaxSub];
    __shared__ cd tw[kMaxSub / 2];
    const int b = blockIdx.y;
    const int hl = row_taps(taps, b, g);
    if (hl <= 0) return;
    const long ho = taps.offset(b);
    const int c0 = blockIdx.x * kCols, M = g.N1;
    const float* xr = x + (long)b * g.L;
    fill_twiddles(tw, M);
    bool nzx = false, nzh = false;
    for (int i = threadIdx.x; i < kCols * M; i += kThreads) {
        const int c = i % kCols, n1 = i / kCols, n2 = c0 + c;
        const long n = (long)n1 * g.N2 + n2;
        cd v{0.0, 0.0};
        if (n2 < g.N2) {
            if (n < g.L) v.x = (double)xr[n];
            if (n < hl) v.y = (double)slab_sample(h_slab, fmt, ho + n);
        }
        nzx |= v.x != 0.0;
        nzh |= v.y != 0.0;
        a[c * M + n1] = v;
    }
    // a row of zeros (digital silence) or a response of zeros convolves to zeros, not to the split's rounding residue
    // (~1e-17 of the partner, which the levelling that follows would scale up to full level): live[b] bit 0 / bit 1 say
    // that the signal / the response has a non-zero sample; the last kernel writes zeros unless both are set
    const int bits = (__syncthreads_or(nzx) ? 1 : 0) | (__syncthreads_or(nzh) ? 2 : 0);
    if (threadIdx.x == 0 && bits) atomicOr(&live[b], bits);
    lds_fft<false>(a, tw, M, g.log1, kCols);
    cd* Zr = Z + (long)b * g.N;
    for (int i = threadIdx.x; i < kCols * M; i += kThreads) {
        const int c = i % kCols, p = i / kCols, n2 = c0 + c;
        if (n2 >= g.N2) continue;
        const int k1 = bitrev(p, g.log1);
        const int m = (int)(((long)n2 * k1) & (g.N - 1));
        Zr[(long)p * g.N2 + n2] = cmul(a[c * M + p], step_twiddle<false>(m, g.N));
    }
}

// grid (N1 / 2 + 1, B): rows k1 = blockIdx.x and N1 - k1 of the matrix
__global__ __launch_bounds__(kThreads) void conv_rows_kernel(Taps taps, cd* __restrict__ Z, ConvGeom g) {
    __shared__ cd a[2 * kMaxSub];
    __shared__ cd tw[kMaxSub / 2];
    const int b = blockIdx.y;
    if (row_taps(taps, b, g) <= 0) return;
    const int M = g.N2;
    const int k1a = blockIdx.x, k1b = (g.N1 - k1a) & (g.N1 - 1);
    const int rows = k1b != k1a ? 2 : 1;
    const int pa = bitrev(k1a, g.log1), pb = bitrev(k1b, g.log1);
    cd* Zr = Z + (long)b * g.N;
    fill_twiddles(tw, M);
    for (int i = threadIdx.x; i < rows * M; i += kThreads) {
        const int r = i / M, q = i - r * M;
        a[i] = Zr[(long)(r ? pb : pa) * M + q];
    }
    __syncthreads();
    lds_fft<false>(a, tw, M, g.log2, rows);
    // a[r][q] = Z[k1_r + N1 bitrev(q)].  Y[k] = (Z[k]^2 - conj(Z[N - k])^2) / (4 i N), 1 / N the inverse transform's scale
    constexpr int kPer = 2 * kMaxSub / kThreads;
    cd y[kPer];
    const double scale = 0.25 / (double)g.N;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int i = threadIdx.x + e * kThreads;
        y[e] = cd{0.0, 0.0};
        if (i >= rows * M) continue;
        const int r = i / M, q = i - r * M;
        const int k2 = bitrev(q, g.log2);
        const int k1 = r ? k1b : k1a;
        // N - k = (N1 - k1) + N1 (N2 - 1 - k2) for k1 > 0, N1 ((N2 - k2) mod N2) for k1 = 0
        const int k2p = k1 == 0 ? ((M - k2) & (M - 1)) : M - 1 - k2;
        const int rp = rows == 2 ? 1 - r : r;
        const cd zk = a[i], zp = a[rp * M + bitrev(k2p, g.log2)];
        const double dx = (zk.x * zk.x - zk.y * zk.y) - (zp.x * zp.x - zp.y * zp.y);
        const double dy = 2.0 * zk.x * zk.y + 2.0 * zp.x * zp.y;
        y[e] = cd{dy * scale, -dx * scale};
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const int i = threadIdx.x + e * kThreads;
        if (i < rows * M) a[i] = y[e];
    }
    __syncthreads();
    lds_fft<true>(a, tw, M, g.log2, rows);
    for (int i = threadIdx.x; i < rows * M; i += kThreads) {
        const int r = i / M, n2 = i - r * M;
        const int k1 = r ? k1b : k1a;
        const int m = (int)(((long)n2 * k1) & (g.N - 1));
        Zr[(long)(r ? pb : pa) * M + n2] = cmul(a[i], step_twiddle<true>(m, g.N));
    }
}

// grid (ceil(N2 / kCols), B)
__global__ __launch_bounds__(kThreads) void conv_cols_inv_kernel(const float* __restrict__ x, Taps taps,
                                                                 const cd* __restrict__ Z, const int* __restrict__ live,
                                                                 float* __restrict__ y, ConvGeom g) {
    __shared__ cd a[kCols * kMaxSub];
    __shared__ cd tw[kMaxSub / 2];
    const int b = blockIdx.y;
    const int hl = row_taps(taps, b, g);
    const int c0 = blockIdx.x * kCols, M = g.N1;
    float* yr = y + (long)b * g.L;
    const bool zeros = hl > 0 && live[b] != 3;
    if (hl <= 0 || zeros) {
        const float* xr = x + (long)b * g.L;
        for (int i = threadIdx.x; i < kCols * M; i += kThreads) {
            const int c = i % kCols, n1 = i / kCols, n2 = c0 + c;
            const long n = (long)n1 * g.N2 + n2;
            if (n2 < g.N2 && n < g.L) yr[n] = zeros ? 0.f : (hl == 0 ? xr[n] : __builtin_nanf(""));
        }
        return;
    }
    const cd* Zr = Z + (long)b * g.N;
    fill_twiddles(tw, M);
    for (int i = threadIdx.x; i < kCols * M; i += kThreads) {
        const int c = i % kCols, p = i / kCols, n2 = c0 + c;
        a[c * M + p] = n2 < g.N2 ? Zr[(long)p * g.N2 + n2] : cd{0.0, 0.0};
    }
    __syncthreads();
    lds_fft<true>(a, tw, M, g.log1, kCols);
    for (int i = threadIdx.x; i < kCols * M; i += kThreads) {
        const int c = i % kCols, n1 = i / kCols, n2 = c0 + c;
        const long n = (long)n1 * g.N2 + n2;
        if (n2 < g.N2 && n < g.L) yr[n] = (float)a[c * M + n1].x;
    }
}

// grid (ceil(L / 256), B, 2): z = 0 the clean row, z = 1 the noise row
__global__ __launch_bounds__(kThreads) void mix_gather_kernel(const void* __restrict__ clean_slab,
                                                              const void* __restrict__ noise_slab, int fmt,
                                                              const fsn_mix_item* __restrict__ items,
                                                              const fsn_mix_seg* __restrict__ segs, int n_segs, int L,
                                                              float* __restrict__ c0, float* __restrict__ nz) {
    const int b = blockIdx.y;
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= L) return;
    const fsn_mix_item it = items[b];
    float v = 0.f;
    if (blockIdx.z == 0) {
        if (n < it.clean_len) v = slab_sample(clean_slab, fmt, it.clean_off + n);
        c0[(long)b * L + n] = v;
    } else {
        // the segment table's slice, clamped to the table; the first segment that covers the sample wins
        const int s0 = it.seg_begin < 0 ? 0 : it.seg_begin;
        const long s1l = (long)s0 + (it.seg_count < 0 ? 0 : it.seg_count);
        const int s1 = s1l > n_segs ? n_segs : (int)s1l;
        for (int s = s0; s < s1; ++s) {
            const fsn_mix_seg sg = segs[s];
            const long d = (long)n - sg.dst_off;
            if (d >= 0 && d < sg.len) {
                v = slab_sample(noise_slab, fmt, sg.src_off + d);
                break;
            }
        }
        nz[(long)b * L + n] = v;
    }
}

constexpr int kLevelThreads = 1024;

// max of v over the workgroup, every thread gets it (the maximum is exact in any order)
__device__ __forceinline__ double block_max(double v, double* scratch) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double m = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, scratch[w]);
    return m;
}

// One workgroup per row: max|c|, sum c^2, max|n|, sum n^2, sum c n in fp64 (fixed order), the scalars of snr_mix from
// them, then noisy = (A c + G n) s3 and clean = A c s3, the clip check on max|noisy| and the single fp32 rounding.
// TARGET: a third row under the clean row's scalars, target = A t s3 with t the clean row convolved with the shortened
// response (c2), or the reverberant row itself where there is none (t_len[b] == 0); clean may then be NULL.  Every
// scalar still comes from c and nz alone, so noisy and clean keep the bits of the two-row form.
template <bool TARGET>
__global__ __launch_bounds__(kLevelThreads) void mix_level_kernel(const float* __restrict__ c, const float* __restrict__ nz,
                                                                  const fsn_mix_item* __restrict__ items, int L, double eps,
                                                                  float* __restrict__ noisy, float* __restrict__ clean,
                                                                  const float* __restrict__ c2, const int* __restrict__ t_len,
                                                                  float* __restrict__ target) {
    __shared__ double scratch[kLevelThreads / 64];
    const int b = blockIdx.x;
    const fsn_mix_item it = items[b];
    const float* cr = c + (long)b * L;
    const float* nr = nz + (long)b * L;
    double mc = 0.0, mn = 0.0, scc = 0.0, snn = 0.0, scn = 0.0;
    for (int i = threadIdx.x; i < L; i += kLevelThreads) {
        const double cv = (double)cr[i], nv = (double)nr[i];
        mc = fmax(mc, fabs(cv));
        mn = fmax(mn, fabs(nv));
        scc = fma(cv, cv, scc);
        snn = fma(nv, nv, snn);
        scn = fma(cv, nv, scn);
    }
    mc = block_max(mc, scratch);
    mn = block_max(mn, scratch);
    scc = fsn_block_sum(scc, scratch);
    snn = fsn_block_sum(snn, scratch);
    scn = fsn_block_sum(scn, scratch);

    const double inv_l = 1.0 / (double)L;
    const double tgt = pow(10.0, (double)it.target_dbfs / 20.0);
    // step 2: c / (max|c| + eps), levelled to the target; A and Gn take a raw sample to its levelled value
    const double rms_c = sqrt(scc * inv_l) / (mc + eps), s1 = tgt / (rms_c + eps);
    const double rms_n = sqrt(snn * inv_l) / (mn + eps), s2 = tgt / (rms_n + eps);
    const double A = s1 / (mc + eps), Gn = s2 / (mn + eps);
    const double clean_rms = rms_c * s1, noise_rms = rms_n * s2;
    // step 3
    const double gain = clean_rms / pow(10.0, (double)it.snr_db / 20.0) / (noise_rms + eps);
    const double G = gain * Gn;
    // step 4: rms of A c + G n from the sums
    double ss = A * A * scc + 2.0 * A * G * scn + G * G * snn;
    ss = ss > 0.0 ? ss : 0.0;
    const double s3 = pow(10.0, (double)it.noisy_target_dbfs / 20.0) / (sqrt(ss * inv_l) + eps);
    const double a3 = A * s3, g3 = G * s3;
    // step 5
    double peak = 0.0;
    for (int i = threadIdx.x; i < L; i += kLevelThreads)
        peak = fmax(peak, fabs(fma(a3, (double)cr[i], g3 * (double)nr[i])));
    peak = block_max(peak, scratch);
    const double d = peak > 0.999 ? (0.99 - eps) / peak : 1.0;
    float* yn = noisy + (long)b * L;
    if (!TARGET) {
        float* yc = clean + (long)b * L;
        for (int i = threadIdx.x; i < L; i += kLevelThreads) {
            const double cv = a3 * (double)cr[i];
            yn[i] = (float)(fma(g3, (double)nr[i], cv) * d);
            yc[i] = (float)(cv * d);
        }
    } else {
        const float* tr = t_len[b] > 0 ? c2 + (long)b * L : cr;
        float* yc = clean ? clean + (long)b * L : nullptr;
        float* yt = target + (long)b * L;
        for (int i = threadIdx.x; i < L; i += kLevelThreads) {
            const double cv = a3 * (double)cr[i];
            yn[i] = (float)(fma(g3, (double)nr[i], cv) * d);
            if (yc) yc[i] = (float)(cv * d);
            yt[i] = (float)(a3 * (double)tr[i] * d);
        }
    }
}

// ---- fsn_rir_shorten: audio_zen/acoustics/rvb.py (reverberation_time_shortening) on a table of responses ---------------
constexpr int kShortenThreads = 1024;
constexpr int kTapRun = 8;  // consecutive taps per thread and pass: 16 bytes of PCM, two 16-byte words of fp32

// np.argmax(np.abs(h)): the larger value wins, among equal values the LOWER index - in any order of combination
struct Peak {
    float v;
    int i;
};
__device__ __forceinline__ Peak higher(Peak a, Peak b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }

// taps [n, n + kTapRun) of a response of hl taps that starts at sample `at` of the slab, zeros from hl on; vec: the run's
// first byte is 16-byte aligned (n is a multiple of kTapRun, so the row's first byte decides for the whole row)
__device__ __forceinline__ void load_taps(const void* slab, int fmt, long at, int n, int hl, bool vec, float (&t)[kTapRun]) {
    if (vec && n + kTapRun <= hl) {
        if (fmt == FSN_SLAB_I16) {
            const int4 r = *reinterpret_cast<const int4*>(static_cast<const short*>(slab) + at + n);
            const int w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t[2 * j] = (float)(short)(w[j] & 0xffff) * (1.0f / 32768.0f);
                t[2 * j + 1] = (float)(short)(w[j] >> 16) * (1.0f / 32768.0f);
            }
        } else {
            const float4* p = reinterpret_cast<const float4*>(static_cast<const float*>(slab) + at + n);
            const float4 a = p[0], b = p[1];
            t[0] = a.x, t[1] = a.y, t[2] = a.z, t[3] = a.w, t[4] = b.x, t[5] = b.y, t[6] = b.z, t[7] = b.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kTapRun; ++j) t[j] = n + j < hl ? slab_sample(slab, fmt, at + n + j) : 0.f;
    }
}

__device__ __forceinline__ void store_taps(float* row, int n, int ld, bool vec, const float (&t)[kTapRun]) {
    if (vec && n + kTapRun <= ld) {
        float4* p = reinterpret_cast<float4*>(row + n);
        p[0] = float4{t[0], t[1], t[2], t[3]};
        p[1] = float4{t[4], t[5], t[6], t[7]};
    } else {
#pragma unroll
        for (int j = 0; j < kTapRun; ++j)
            if (n + j < ld) row[n + j] = t[j];
    }
}

// grid (B): one workgroup per response.  Pass 1: the peak of |h| over the WHOLE response, per thread in rising index
// order, then over the wave by shuffles and over the waves in LDS - a fixed tree, and `higher` makes the result the one
// of np.argmax whatever the tree.  Pass 2: the window in fp64 (exp10 of x = -q (n - N1), one rounded product as numpy
// forms it; an fp64 pow(10, x) costs about twice as much and most of this kernel's time), its fp32 rounding, and
// out = h * win as one fp32 product, for the first ld taps.
__global__ __launch_bounds__(kShortenThreads) void rir_shorten_kernel(const void* __restrict__ h_slab, int fmt, Taps taps,
                                                                      const fsn_mix_target* __restrict__ targets,
                                                                      float* __restrict__ out, int ld, float* __restrict__ win,
                                                                      int* __restrict__ idx_out, long* __restrict__ t_off,
                                                                      int* __restrict__ t_len) {
    __shared__ Peak wave_peak[kShortenThreads / 64];
    const int b = blockIdx.x;
    const int len = taps.length(b);
    const int hl = len > 0 && h_slab ? len : 0;  // no slab (a workspace without a transform): nothing is read
    const long at = hl ? taps.offset(b) : 0;
    const fsn_mix_target tg = targets[b];
    const bool known = tg.mode >= 0 && tg.mode <= 2;
    const bool windowed = tg.mode == 1 || tg.mode == 2;
    const size_t sample = fmt == FSN_SLAB_I16 ? sizeof(short) : sizeof(float);
    const bool src16 = ((reinterpret_cast<uintptr_t>(h_slab) + (size_t)at * sample) & 15) == 0;
    float t[kTapRun];

    int idx = 0;
    if (windowed || idx_out) {
        Peak pk{-1.f, 0x7fffffff};
        for (int n = threadIdx.x * kTapRun; n < hl; n += kShortenThreads * kTapRun) {
            load_taps(h_slab, fmt, at, n, hl, src16, t);
#pragma unroll
            for (int j = 0; j < kTapRun; ++j) {
                const float a = fabsf(t[j]);
                if (n + j < hl && a > pk.v) pk = Peak{a, n + j};
            }
        }
        for (int o = 32; o > 0; o >>= 1) pk = higher(pk, Peak{__shfl_down(pk.v, o, 64), __shfl_down(pk.i, o, 64)});
        if ((threadIdx.x & 63) == 0) wave_peak[threadIdx.x >> 6] = pk;
        __syncthreads();
        pk = wave_peak[0];
        for (int w = 1; w < kShortenThreads / 64; ++w) pk = higher(pk, wave_peak[w]);
        idx = pk.v < 0.f ? 0 : pk.i;  // an empty response, or one of NaNs alone
    }
    if (threadIdx.x == 0) {
        if (idx_out) idx_out[b] = idx;
        if (t_len) {
            t_off[b] = (long)b * ld;
            t_len[b] = tg.mode != 0 && len > 0 ? (len < ld ? len : ld) : 0;
        }
    }

    // as the taps of a convolution (t_len given) only what it reads is written: nothing for a row without a shortened
    // response, no zeros behind the others
    if (t_len && (tg.mode == 0 || hl == 0)) return;
    const int end = t_len && hl < ld ? hl : ld;
    const long n1 = (long)idx + tg.after_max;
    float* orow = out + (long)b * ld;
    float* wrow = win ? win + (long)b * ld : nullptr;
    const bool dst16 = ((reinterpret_cast<uintptr_t>(orow) | reinterpret_cast<uintptr_t>(wrow)) & 15) == 0;
    for (int n = threadIdx.x * kTapRun; n < end; n += kShortenThreads * kTapRun) {
        load_taps(h_slab, fmt, at, n, hl, src16, t);
        float w[kTapRun];
#pragma unroll
        for (int j = 0; j < kTapRun; ++j) {
            const long m = (long)n + j;
            float wv = 0.f;
            if (m < hl) {
                if (!known)
                    wv = __builtin_nanf("");
                else if (!windowed || m < n1)
                    wv = 1.f;
                else if (tg.mode == 1)
                    wv = (float)exp10(-tg.q * (double)(m - n1));
            }
            w[j] = wv;
            t[j] = t[j] * wv;
        }
        store_taps(orow, n, ld, dst16, t);
        if (wrow) store_taps(wrow, n, ld, dst16, w);
    }
}

}  // namespace

// N = 2^logN = N1 N2 with N1 <= N2 <= 512
static ConvGeom conv_geom(int L, int logN, bool planned) {
    ConvGeom g;
    g.planned = planned ? 1 : 0;
    g.L = L;
    g.N = 1 << logN;
    g.log1 = logN / 2;
    g.log2 = logN - g.log1;
    g.N1 = 1 << g.log1;
    g.N2 = 1 << g.log2;
    return g;
}

int fsn_launch_conv_rows(const float* x, int B, int L, const void* h_slab, int fmt, const void* h_off, int off_stride,
                         const void* h_len, int len_stride, float* y, void* Z, int* live, int logN, hipStream_t s) {
    const Taps taps{static_cast<const char*>(h_off), static_cast<const char*>(h_len), off_stride, len_stride};
    const ConvGeom g = conv_geom(L, logN, Z != nullptr);
    const dim3 cols((g.N2 + kCols - 1) / kCols, B);
    if (Z) {
        // cleared by a kernel, like every flag array of this library: a captured call replays it as a kernel node
        const int rc = fsn_launch_zero_words(reinterpret_cast<unsigned*>(live), (size_t)B, s);
        if (rc != FSN_OK) return rc;
        hipLaunchKernelGGL(conv_cols_fwd_kernel, cols, dim3(kThreads), 0, s, x, h_slab, fmt, taps, static_cast<cd*>(Z), live, g);
        FSN_TRY_LAUNCH("conv_cols_fwd_kernel");
        hipLaunchKernelGGL(conv_rows_kernel, dim3(g.N1 / 2 + 1, B), dim3(kThreads), 0, s, taps, static_cast<cd*>(Z), g);
        FSN_TRY_LAUNCH("conv_rows_kernel");
    }
    hipLaunchKernelGGL(conv_cols_inv_kernel, cols, dim3(kThreads), 0, s, x, taps, static_cast<const cd*>(Z), live, y, g);
    return fsn_check_launch("conv_cols_inv_kernel");
}

int fsn_launch_mix_gather(const void* clean_slab, const void* noise_slab, int fmt, const fsn_mix_item* items,
                          const fsn_mix_seg* segs, int n_segs, int B, int L, float* c0, float* nz, hipStream_t s) {
    hipLaunchKernelGGL(mix_gather_kernel, dim3((L + kThreads - 1) / kThreads, B, 2), dim3(kThreads), 0, s, clean_slab,
                       noise_slab, fmt, items, segs, n_segs, L, c0, nz);
    return fsn_check_launch("mix_gather_kernel");
}

int fsn_launch_mix_level(const float* c, const float* nz, const fsn_mix_item* items, int B, int L, float eps, float* noisy,
                         float* clean, hipStream_t s) {
    hipLaunchKernelGGL(mix_level_kernel<false>, dim3(B), dim3(kLevelThreads), 0, s, c, nz, items, L, (double)eps, noisy, clean,
                       static_cast<const float*>(nullptr), static_cast<const int*>(nullptr), static_cast<float*>(nullptr));
    return fsn_check_launch("mix_level_kernel");
}

int fsn_launch_mix_level_target(const float* c, const float* nz, const float* c2, const int* t_len, const fsn_mix_item* items,
                                int B, int L, float eps, float* noisy, float* clean, float* target, hipStream_t s) {
    hipLaunchKernelGGL(mix_level_kernel<true>, dim3(B), dim3(kLevelThreads), 0, s, c, nz, items, L, (double)eps, noisy, clean,
                       c2, t_len, target);
    return fsn_check_launch("mix_level_kernel<target>");
}

int fsn_launch_rir_shorten(const void* h_slab, int fmt, const void* h_off, int off_stride, const void* h_len, int len_stride,
                           int B, const fsn_mix_target* targets, float* out, int ld, float* win, int* idx, long* t_off,
                           int* t_len, hipStream_t s) {
    const Taps taps{static_cast<const char*>(h_off), static_cast<const char*>(h_len), off_stride, len_stride};
    hipLaunchKernelGGL(rir_shorten_kernel, dim3(B), dim3(kShortenThreads), 0, s, h_slab, fmt, taps, targets, out, ld, win, idx,
                       t_off, t_len);
    return fsn_check_launch("rir_shorten_kernel");
}
