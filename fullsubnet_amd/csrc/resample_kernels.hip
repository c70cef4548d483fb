// Sample-rate conversion on the device (fsn_resample / fsn_resample_taps, include/fsn_hip.h): a rational-ratio polyphase
// FIR resampler for ragged batches, scipy.signal.resample_poly's construction generalised by (zeros, beta, rolloff).
// DESIGN 9c pins the arithmetic.
//
//   resample_taps_kernel  h[t] = u g[t] / sum(g), g = kaiser(2H + 1, beta) fc sinc(fc t), fp64 (I0 as a series, sinpi),
//                         one fixed-order sum; natural order [2H + 1] and polyphase order [u][Js]     -> h, poly
//   resample_kernel       y[k] = fp32(sum_m h[k d + H - m u] x[m]): a workgroup takes `tile` consecutive outputs of a row,
//                         stages the stretch of the row under them in LDS (zeros outside the row) and - when it fits beside
//                         that - the whole polyphase table; a thread produces eight outputs k, k + S, .. of ONE phase
//                         (S a multiple of u, about 1024), so a tap is loaded once per eight multiply-adds                -> y
//   resample_copy_kernel  u == d == 1: the row bit for bit
//
// Output k of a row has phase p = (k d + H) mod u and newest input q = (k d + H) / u; its taps are row p of the table,
// poly[p][j] = h[p + j u] (zero past 2H), against x[q - j], j = 0 .. J - 1 in that order: the order depends on (u, d,
// design, k) alone and the zero taps and the zeros staged outside [0, n) add exact zeros, so a row has the same bits alone,
// in any batch and in any tile.  Sums are fp64 fma chains, one rounding to fp32 at the store.  Every product of a sample
// position with u or d is 64-bit.  No atomics, no flags, nothing handed from one workgroup to another.
#include "fsn_common.h"

namespace {

constexpr int kThreads = kFsnResampleThreads;
constexpr int kR = kFsnResampleOutPerThread;
constexpr int kTapThreads = 1024;

constexpr int kI0Terms = 512;

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^2k / (k!)^2), all terms positive; inv_k2[k] = 1 / k^2
__device__ __forceinline__ double bessel_i0(double x, const double* inv_k2) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < kI0Terms; ++k) {
        term *= q * inv_k2[k];
        sum += term;
        if (term < 1e-19 * sum) break;
    }
    return sum;
}

// one workgroup.  h: [taps]; poly: [u][Js] or NULL
__global__ __launch_bounds__(kTapThreads) void resample_taps_kernel(FsnResamplePlan p, double* __restrict__ h,
                                                                    double* __restrict__ poly) {
    __shared__ double scratch[kTapThreads / 64];
    __shared__ double inv_k2[kI0Terms];
    if (threadIdx.x >= 1 && threadIdx.x < kI0Terms) inv_k2[threadIdx.x] = 1.0 / ((double)threadIdx.x * (double)threadIdx.x);
    __syncthreads();
    const int P = p.u > p.d ? p.u : p.d;
    const double fc = p.rolloff / (double)P;
    const double i0_beta = bessel_i0(p.beta, inv_k2);
    double part = 0.0;
    for (int i = threadIdx.x; i < p.taps; i += kTapThreads) {
        const int t = i - p.H;
        const double r = (double)t / (double)p.H;
        const double rad = 1.0 - r * r;
        const double win = bessel_i0(p.beta * sqrt(rad > 0.0 ? rad : 0.0), inv_k2) / i0_beta;
        const double v = fc * (double)t;
        const double sinc = t == 0 ? 1.0 : sinpi(v) / (M_PI * v);
        const double g = win * fc * sinc;
        h[i] = g;
        part += g;
    }
    const double sum = fsn_block_sum(part, scratch);
    for (int i = threadIdx.x; i < p.taps; i += kTapThreads) {  // each thread its own entries
        const double hv = (double)p.u * h[i] / sum;
        h[i] = hv;
        if (poly) poly[(long)(i % p.u) * p.Js + i / p.u] = hv;
    }
    if (!poly) return;
    for (int i = p.taps + threadIdx.x; i < p.u * p.J; i += kTapThreads) poly[(long)(i % p.u) * p.Js + i / p.u] = 0.0;
    if (p.Js > p.J)
        for (int q = threadIdx.x; q < p.u; q += kTapThreads) poly[(long)q * p.Js + p.J] = 0.0;
}

__device__ __forceinline__ int row_samples(const int* lengths, int b, int L_max) {
    if (!lengths) return L_max;
    const int l = lengths[b];
    return l < 0 ? 0 : (l > L_max ? L_max : l);
}

// grid (ceil(L_out_max / tile), B).  Dynamic LDS: [u][Js] doubles when TAPS_LDS, then p.stretch floats.
template <bool TAPS_LDS>
__global__ __launch_bounds__(kThreads) void resample_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                            int L_max, FsnResamplePlan p, const double* __restrict__ poly,
                                                            float* __restrict__ y, int L_out_max,
                                                            int* __restrict__ out_lengths) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    float* xs = reinterpret_cast<float*>(lds + (TAPS_LDS ? (size_t)p.u * p.Js : 0));
    const int b = blockIdx.y;
    const int n = row_samples(lengths, b, L_max);
    long n_out = fsn_resample_n_out(n, p.u, p.d);
    n_out = n_out > L_out_max ? L_out_max : n_out;
    if (blockIdx.x == 0 && threadIdx.x == 0 && out_lengths) out_lengths[b] = (int)n_out;
    const long K0 = (long)blockIdx.x * p.tile;
    float* yr = y + (long)b * L_out_max;
    if (K0 >= n_out) {  // the whole tile lies behind the row: zeros
        const long end = K0 + p.tile < L_out_max ? K0 + p.tile : L_out_max;
        for (long k = K0 + threadIdx.x; k < end; k += kThreads) yr[k] = 0.f;
        return;
    }
    // inputs m_a .. m_b: from the oldest sample under the tile's first output to the newest under its last
    const float* xr = x + (long)b * L_max;
    const long m_a = (K0 * p.d + p.H) / p.u - (p.J - 1);
    const long m_b = ((K0 + p.tile - 1) * p.d + p.H) / p.u;
    const int count = (int)(m_b - m_a + 1);  // <= p.stretch
    for (int i = threadIdx.x; i < count; i += kThreads) {
        const long m = m_a + i;
        xs[i] = (m >= 0 && m < n) ? xr[m] : 0.f;
    }
    if (TAPS_LDS)
        for (int i = threadIdx.x; i < p.u * p.Js; i += kThreads) lds[i] = poly[i];
    __syncthreads();
    const double* table = TAPS_LDS ? lds : poly;
    const int step = (p.S / p.u) * p.d;  // inputs between two outputs of a thread
    for (int t = threadIdx.x; t < p.S; t += kThreads) {
        const long k = K0 + t;
        const long c = k * p.d + p.H;
        const long q = c / p.u;
        const int phase = (int)(c - q * p.u);
        const double* row = table + (long)phase * p.Js;
        const float* xq = xs + (int)(q - m_a);  // x[q]; x[q - j] exists in LDS down to j = J - 1
        double acc[kR];
#pragma unroll
        for (int r = 0; r < kR; ++r) acc[r] = 0.0;
        for (int j = 0; j < p.J; ++j) {
            const double hv = row[j];
#pragma unroll
            for (int r = 0; r < kR; ++r) acc[r] = fma(hv, (double)xq[r * step - j], acc[r]);
        }
#pragma unroll
        for (int r = 0; r < kR; ++r) {
            const long kr = k + (long)r * p.S;
            if (kr < n_out) yr[kr] = (float)acc[r];
            else if (kr < L_out_max) yr[kr] = 0.f;
        }
    }
}

// grid (ceil(L_out_max / (4 kThreads)), B)
__global__ __launch_bounds__(kThreads) void resample_copy_kernel(const float* __restrict__ x, const int* __restrict__ lengths,
                                                                 int L_max, float* __restrict__ y, int L_out_max,
                                                                 int* __restrict__ out_lengths) {
    const int b = blockIdx.y;
    int n = row_samples(lengths, b, L_max);
    n = n > L_out_max ? L_out_max : n;
    if (blockIdx.x == 0 && threadIdx.x == 0 && out_lengths) out_lengths[b] = n;
    const float* xr = x + (long)b * L_max;
    float* yr = y + (long)b * L_out_max;
    const long k0 = (long)blockIdx.x * (4 * kThreads) + threadIdx.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long k = k0 + (long)e * kThreads;
        if (k < L_out_max) yr[k] = k < n ? xr[k] : 0.f;
    }
}

}  // namespace

int fsn_launch_resample_taps(const FsnResamplePlan& p, double* h, double* poly, hipStream_t s) {
    hipLaunchKernelGGL(resample_taps_kernel, dim3(1), dim3(kTapThreads), 0, s, p, h, poly);
    return fsn_check_launch("resample_taps_kernel");
}

int fsn_launch_resample(const float* x, const int* lengths, int B, int L_max, const FsnResamplePlan& p, const double* poly,
                        float* y, int L_out_max, int* out_lengths, hipStream_t s) {
    if (p.u == 1 && p.d == 1) {
        hipLaunchKernelGGL(resample_copy_kernel, dim3((L_out_max + 4 * kThreads - 1) / (4 * kThreads), B), dim3(kThreads), 0, s, x,
                           lengths, L_max, y, L_out_max, out_lengths);
        return fsn_check_launch("resample_copy_kernel");
    }
    const size_t table = p.taps_in_lds ? (size_t)p.u * p.Js * sizeof(double) : 0;
    const size_t lds = table + (size_t)p.stretch * sizeof(float);
    if (lds > kFsnResampleLdsBytes) {
        fsn_set_error("fsn_launch_resample: %zu bytes of LDS, a workgroup holds %zu", lds, kFsnResampleLdsBytes);
        return FSN_ERR_ARG;
    }
    const dim3 grid((L_out_max + p.tile - 1) / p.tile, B);
    if (p.taps_in_lds) {
        FSN_TRY_RESERVE_LDS("resample_kernel", resample_kernel<true>, lds);
        hipLaunchKernelGGL(resample_kernel<true>, grid, dim3(kThreads), lds, s, x, lengths, L_max, p, poly, y, L_out_max,
                           out_lengths);
    } else {
        FSN_TRY_RESERVE_LDS("resample_kernel", resample_kernel<false>, lds);
        hipLaunchKernelGGL(resample_kernel<false>, grid, dim3(kThreads), lds, s, x, lengths, L_max, p, poly, y, L_out_max,
                           out_lengths);
    }
    return fsn_check_launch("resample_kernel");
}
