// STFT / iSTFT for transform sizes and hops other than the FullSubNet recipe's 512 / 256
// (audio_zen/acoustics/feature.py:9-91 with other TOML values; improved_fullsubnet/model.py:550-557,
// 582-589 uses 512 / 128 at 16 kHz and 960 / 480 at 48 kHz).  The transform is < 0.1 % of the path's
// work, so the general case is a direct O(N^2) DFT in fp64 from an exact twiddle table in LDS: any even
// N, no radix restrictions, and - like the radix-8 fast path - the result is the correctly rounded
// transform of the fp32 windowed frame (N fp64 rounding errors of 2^-53 each before the final
// rounding to fp32).  ~1.3 GFLOP fp64 per 1000 frames at N = 960: microseconds next to the LSTMs.
#include "fsn_common.h"

namespace {

__device__ __forceinline__ void fill_twiddles(double* c, double* s, int N) {
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        double sv, cv;
        sincospi(2.0 * (double)n / (double)N, &sv, &cv);
        c[n] = cv;
        s[n] = sv;
    }
}

// Ragged batches (kRagged; fsn_stft_ragged_generic, fsn_istft_ragged): lengths [B] holds row b's sample count L_b, the
// row stride stays L (the longest row) and T is the longest row's frame count.  Row b is the transform of its own
// L_b samples - reflected at its own end - in its first T_b = 1 + L_b / hop frames; a frame past T_b is a zero store
// (forward) or is skipped (inverse: the overlap-add never reads it).  Values are clamped to [N / 2 + 1, L], so no index
// leaves the row whatever the array holds.  With L_b = L the index arithmetic, and so every bit, is the rectangular one.
__device__ __forceinline__ int row_samples(const int* lengths, int b, int L, int N) {
    const int l = lengths[b];
    return l < N / 2 + 1 ? N / 2 + 1 : (l > L ? L : l);
}
__device__ __forceinline__ int row_frames(const int* lengths, int b, int L, int N, int hop, int T) {
    const int t = 1 + row_samples(lengths, b, L, N) / hop;
    return t < T ? t : T;
}

// grid (B * T, ceil(F / 256)); re / im / mag [B][F][T] (any may be NULL)
template <bool kRagged>
__global__ __launch_bounds__(256) void dft_stft_kernel(const float* __restrict__ y, const float* __restrict__ window,
                                                       float* __restrict__ re, float* __restrict__ im,
                                                       float* __restrict__ mag, int L, int T, int N, int hop, int F,
                                                       const int* __restrict__ lengths) {
    extern __shared__ double sh[];
    double *x = sh, *c = sh + N, *s = sh + 2 * N;
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    const int Lb = kRagged ? row_samples(lengths, b, L, N) : L;
    if (kRagged && t >= 1 + Lb / hop) {  // past the row's end (the whole workgroup: b and t are its own)
        const int f = blockIdx.y * blockDim.x + threadIdx.x;
        if (f < F) {
            const long o = ((long)b * F + f) * T + t;
            if (re) re[o] = 0.f;
            if (im) im[o] = 0.f;
            if (mag) mag[o] = 0.f;
        }
        return;
    }
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        int j = hop * t + n - N / 2;  // centre padding, reflect without repeating the edge
        j = j < 0 ? -j : j;
        j = j >= Lb ? 2 * (Lb - 1) - j : j;
        x[n] = (double)(y[(long)b * L + j] * window[n]);  // the frame is rounded to fp32 like ATen's
    }
    fill_twiddles(c, s, N);
    __syncthreads();
    const int f = blockIdx.y * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double ar = 0.0, ai = 0.0;
    int idx = 0;
    for (int n = 0; n < N; ++n) {
        const double xv = x[n];
        ar = fma(xv, c[idx], ar);
        ai = fma(-xv, s[idx], ai);
        idx += f;
        idx = idx >= N ? idx - N : idx;
    }
    const float fr = (float)ar, fi = (float)ai;
    const long o = ((long)b * F + f) * T + t;
    if (re) re[o] = fr;
    if (im) im[o] = fi;
    if (mag) mag[o] = (float)sqrt((double)fr * fr + (double)fi * fi);
}

// grid (B * T, ceil(N / 256)); re / im [B][F][T] -> windowed time frames wframes [B][T][N]
template <bool kRagged>
__global__ __launch_bounds__(256) void dft_irfft_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                        const float* __restrict__ window, float* __restrict__ wframes,
                                                        int T, int N, int F, const int* __restrict__ lengths, int L, int hop) {
    extern __shared__ double sh[];
    double *xr = sh, *xi = sh + F, *c = sh + 2 * F, *s = sh + 2 * F + N;
    const int b = blockIdx.x / T, t = blockIdx.x % T;
    if (kRagged && t >= row_frames(lengths, b, L, N, hop, T)) return;  // neither read nor written: the overlap-add stops at T_b
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        const long o = ((long)b * F + f) * T + t;
        const bool edge = f == 0 || f == N / 2;  // C2R: imaginary parts of DC / Nyquist are ignored
        const double k = edge ? 1.0 : 2.0;
        xr[f] = k * (double)re[o];
        xi[f] = edge ? 0.0 : k * (double)im[o];
    }
    fill_twiddles(c, s, N);
    __syncthreads();
    const int n = blockIdx.y * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double acc = 0.0;
    int idx = 0;
    for (int f = 0; f < F; ++f) {
        acc = fma(xr[f], c[idx], acc);
        acc = fma(-xi[f], s[idx], acc);
        idx += n;
        idx = idx >= N ? idx - N : idx;
    }
    const float v = (float)(acc / (double)N);
    wframes[((long)b * T + t) * N + n] = v * window[n];
}

// ---- two-level form: N = P Q -------------------------------------------------------------------------------------
// The direct transform above costs N^2 / 2 multiply-adds per frame and rebuilds its twiddle table (N sincospi in fp64)
// in every workgroup: 10.8 % of Improved FullSubNet's step at 48 kHz (960 / 480; profiles/r02_kernel_stats_improved48_b32.md).
// Any composite N splits once, Cooley-Tukey style, into Q transforms of length P and P of length Q, each still direct,
// still fp64, still from the exact N-entry table (W_P^a = W_N^{Q a}, W_Q^b = W_N^{P b}): N (P + Q) instead of N^2 -
// 62 N at 960 = 30 x 32 - and a workgroup builds the table ONCE and walks over many frames.  No radix-specific code:
// 400 = 20 x 20, 512 = 16 x 32, 960 = 30 x 32, 1536 = 32 x 48 all take this path.
//   forward, n = Q n1 + n2, k = k1 + P k2:
//     Bt[n2][k1] = W_N^{n2 k1} sum_{n1} x[Q n1 + n2] W_N^{Q n1 k1}         (x real: 2 fma per term)
//     X[k1 + P k2] = sum_{n2} Bt[n2][k1] W_N^{P n2 k2}                       (k <= N / 2 only)
//   inverse (C2R), the same index split with conjugate twiddles:
//     Ct[n2][k1] = conj(W_N^{n2 k1}) sum_{k2} X[k1 + P k2] conj(W_N^{P n2 k2}), X completed by Hermitian symmetry
//     x[Q n1 + n2] = Re sum_{k1} Ct[n2][k1] conj(W_N^{Q n1 k1})              (2 fma per term)
// LDS: table 2 N + frame N (2 N complex for the inverse) + intermediate 2 N doubles: 38 / 46 KB at N = 960.
template <bool kRagged>
__global__ __launch_bounds__(256) void dft2_stft_kernel(const float* __restrict__ y, const float* __restrict__ window,
                                                        float* __restrict__ re, float* __restrict__ im,
                                                        float* __restrict__ mag, int L, int T, int N, int hop, int F, int P,
                                                        int Q, long frames, const int* __restrict__ lengths) {
    extern __shared__ double sh[];
    double *c = sh, *s = sh + N, *x = sh + 2 * N, *br = sh + 3 * N, *bi = sh + 4 * N;
    fill_twiddles(c, s, N);
    for (long fr = blockIdx.x; fr < frames; fr += gridDim.x) {
        const int b = (int)(fr / T), t = (int)(fr % T);
        __syncthreads();  // table ready / previous frame's stage 2 done with x and Bt
        const int Lb = kRagged ? row_samples(lengths, b, L, N) : L;
        if (kRagged && t >= 1 + Lb / hop) {  // past the row's end: a zero store (every thread takes this branch)
            for (int k = threadIdx.x; k < F; k += blockDim.x) {
                const long o = ((long)b * F + k) * T + t;
                if (re) re[o] = 0.f;
                if (im) im[o] = 0.f;
                if (mag) mag[o] = 0.f;
            }
            continue;
        }
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            int j = hop * t + n - N / 2;  // centre padding, reflect without repeating the edge
            j = j < 0 ? -j : j;
            j = j >= Lb ? 2 * (Lb - 1) - j : j;
            x[n] = (double)(y[(long)b * L + j] * window[n]);  // the frame is rounded to fp32 like ATen's
        }
        __syncthreads();
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const int k1 = i / Q, n2 = i - k1 * Q;
            double ar = 0.0, ai = 0.0;
            int idx = 0;
            const int step = (int)(((long)Q * k1) % N);
            for (int n1 = 0; n1 < P; ++n1) {
                const double xv = x[Q * n1 + n2];
                ar = fma(xv, c[idx], ar);
                ai = fma(-xv, s[idx], ai);
                idx += step;
                idx = idx >= N ? idx - N : idx;
            }
            const int tw = (int)(((long)n2 * k1) % N);
            const double wr = c[tw], wi = -s[tw];
            br[n2 * P + k1] = ar * wr - ai * wi;
            bi[n2 * P + k1] = ar * wi + ai * wr;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < F; k += blockDim.x) {
            const int k2 = k / P, k1 = k - k2 * P;
            double ar = 0.0, ai = 0.0;
            int idx = 0;
            const int step = (int)(((long)P * k2) % N);
            for (int n2 = 0; n2 < Q; ++n2) {
                const double vr = br[n2 * P + k1], vi = bi[n2 * P + k1], wr = c[idx], wi = -s[idx];
                ar = fma(vr, wr, ar);
                ar = fma(-vi, wi, ar);
                ai = fma(vr, wi, ai);
                ai = fma(vi, wr, ai);
                idx += step;
                idx = idx >= N ? idx - N : idx;
            }
            const float fr32 = (float)ar, fi32 = (float)ai;
            const long o = ((long)b * F + k) * T + t;
            if (re) re[o] = fr32;
            if (im) im[o] = fi32;
            if (mag) mag[o] = (float)sqrt((double)fr32 * fr32 + (double)fi32 * fi32);
        }
    }
}

template <bool kRagged>
__global__ __launch_bounds__(256) void dft2_irfft_kernel(const float* __restrict__ re, const float* __restrict__ im,
                                                         const float* __restrict__ window, float* __restrict__ wframes,
                                                         int T, int N, int F, int P, int Q, long frames,
                                                         const int* __restrict__ lengths, int L, int hop) {
    extern __shared__ double sh[];
    double *c = sh, *s = sh + N, *xr = sh + 2 * N, *xi = sh + 3 * N, *cr = sh + 4 * N, *ci = sh + 5 * N;
    fill_twiddles(c, s, N);
    for (long fr = blockIdx.x; fr < frames; fr += gridDim.x) {
        const int b = (int)(fr / T), t = (int)(fr % T);
        __syncthreads();
        if (kRagged && t >= row_frames(lengths, b, L, N, hop, T)) continue;  // neither read nor written (every thread)
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            const long o = ((long)b * F + f) * T + t;
            const bool edge = f == 0 || f == N / 2;  // C2R: imaginary parts of DC / Nyquist are ignored
            const double vr = (double)re[o], vi = edge ? 0.0 : (double)im[o];
            xr[f] = vr;
            xi[f] = vi;
            if (!edge) {  // X[N - f] = conj(X[f])
                xr[N - f] = vr;
                xi[N - f] = -vi;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const int k1 = i / Q, n2 = i - k1 * Q;
            double ar = 0.0, ai = 0.0;
            int idx = 0;
            const int step = (int)(((long)P * n2) % N);
            for (int k2 = 0; k2 < Q; ++k2) {
                const double vr = xr[k1 + P * k2], vi = xi[k1 + P * k2], wr = c[idx], wi = s[idx];  // conj(W) = c + i s
                ar = fma(vr, wr, ar);
                ar = fma(-vi, wi, ar);
                ai = fma(vr, wi, ai);
                ai = fma(vi, wr, ai);
                idx += step;
                idx = idx >= N ? idx - N : idx;
            }
            const int tw = (int)(((long)n2 * k1) % N);
            const double wr = c[tw], wi = s[tw];
            cr[n2 * P + k1] = ar * wr - ai * wi;
            ci[n2 * P + k1] = ar * wi + ai * wr;
        }
        __syncthreads();
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            const int n1 = n / Q, n2 = n - n1 * Q;
            double acc = 0.0;
            int idx = 0;
            const int step = (int)(((long)Q * n1) % N);
            for (int k1 = 0; k1 < P; ++k1) {
                acc = fma(cr[n2 * P + k1], c[idx], acc);  // Re (Ct conj(W))
                acc = fma(-ci[n2 * P + k1], s[idx], acc);
                idx += step;
                idx = idx >= N ? idx - N : idx;
            }
            const float v = (float)(acc / (double)N);
            wframes[((long)b * T + t) * N + n] = v * window[n];
        }
    }
}

// the split with P <= Q, both > 3, P as large as possible; 0: N is (twice) a prime or too large for the LDS: direct form
int dft2_factor(int N) {
    if (N > 2048) return 0;
    int best = 0;
    for (int p = 4; (long)p * p <= N; ++p)
        if (N % p == 0) best = p;
    return best;
}

// overlap-add (ascending frame order, fp32), division by the overlap-added squared window, centre
// trim and length handling of torch.istft.  kRagged: row b over its own Tb frames (the frame stride stays T) at its own
// length, zeros from there on
template <bool kRagged>
__global__ __launch_bounds__(256) void ola_generic_kernel(const float* __restrict__ wframes,
                                                          const float* __restrict__ window, float* __restrict__ y,
                                                          int B, int T, int N, int hop, int length,
                                                          const int* __restrict__ lengths) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)B * length) return;
    const int b = (int)(gid / length), j = (int)(gid % length);
    const int Lb = kRagged ? row_samples(lengths, b, length, N) : length;
    const int Tb = kRagged ? row_frames(lengths, b, length, N, hop, T) : T;
    const int p = j + N / 2;
    const long total = (long)N + (long)hop * (Tb - 1);
    float out = 0.f;
    if (p < total && j < Lb) {
        int t0 = p - N + 1;
        t0 = t0 <= 0 ? 0 : (t0 + hop - 1) / hop;
        int t1 = p / hop;
        t1 = t1 < Tb ? t1 : Tb - 1;
        float acc = 0.f, env = 0.f;
        for (int t = t0; t <= t1; ++t) {
            const int n = p - hop * t;
            const float w = window[n];
            acc = acc + wframes[((long)b * T + t) * N + n];
            env = env + w * w;
        }
        out = acc / env;
    }
    y[gid] = out;
}

}  // namespace

// Every instantiation is a kernel symbol of its own: the dynamic-LDS limit above 64 KB is raised on the one launched.
template <bool kRagged>
static int launch_dft_stft(const float* y, int B, int L, const float* window, float* re, float* im, float* mag, int T, int N,
                           int hop, const int* lengths, hipStream_t s) {
    const int F = N / 2 + 1;
    if (const int P = dft2_factor(N)) {
        const long frames = (long)B * T;
        const unsigned grid = (unsigned)(frames < 1024 ? frames : 1024);
        if (5 * N * sizeof(double) > 64 * 1024)
            (void)fsn_request_lds(dft2_stft_kernel<kRagged>, 5 * N * sizeof(double));
        hipLaunchKernelGGL(dft2_stft_kernel<kRagged>, dim3(grid), dim3(256), 5 * N * sizeof(double), s, y, window, re, im, mag,
                           L, T, N, hop, F, P, N / P, frames, lengths);
        return fsn_check_launch("dft2_stft_kernel");
    }
    const size_t lds = 3 * N * sizeof(double);  // 96 KB at N = 4096: above 64 KB a launch needs the attribute raised
    if (lds > 64 * 1024)
        (void)fsn_request_lds(dft_stft_kernel<kRagged>, lds);
    hipLaunchKernelGGL(dft_stft_kernel<kRagged>, dim3((unsigned)(B * T), (F + 255) / 256), dim3(256), lds, s, y, window, re, im,
                       mag, L, T, N, hop, F, lengths);
    return fsn_check_launch("dft_stft_kernel");
}

// lengths != NULL: the ragged batch (length is then the row stride L_max of the waveforms)
template <bool kRagged>
static int launch_dft_istft(const float* re, const float* im, const float* window, float* wframes, float* y, int B, int T,
                            int N, int hop, int length, const int* lengths, hipStream_t s) {
    const int F = N / 2 + 1;
    if (const int P = dft2_factor(N)) {
        const long frames = (long)B * T;
        const unsigned grid = (unsigned)(frames < 1024 ? frames : 1024);
        if (6 * N * sizeof(double) > 64 * 1024)
            (void)fsn_request_lds(dft2_irfft_kernel<kRagged>, 6 * N * sizeof(double));
        hipLaunchKernelGGL(dft2_irfft_kernel<kRagged>, dim3(grid), dim3(256), 6 * N * sizeof(double), s, re, im, window, wframes,
                           T, N, F, P, N / P, frames, lengths, length, hop);
        FSN_TRY_LAUNCH("dft2_irfft_kernel");
    } else {
        const size_t lds = (2 * F + 2 * N) * sizeof(double);
        if (lds > 64 * 1024)
            (void)fsn_request_lds(dft_irfft_kernel<kRagged>, lds);
        hipLaunchKernelGGL(dft_irfft_kernel<kRagged>, dim3((unsigned)(B * T), (N + 255) / 256), dim3(256), lds, s, re, im, window,
                           wframes, T, N, F, lengths, length, hop);
        FSN_TRY_LAUNCH("dft_irfft_kernel");
    }
    const long n = (long)B * length;
    hipLaunchKernelGGL(ola_generic_kernel<kRagged>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, wframes, window, y, B, T,
                       N, hop, length, lengths);
    return fsn_check_launch("ola_generic_kernel");
}

int fsn_launch_dft_stft(const float* y, int B, int L, const float* window, float* re, float* im, float* mag, int T,
                        int N, int hop, hipStream_t s, const int* lengths) {
    return lengths ? launch_dft_stft<true>(y, B, L, window, re, im, mag, T, N, hop, lengths, s)
                   : launch_dft_stft<false>(y, B, L, window, re, im, mag, T, N, hop, nullptr, s);
}

int fsn_launch_dft_istft(const float* re, const float* im, const float* window, float* wframes, float* y, int B, int T,
                         int N, int hop, int length, hipStream_t s, const int* lengths) {
    return lengths ? launch_dft_istft<true>(re, im, window, wframes, y, B, T, N, hop, length, lengths, s)
                   : launch_dft_istft<false>(re, im, window, wframes, y, B, T, N, hop, length, nullptr, s);
}
