// Validation metrics on the device (fsn_stoi / fsn_si_sdr, include/fsn_hip.h): the short-time objective intelligibility
// measure of Taal, Hendriks, Heusdens and Jensen (2011) as audio_zen/metrics.py:34 asks for it (not extended), and the
// SI-SDR of metrics.py:19-31, for ragged batches of clean / estimate pairs.  DESIGN 9b pins every constant.
//
//   stoi_taps_kernel      Kaiser-windowed sinc of the resampler (I0 as a series), normalised to unit sum     -> taps
//   stoi_resample_kernel  polyphase resampling to 10 kHz of both signals of every row                  x, y  -> rs
//   stoi_energy_kernel    energies of the clean row's 256-sample frames, hop 128, in dB                rs    -> energy
//   stoi_keep_kernel      per row: the loudest frame, the frames within 40 dB of it, in order          energy -> kept, n_kept
//   stoi_band_kernel      a frame of the silence-free signals (overlap-added from the kept frames as it is read), window,
//                         ONE 512-point transform for clean + i estimate, Hermitian split, 15 band sums      -> tob
//   stoi_corr_kernel      one thread per (segment of 30 frames, band): scale, clip, centre, normalise, correlate;
//                         one partial sum per workgroup, in a fixed order                                     -> partial
//   stoi_finish_kernel    the partial sums of a row in a fixed order, d = sum / (15 J) or 1e-5 for a short row -> d
//   si_sdr_kernel         one workgroup per row: <r, e>, <r, r>, then |a r|^2 and |e - a r|^2 in a second pass
//
// Everything is fp64 and every per-row count follows from the row's own length, so a row's bits do not depend on the
// batch it is scored in; there are no atomics and no flags, and nothing is read before a kernel of the same call wrote it.
#include "fsn_common.h"

namespace {

#include "fft64_lds.h"  // cd, bitrev, fill_twiddles, lds_fft

constexpr int kThreads = kFftThreads;
constexpr int kFrame = 256, kHop = 128, kNfft = 512, kLogNfft = 9;
constexpr int kBands = 15, kSeg = 30;
constexpr int kMaxTaps = 1741;                 // 48 kHz: 2 x 870 + 1
constexpr int kResampleIn = 1576;              // input samples under 256 outputs: (255 down + 2 half) / up + 2 at 48 kHz = 1574
constexpr int kFramesPerGroup = 4;             // transforms per workgroup of the band kernel: 32 KB of LDS
constexpr double kEps = 2.220446049250313e-16;  // 2^-52
constexpr int kSdrThreads = 1024;

struct Row {
    int n, n10, nf;  // samples, samples at 10 kHz, frames of 256 at hop 128 with start < n10 - 256
};
__device__ __forceinline__ Row row_of(const int* lengths, int b, const FsnStoiPlan& p) {
    Row r;
    r.n = fsn_stoi_row_samples(lengths, b, p.L_max);
    r.n10 = fsn_stoi_n10(r.n, p.up, p.down, p.half);
    r.nf = fsn_stoi_frames(r.n10);
    return r;
}

// hanning(258)[1:-1]
__device__ __forceinline__ double stoi_window(int s) { return 0.5 - 0.5 * cospi(2.0 * (double)(s + 1) / 257.0); }

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^2k / (k!)^2), all terms positive
__device__ __forceinline__ double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-19 * sum) break;
    }
    return sum;
}

// one workgroup: h[t] = kaiser(2 half + 1, beta)[t] 2 up fc sinc(2 fc t), t = -half .. half, then h / sum(h)
__global__ __launch_bounds__(1024) void stoi_taps_kernel(double* __restrict__ taps, int up, int down, int half) {
    __shared__ double scratch[16];
    const int n = 2 * half + 1;
    const int P = up > down ? up : down;
    const double beta = 0.1102 * (60.0 - 8.7);
    const double i0_beta = bessel_i0(beta);
    const double fc = 1.0 / (2.0 * (double)P);
    double part = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const int t = i - half;
        const double u = (double)t / (double)half;
        const double rad = 1.0 - u * u;
        const double win = bessel_i0(beta * sqrt(rad > 0.0 ? rad : 0.0)) / i0_beta;
        const double x = (double)t / (double)P;  // 2 fc t
        const double sinc = t == 0 ? 1.0 : sinpi(x) / (M_PI * x);
        const double h = win * (2.0 * (double)up * fc) * sinc;
        taps[i] = h;
        part += h;
    }
    const double sum = fsn_block_sum(part, scratch);
    for (int i = threadIdx.x; i < n; i += 1024) taps[i] = taps[i] / sum;  // each thread its own entries
}

// grid (ceil(n10_max / 256), B): output sample k of both signals,
// up * sum_m taps[k down + half - m up] x[m] over the m inside the row whose tap exists.  The taps and the stretch of
// both input rows that the workgroup's 256 outputs touch sit in LDS (fp64, clean and estimate side by side).
__global__ __launch_bounds__(kThreads) void stoi_resample_kernel(const float* __restrict__ clean,
                                                                 const float* __restrict__ estimate,
                                                                 const int* __restrict__ lengths,
                                                                 const double* __restrict__ taps, FsnStoiPlan p,
                                                                 double* __restrict__ rs) {
    __shared__ double h[kMaxTaps];
    __shared__ cd in[kResampleIn];
    const int b = blockIdx.y;
    const Row row = row_of(lengths, b, p);
    const int k0 = blockIdx.x * kThreads;
    if (k0 >= row.n10) return;
    const int k = k0 + threadIdx.x;
    const float* xr = clean + (long)b * p.L_max;
    const float* yr = estimate + (long)b * p.L_max;
    double* ox = rs + (long)b * 2 * p.n10_max + k;
    double* oy = ox + p.n10_max;
    if (!p.half) {
        if (k < row.n10) {
            *ox = (double)xr[k];
            *oy = (double)yr[k];
        }
        return;
    }
    // inputs m_a .. m_b: from the first tap of output k0 to the last tap of the workgroup's last output, inside the row
    // (m_a <= n - 1 because k0 down < n up and half >= up; at most (255 down + 2 half) / up + 2 <= kResampleIn of them)
    const long lo0 = (long)k0 * p.down - p.half;
    const int m_a = lo0 <= 0 ? 0 : (int)((lo0 + p.up - 1) / p.up);
    const int k_last = k0 + kThreads - 1 < row.n10 - 1 ? k0 + kThreads - 1 : row.n10 - 1;
    int m_b = (int)(((long)k_last * p.down + p.half) / p.up);
    m_b = m_b > row.n - 1 ? row.n - 1 : m_b;
    for (int i = threadIdx.x; i < 2 * p.half + 1; i += kThreads) h[i] = taps[i];
    for (int i = threadIdx.x; i <= m_b - m_a; i += kThreads) in[i] = cd{(double)xr[m_a + i], (double)yr[m_a + i]};
    __syncthreads();
    if (k >= row.n10) return;
    const long c = (long)k * p.down;
    const long lo = c - p.half;
    const int m_lo = lo <= 0 ? 0 : (int)((lo + p.up - 1) / p.up);  // >= m_a
    int m_hi = (int)((c + p.half) / p.up);                          // <= m_b after the clamp
    m_hi = m_hi > row.n - 1 ? row.n - 1 : m_hi;
    int j = (int)(c + p.half - (long)m_lo * p.up);  // <= 2 half by the choice of m_lo, >= 0 down to m_hi
    double ax = 0.0, ay = 0.0;
    for (int m = m_lo; m <= m_hi; ++m, j -= p.up) {
        const double hv = h[j];
        const cd v = in[m - m_a];
        ax = fma(hv, v.x, ax);
        ay = fma(hv, v.y, ay);
    }
    *ox = (double)p.up * ax;
    *oy = (double)p.up * ay;
}

// grid (ceil(nf_max / 4), B): one wave per frame of the clean row, E = 20 log10(|w x| + eps)
__global__ __launch_bounds__(kThreads) void stoi_energy_kernel(const int* __restrict__ lengths, const double* __restrict__ rs,
                                                               FsnStoiPlan p, double* __restrict__ energy) {
    const int b = blockIdx.y;
    const Row row = row_of(lengths, b, p);
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (i >= row.nf) return;  // whole waves; the kernel has no barrier
    const double* xr = rs + (long)b * 2 * p.n10_max + (long)i * kHop;  // i kHop + 255 < n10
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < kFrame / 64; ++e) {
        const int s = lane + 64 * e;
        const double v = stoi_window(s) * xr[s];
        acc = fma(v, v, acc);
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) energy[(long)b * p.nf_max + i] = 20.0 * log10(sqrt(acc) + kEps);
}

// grid B, one wave per row: frame i stays iff max(E) - 40 - E_i < 0; kept[] lists those frames in order
__global__ __launch_bounds__(64) void stoi_keep_kernel(const int* __restrict__ lengths, const double* __restrict__ energy,
                                                       FsnStoiPlan p, int* __restrict__ kept, int* __restrict__ n_kept) {
    const int b = blockIdx.x;
    const Row row = row_of(lengths, b, p);
    const int lane = threadIdx.x;
    const double* E = energy + (long)b * p.nf_max;
    int* kp = kept + (long)b * p.nf_max;
    double mx = -__builtin_huge_val();
    for (int i = lane; i < row.nf; i += 64) mx = fmax(mx, E[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    int base = 0;
    for (int i0 = 0; i0 < row.nf; i0 += 64) {
        const int i = i0 + lane;
        const bool keep = i < row.nf && (mx - 40.0) - E[i] < 0.0;
        const unsigned long long m = __ballot(keep);
        if (keep) kp[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += __popcll(m);
    }
    if (lane == 0) n_kept[b] = base;
}

// grid (ceil(m_max / 4), B): spectral frames m0 .. m0 + 3 of row b.  Sample s of frame m of the silence-free signal is
// the sum of the (windowed) kept frames m and m - 1 (s < 128) or m and m + 1 (s >= 128) at that position.
__global__ __launch_bounds__(kThreads) void stoi_band_kernel(const double* __restrict__ rs, const int* __restrict__ kept,
                                                             const int* __restrict__ n_kept, FsnStoiPlan p,
                                                             double* __restrict__ tob) {
    __shared__ cd a[kFramesPerGroup * kNfft];
    __shared__ cd tw[kNfft / 2];
    __shared__ double win[kFrame];
    __shared__ int live[kFramesPerGroup];
    const int b = blockIdx.y;
    const int M = n_kept[b] - 1;
    const int m0 = blockIdx.x * kFramesPerGroup;
    if (m0 >= M) return;
    const int s = threadIdx.x;
    fill_twiddles(tw, kNfft);
    win[s] = stoi_window(s);
    __syncthreads();
    const int* kp = kept + (long)b * p.nf_max;
    const double* xr = rs + (long)b * 2 * p.n10_max;
    const double* yr = xr + p.n10_max;
#pragma unroll
    for (int r = 0; r < kFramesPerGroup; ++r) {
        const int m = m0 + r;
        cd v{0.0, 0.0};
        if (m < M) {
            const long p0 = (long)kp[m] * kHop + s;
            double xv = win[s] * xr[p0], yv = win[s] * yr[p0];
            const int other = s < kHop ? (m >= 1 ? kp[m - 1] : -1) : kp[m + 1];  // m + 1 <= M = n_kept - 1
            if (other >= 0) {
                const int s2 = s < kHop ? s + kHop : s - kHop;
                const long p1 = (long)other * kHop + s2;
                xv += win[s2] * xr[p1];
                yv += win[s2] * yr[p1];
            }
            v = cd{win[s] * xv, win[s] * yv};
        }
        a[r * kNfft + s] = v;
        a[r * kNfft + kFrame + s] = cd{0.0, 0.0};
        // a signal whose frame is all zeros has a spectrum of zeros, not the split's rounding residue of the other one
        const int lx = __syncthreads_or(v.x != 0.0), ly = __syncthreads_or(v.y != 0.0);
        if (s == 0) live[r] = (lx ? 1 : 0) | (ly ? 2 : 0);
    }
    __syncthreads();
    lds_fft<false>(a, tw, kNfft, kLogNfft, kFramesPerGroup);
    // slot bitrev(k) of a row holds Z[k] = X[k] + i Y[k]:  X[k] = (Z[k] + conj Z[N - k]) / 2,  Y[k] = (Z[k] - conj Z[N - k]) / 2i
    constexpr int kEdges[kBands + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
    if (s < kFramesPerGroup * 2 * kBands) {
        const int r = s / (2 * kBands), sig = (s / kBands) & 1, band = s % kBands;
        const int m = m0 + r;
        if (m < M) {
            double acc = 0.0;
            for (int k = kEdges[band]; k < kEdges[band + 1]; ++k) {
                const cd z = a[r * kNfft + bitrev(k, kLogNfft)], zp = a[r * kNfft + bitrev(kNfft - k, kLogNfft)];
                const double re = sig ? z.y + zp.y : z.x + zp.x;
                const double im = sig ? zp.x - z.x : z.y - zp.y;
                acc += 0.25 * (re * re + im * im);
            }
            const double out = (live[r] >> sig) & 1 ? sqrt(acc) : 0.0;
            tob[(((long)b * 2 + sig) * kBands + band) * p.m_max + m] = out;
        }
    }
}

// grid (j_blocks, 15, B): segment j = frames j .. j + 29 of band blockIdx.y
__global__ __launch_bounds__(kThreads) void stoi_corr_kernel(const double* __restrict__ tob, const int* __restrict__ n_kept,
                                                             FsnStoiPlan p, double clip, double* __restrict__ partial) {
    __shared__ double scratch[kThreads / 64];
    const int b = blockIdx.z, band = blockIdx.y;
    const int J = n_kept[b] - 1 - (kSeg - 1);
    const int j0 = blockIdx.x * kThreads;
    if (j0 >= J) return;
    const int j = j0 + threadIdx.x;
    double corr = 0.0;
    if (j < J) {
        const double* xs = tob + (((long)b * 2) * kBands + band) * p.m_max + j;
        const double* ys = xs + (long)kBands * p.m_max;
        double x[kSeg], y[kSeg];
        double sxx = 0.0, syy = 0.0;
#pragma unroll
        for (int i = 0; i < kSeg; ++i) {
            x[i] = xs[i];
            y[i] = ys[i];
            sxx += x[i] * x[i];
            syy += y[i] * y[i];
        }
        const double scale = sqrt(sxx) / (sqrt(syy) + kEps);
        double mx = 0.0, my = 0.0;
#pragma unroll
        for (int i = 0; i < kSeg; ++i) {
            y[i] = fmin(y[i] * scale, x[i] * (1.0 + clip));
            mx += x[i];
            my += y[i];
        }
        mx /= (double)kSeg;
        my /= (double)kSeg;
        double nx = 0.0, ny = 0.0;
#pragma unroll
        for (int i = 0; i < kSeg; ++i) {
            x[i] -= mx;
            y[i] -= my;
            nx += x[i] * x[i];
            ny += y[i] * y[i];
        }
        nx = sqrt(nx) + kEps;
        ny = sqrt(ny) + kEps;
#pragma unroll
        for (int i = 0; i < kSeg; ++i) corr += (y[i] / ny) * (x[i] / nx);
    }
    corr = fsn_block_sum(corr, scratch);
    if (threadIdx.x == 0) partial[((long)b * kBands + band) * p.j_blocks + blockIdx.x] = corr;
}

// one thread per row: the row's partial sums band by band, workgroup by workgroup
__global__ __launch_bounds__(64) void stoi_finish_kernel(const double* __restrict__ partial, const int* __restrict__ n_kept,
                                                         FsnStoiPlan p, double* __restrict__ d) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int M = n_kept[b] - 1;
    if (M < kSeg) {
        d[b] = 1e-5;
        return;
    }
    const int J = M - (kSeg - 1);
    const int blocks = (J + kThreads - 1) / kThreads;
    double tot = 0.0;
    for (int band = 0; band < kBands; ++band)
        for (int i = 0; i < blocks; ++i) tot += partial[((long)b * kBands + band) * p.j_blocks + i];
    d[b] = tot / (double)(J * kBands);
}

// grid B: 10 log10(|a r|^2 / |e - a r|^2), a = <r, e> / <r, r>
__global__ __launch_bounds__(kSdrThreads) void si_sdr_kernel(const float* __restrict__ reference,
                                                             const float* __restrict__ estimate,
                                                             const int* __restrict__ lengths, int L_max,
                                                             double* __restrict__ out_db) {
    __shared__ double scratch[kSdrThreads / 64];
    const int b = blockIdx.x;
    const int n = fsn_stoi_row_samples(lengths, b, L_max);
    const float* rr = reference + (long)b * L_max;
    const float* er = estimate + (long)b * L_max;
    double srr = 0.0, sre = 0.0;
    for (int i = threadIdx.x; i < n; i += kSdrThreads) {
        const double r = (double)rr[i], e = (double)er[i];
        srr = fma(r, r, srr);
        sre = fma(r, e, sre);
    }
    srr = fsn_block_sum(srr, scratch);
    sre = fsn_block_sum(sre, scratch);
    const double alpha = sre / srr;
    double sp = 0.0, sn = 0.0;
    for (int i = threadIdx.x; i < n; i += kSdrThreads) {
        const double pr = alpha * (double)rr[i];
        const double nz = (double)er[i] - pr;
        sp = fma(pr, pr, sp);
        sn = fma(nz, nz, sn);
    }
    sp = fsn_block_sum(sp, scratch);
    sn = fsn_block_sum(sn, scratch);
    if (threadIdx.x == 0) out_db[b] = 10.0 * log10(sp / sn);
}

}  // namespace

int fsn_launch_stoi(const float* clean, const float* estimate, const int* lengths, const FsnStoiPlan& p,
                    const FsnStoiBuffers& w, double* d, hipStream_t s) {
    if (2 * p.half + 1 > kMaxTaps) {
        fsn_set_error("fsn_launch_stoi: %d taps, the resampling kernel holds %d", 2 * p.half + 1, kMaxTaps);
        return FSN_ERR_ARG;
    }
    if (p.half && ((kThreads - 1) * p.down + 2 * p.half) / p.up + 2 > kResampleIn) {
        fsn_set_error("fsn_launch_stoi: ratio %d / %d with %d taps: more input per workgroup than the resampling kernel holds",
                      p.up, p.down, 2 * p.half + 1);
        return FSN_ERR_ARG;
    }
    if (p.half) {
        hipLaunchKernelGGL(stoi_taps_kernel, dim3(1), dim3(1024), 0, s, w.taps, p.up, p.down, p.half);
        FSN_TRY_LAUNCH("stoi_taps_kernel");
    }
    hipLaunchKernelGGL(stoi_resample_kernel, dim3((p.n10_max + kThreads - 1) / kThreads, p.B), dim3(kThreads), 0, s, clean,
                       estimate, lengths, w.taps, p, w.rs);
    FSN_TRY_LAUNCH("stoi_resample_kernel");
    if (p.nf_max > 0) {
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((p.nf_max + kThreads / 64 - 1) / (kThreads / 64), p.B), dim3(kThreads), 0,
                           s, lengths, w.rs, p, w.energy);
        FSN_TRY_LAUNCH("stoi_energy_kernel");
    }
    hipLaunchKernelGGL(stoi_keep_kernel, dim3(p.B), dim3(64), 0, s, lengths, w.energy, p, w.kept, w.n_kept);
    FSN_TRY_LAUNCH("stoi_keep_kernel");
    if (p.m_max >= kSeg) {  // otherwise no row can reach 30 spectral frames
        hipLaunchKernelGGL(stoi_band_kernel, dim3((p.m_max + kFramesPerGroup - 1) / kFramesPerGroup, p.B), dim3(kThreads), 0,
                           s, w.rs, w.kept, w.n_kept, p, w.tob);
        FSN_TRY_LAUNCH("stoi_band_kernel");
        hipLaunchKernelGGL(stoi_corr_kernel, dim3(p.j_blocks, kBands, p.B), dim3(kThreads), 0, s, w.tob, w.n_kept, p,
                           pow(10.0, 15.0 / 20.0), w.partial);
        FSN_TRY_LAUNCH("stoi_corr_kernel");
    }
    hipLaunchKernelGGL(stoi_finish_kernel, dim3((p.B + 63) / 64), dim3(64), 0, s, w.partial, w.n_kept, p, d);
    return fsn_check_launch("stoi_finish_kernel");
}

int fsn_launch_si_sdr(const float* reference, const float* estimate, const int* lengths, int B, int L_max, double* out_db,
                      hipStream_t s) {
    hipLaunchKernelGGL(si_sdr_kernel, dim3(B), dim3(kSdrThreads), 0, s, reference, estimate, lengths, L_max, out_db);
    return fsn_check_launch("si_sdr_kernel");
}
