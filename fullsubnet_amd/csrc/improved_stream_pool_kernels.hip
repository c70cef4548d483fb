// Streaming pool for Improved FullSubNet (fsn_improved_stream_pool_*): the model step of fsn_improved_stream_step over a
// SUBSET of the slots of a pool whose sessions open, advance and close on their own, and the frame transforms around it at
// the model's own size (960 / 480 at 48 kHz: fft_kernels.hip's pool kernels are 512 / 256 only).
//
// The pool's state is one record per slot (FsnImprovedPoolLayout, fsn_common.h).  A step (fsn_api_improved_stream_pool.hip)
//   1. gathers the listed slots' (h, c) rows, fp64 sums and counts into a compact state in exactly the lockstep entry's
//      layout at B = n (pad rows and rows of an id outside the pool are zeros, so every row the recurrent kernels touch is
//      finite; such a row's count is -1),
//   2. runs the lockstep entry's own sequence on it - improved_stream_kernels.hip's front and sections kernels take every
//      row's divisor count from the gathered counts instead of one t0 -,
//   3. scatters rows, sums and counts + k back to the listed, valid records.
// Slots that are not listed are never written.  One workgroup (or thread) owns a record's field in every kernel; all row
// copies move 16 bytes per lane, coalesced along H.
//
// Transforms: one workgroup per listed slot and frame.  The arithmetic is dft_kernels.hip's, restated line by line: the
// fp32 windowed frame, an fp64 DFT from the exact N-entry twiddle table in LDS - two-level (N = P Q) where N splits, direct
// where it does not -, one rounding to fp32; the inverse likewise, then fp32 window, overlap-add in ascending frame order
// and the division by the overlap-added squared window as ola_generic_kernel forms it.
#include "fsn_common.h"

namespace {

// the record of slots[i], or NULL for i >= n or an id outside the pool (such a row is skipped by every kernel)
__device__ __forceinline__ char* record_of(char* state, size_t slot_bytes, int capacity, const int* slots, int n, int i) {
    if (i >= n) return nullptr;
    const int slot = slots[i];
    return (slot >= 0 && slot < capacity) ? state + (size_t)slot * slot_bytes : nullptr;
}

// ---- records <-> the compact state ------------------------------------------------------------------------------------------
// blockIdx.y = 4 block + array for the (h, c) arrays (block 0 the full-band one: one row per slot; block 1 + i section i:
// units_i rows per slot, row b units_i + u as the lockstep glue orders them), a thread moves one f32x4; the plane behind them
// moves the sums and the count, one thread per listed row.  Gather fills every padded row; scatter writes the listed, valid
// ones and their counts + k (the last kernel of a step: nothing reads a record after it).
template <bool SCATTER>
__global__ __launch_bounds__(256) void improved_pool_rows_kernel(const FsnImprovedPool a) {
    const int planes = 4 * (1 + a.L.n);
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if ((int)blockIdx.y == planes) {
        if (idx >= a.n) return;
        const int i = (int)idx;
        char* rec = record_of(a.state, a.L.slot_bytes, a.capacity, a.slots, a.n, i);
        if (SCATTER) {
            if (!rec) return;
            *reinterpret_cast<double*>(rec + a.L.fb_sum) = a.fb_sum[i];
            for (int j = 0; j < a.L.n; ++j) reinterpret_cast<double*>(rec + a.L.sb_sum)[j] = a.sb_sum[(size_t)j * a.n + i];
            *reinterpret_cast<long*>(rec + a.L.steps) = a.t0[i] + a.k;
        } else {
            a.fb_sum[i] = rec ? *reinterpret_cast<const double*>(rec + a.L.fb_sum) : 0.0;
            for (int j = 0; j < a.L.n; ++j)
                a.sb_sum[(size_t)j * a.n + i] = rec ? reinterpret_cast<const double*>(rec + a.L.sb_sum)[j] : 0.0;
            long t0 = -1;
            if (rec) {
                t0 = *reinterpret_cast<const long*>(rec + a.L.steps);
                t0 = t0 < 0 ? 0 : t0;
            }
            a.t0[i] = t0;
        }
        return;
    }
    const int blk = blockIdx.y / 4, arr = blockIdx.y % 4;
    const int H4 = (blk ? a.L.Hs : a.L.Hf) / 4, rps = blk ? a.L.units[blk - 1] : 1;
    const long row = idx / H4;
    const int c4 = (int)(idx % H4);
    if (row >= a.rows[blk]) return;
    const int i = (int)(row / rps), r = (int)(row % rps);
    char* rec = record_of(a.state, a.L.slot_bytes, a.capacity, a.slots, a.n, i);
    f32x4* tile = reinterpret_cast<f32x4*>(a.tile[blk][arr]) + row * H4 + c4;
    const size_t off = blk ? a.L.sb[blk - 1][arr] : a.L.fb[arr];
    if (SCATTER) {
        if (rec) *(reinterpret_cast<f32x4*>(rec + off) + (size_t)r * H4 + c4) = *tile;
    } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rec) v = *(reinterpret_cast<const f32x4*>(rec + off) + (size_t)r * H4 + c4);
        *tile = v;
    }
}

// ---- the transforms -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fill_twiddles(double* c, double* s, int N) {
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        double sv, cv;
        sincospi(2.0 * (double)n / (double)N, &sv, &cv);
        c[n] = cv;
        s[n] = sv;
    }
}

// Analysis: frame = in_tail[slot] ++ hops[i], window, real DFT of N = 2 hop points -> spec_re / spec_im [F] and frame_no[i]
// in the record, mag [n][F]; then in_tail[slot] = hops[i].  Frame 0 of a session takes the reflected samples y[hop .. 1] as
// its left half: prime[i] holds y[1 .. hop] and is read backwards (prime == NULL: the caller's promise that no listed
// session is at frame 0).  A row with an id outside the pool or a negative frame number writes a zero magnitude and no state.
// kTwo: N = P Q (dft2_stft_kernel), else the direct form (dft_stft_kernel).  LDS doubles: 5 N / 3 N.
template <bool kTwo>
__global__ __launch_bounds__(256) void improved_pool_analysis_kernel(char* __restrict__ state, const FsnImprovedPoolLayout L,
                                                                     int capacity, const int* __restrict__ slots, int n,
                                                                     const float* __restrict__ hops, const float* __restrict__ prime,
                                                                     const int* __restrict__ frame_no,
                                                                     const float* __restrict__ window, float* __restrict__ mag,
                                                                     int P, int Q) {
    extern __shared__ double sh[];
    const int hop = L.hop, N = 2 * L.hop, F = L.F, i = blockIdx.x;
    char* rec = record_of(state, L.slot_bytes, capacity, slots, n, i);
    const int t = rec ? frame_no[i] : -1;
    if (t < 0) {  // the whole workgroup
        for (int f = threadIdx.x; f < F; f += blockDim.x) mag[(long)i * F + f] = 0.f;
        return;
    }
    double *c = sh, *s = sh + N, *x = sh + 2 * N;
    fill_twiddles(c, s, N);
    float* tail = reinterpret_cast<float*>(rec + L.in_tail);
    for (int nn = threadIdx.x; nn < N; nn += blockDim.x) {
        float xs;
        if (nn < hop)
            xs = (t == 0 && prime) ? prime[(long)i * hop + hop - 1 - nn] : tail[nn];  // y[hop - nn]
        else
            xs = hops[(long)i * hop + nn - hop];
        x[nn] = (double)(xs * window[nn]);  // the frame is rounded to fp32 like ATen's
    }
    __syncthreads();  // every read of the carried hop is done
    for (int nn = threadIdx.x; nn < hop; nn += blockDim.x) tail[nn] = hops[(long)i * hop + nn];
    if (threadIdx.x == 0) *reinterpret_cast<int*>(rec + L.frame) = t;
    float* sre = reinterpret_cast<float*>(rec + L.spec_re);
    float* sim = reinterpret_cast<float*>(rec + L.spec_im);
    if (kTwo) {
        double *br = sh + 3 * N, *bi = sh + 4 * N;
        for (int j = threadIdx.x; j < N; j += blockDim.x) {
            const int k1 = j / Q, n2 = j - k1 * Q;
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
            sre[k] = fr32;
            sim[k] = fi32;
            mag[(long)i * F + k] = (float)sqrt((double)fr32 * fr32 + (double)fi32 * fi32);
        }
    } else {
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            double ar = 0.0, ai = 0.0;
            int idx = 0;
            for (int nn = 0; nn < N; ++nn) {
                const double xv = x[nn];
                ar = fma(xv, c[idx], ar);
                ai = fma(-xv, s[idx], ai);
                idx += f;
                idx = idx >= N ? idx - N : idx;
            }
            const float fr32 = (float)ar, fi32 = (float)ai;
            sre[f] = fr32;
            sim[f] = fi32;
            mag[(long)i * F + f] = (float)sqrt((double)fr32 * fr32 + (double)fi32 * fi32);
        }
    }
}

// Synthesis: the record's waiting spectrum times the two mask planes (mask [n][2][F]: mask[0] re, mask[1] im, fp32 products),
// the inverse real DFT, the window -> the windowed frame m = the record's frame number, staged in LDS.  Then ola_generic_kernel
// one hop at a time: frame m >= 1 emits out[i][s] = (ola_tail[s] + wframe[s]) / (w[s + hop]^2 + w[s]^2); frame 0 emits nothing
// (its first half is the trimmed centre pad); ola_tail[slot] = the frame's second half.  tail_samples[i] >= 0: the session
// ends with this frame - the first tail_samples samples of that second half, divided by the one-frame envelope, go to
// out[i][hop ..].  Everything else of out [n][2 hop] is zeros; a row with an id outside the pool is all zeros.
// kTwo: dft2_irfft_kernel's form (LDS 6 N doubles, the frame staged over the spectrum's first array), else
// dft_irfft_kernel's (2 F + 2 N doubles and N floats).
template <bool kTwo>
__global__ __launch_bounds__(256) void improved_pool_synthesis_kernel(char* __restrict__ state, const FsnImprovedPoolLayout L,
                                                                      int capacity, const int* __restrict__ slots, int n,
                                                                      const float* __restrict__ mask,
                                                                      const int* __restrict__ tail_samples,
                                                                      const float* __restrict__ window, float* __restrict__ out,
                                                                      int P, int Q) {
    extern __shared__ double sh[];
    const int hop = L.hop, N = 2 * L.hop, F = L.F, i = blockIdx.x;
    char* rec = record_of(state, L.slot_bytes, capacity, slots, n, i);
    float* o = out + (long)i * 2 * hop;
    if (!rec) {  // the whole workgroup
        for (int j = threadIdx.x; j < 2 * hop; j += blockDim.x) o[j] = 0.f;
        return;
    }
    const float* sre = reinterpret_cast<const float*>(rec + L.spec_re);
    const float* sim = reinterpret_cast<const float*>(rec + L.spec_im);
    const float* mr = mask + (long)i * 2 * F;
    const float* mi = mr + F;
    float* wf;
    if (kTwo) {
        double *c = sh, *s = sh + N, *xr = sh + 2 * N, *xi = sh + 3 * N, *cr = sh + 4 * N, *ci = sh + 5 * N;
        wf = reinterpret_cast<float*>(xr);  // free once the first stage is through
        fill_twiddles(c, s, N);
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            const bool edge = f == 0 || f == N / 2;  // C2R: imaginary parts of DC / Nyquist are ignored
            const float er = mr[f] * sre[f], ei = mi[f] * sim[f];
            const double vr = (double)er, vi = edge ? 0.0 : (double)ei;
            xr[f] = vr;
            xi[f] = vi;
            if (!edge) {  // X[N - f] = conj(X[f])
                xr[N - f] = vr;
                xi[N - f] = -vi;
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < N; j += blockDim.x) {
            const int k1 = j / Q, n2 = j - k1 * Q;
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
        for (int nn = threadIdx.x; nn < N; nn += blockDim.x) {
            const int n1 = nn / Q, n2 = nn - n1 * Q;
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
            wf[nn] = v * window[nn];
        }
    } else {
        double *xr = sh, *xi = sh + F, *c = sh + 2 * F, *s = sh + 2 * F + N;
        wf = reinterpret_cast<float*>(sh + 2 * F + 2 * N);
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            const bool edge = f == 0 || f == N / 2;
            const double k = edge ? 1.0 : 2.0;
            const float er = mr[f] * sre[f], ei = mi[f] * sim[f];
            xr[f] = k * (double)er;
            xi[f] = edge ? 0.0 : k * (double)ei;
        }
        fill_twiddles(c, s, N);
        __syncthreads();
        for (int nn = threadIdx.x; nn < N; nn += blockDim.x) {
            double acc = 0.0;
            int idx = 0;
            for (int f = 0; f < F; ++f) {
                acc = fma(xr[f], c[idx], acc);
                acc = fma(-xi[f], s[idx], acc);
                idx += nn;
                idx = idx >= N ? idx - N : idx;
            }
            const float v = (float)(acc / (double)N);
            wf[nn] = v * window[nn];
        }
    }
    __syncthreads();
    const int m = *reinterpret_cast<const int*>(rec + L.frame), rem = tail_samples[i];
    float* tail = reinterpret_cast<float*>(rec + L.ola_tail);
    for (int j = threadIdx.x; j < hop; j += blockDim.x) {
        const float w_lo = window[j + hop], w_hi = window[j];
        float env = w_lo * w_lo;
        env = env + w_hi * w_hi;
        const float acc = tail[j] + wf[j];
        o[j] = m >= 1 ? acc / env : 0.f;
        const float next = wf[j + hop];
        tail[j] = next;
        o[hop + j] = j < rem ? next / (w_lo * w_lo) : 0.f;
    }
}

// dft_kernels.hip's split: P <= Q, both > 3, P as large as possible; 0: the direct form
int split_of(int N) {
    if (N > 2048) return 0;
    int best = 0;
    for (int p = 4; (long)p * p <= N; ++p)
        if (N % p == 0) best = p;
    return best;
}

int check_pool(const FsnImprovedPool& a, const char* what) {
    bool ok = a.state && a.slots && a.fb_sum && a.sb_sum && a.t0 && a.capacity >= 1 && a.n >= 1 && a.n <= a.capacity && a.k >= 1 &&
              a.L.n >= 1 && a.L.n <= 8 && a.L.Hf >= 4 && a.L.Hf % 4 == 0 && a.L.Hs >= 4 && a.L.Hs % 4 == 0 && a.rows[0] >= a.n;
    for (int b = 0; ok && b <= a.L.n; ++b) {
        ok = a.rows[b] >= (b ? (long)a.n * a.L.units[b - 1] : (long)a.n);
        for (int arr = 0; ok && arr < 4; ++arr) ok = a.tile[b][arr] && (uintptr_t)a.tile[b][arr] % 16 == 0;
    }
    if (!ok) {
        fsn_set_error("%s: geometry outside the kernel (1 .. 8 sections, hidden sizes multiples of 4, padded rows not below the rows)", what);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

int check_transform(const FsnImprovedPoolLayout& L, int capacity, int n, const char* what) {
    if (capacity < 1 || n < 1 || L.hop < 2 || L.F != L.hop + 1 || 2 * L.hop > 4096) {
        fsn_set_error("%s: geometry outside the kernel (n_fft = 2 hop = 2 (F - 1) in 4 .. 4096)", what);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

}  // namespace

static int pool_rows(bool scatter, const FsnImprovedPool& a, hipStream_t s) {
    const int rc = check_pool(a, scatter ? "improved pool scatter" : "improved pool gather");
    if (rc != FSN_OK) return rc;
    long threads = a.n;
    for (int b = 0; b <= a.L.n; ++b) {
        const long t = (long)a.rows[b] * ((b ? a.L.Hs : a.L.Hf) / 4);
        threads = t > threads ? t : threads;
    }
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)(4 * (1 + a.L.n) + 1));
    if (scatter)
        hipLaunchKernelGGL(improved_pool_rows_kernel<true>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(improved_pool_rows_kernel<false>, grid, dim3(256), 0, s, a);
    return fsn_check_launch("improved_pool_rows_kernel");
}
int fsn_launch_improved_pool_gather(const FsnImprovedPool& a, hipStream_t s) { return pool_rows(false, a, s); }
int fsn_launch_improved_pool_scatter(const FsnImprovedPool& a, hipStream_t s) { return pool_rows(true, a, s); }

int fsn_launch_improved_pool_analysis(void* state, const FsnImprovedPoolLayout& L, int capacity, const int* slots, int n,
                                      const float* hops, const float* prime, const int* frame_no, const float* window, float* mag,
                                      hipStream_t s) {
    const int rc = check_transform(L, capacity, n, "improved pool analysis");
    if (rc != FSN_OK) return rc;
    const int N = 2 * L.hop;
    if (const int P = split_of(N)) {
        hipLaunchKernelGGL(improved_pool_analysis_kernel<true>, dim3(n), dim3(256), 5 * N * sizeof(double), s,
                           static_cast<char*>(state), L, capacity, slots, n, hops, prime, frame_no, window, mag, P, N / P);
        return fsn_check_launch("improved_pool_analysis_kernel");
    }
    const size_t lds = 3 * N * sizeof(double);  // 96 KB at N = 4096: above 64 KB a launch needs the attribute raised
    if (lds > 64 * 1024) FSN_TRY_RESERVE_LDS("improved pool analysis", improved_pool_analysis_kernel<false>, lds);
    hipLaunchKernelGGL(improved_pool_analysis_kernel<false>, dim3(n), dim3(256), lds, s, static_cast<char*>(state), L, capacity,
                       slots, n, hops, prime, frame_no, window, mag, 0, 0);
    return fsn_check_launch("improved_pool_analysis_kernel");
}

int fsn_launch_improved_pool_synthesis(void* state, const FsnImprovedPoolLayout& L, int capacity, const int* slots, int n,
                                       const float* mask, const int* tail_samples, const float* window, float* out, hipStream_t s) {
    const int rc = check_transform(L, capacity, n, "improved pool synthesis");
    if (rc != FSN_OK) return rc;
    const int N = 2 * L.hop;
    if (const int P = split_of(N)) {
        const size_t lds = 6 * N * sizeof(double);  // 96 KB at N = 2048
        if (lds > 64 * 1024) FSN_TRY_RESERVE_LDS("improved pool synthesis", improved_pool_synthesis_kernel<true>, lds);
        hipLaunchKernelGGL(improved_pool_synthesis_kernel<true>, dim3(n), dim3(256), lds, s, static_cast<char*>(state), L, capacity,
                           slots, n, mask, tail_samples, window, out, P, N / P);
        return fsn_check_launch("improved_pool_synthesis_kernel");
    }
    const size_t lds = (2 * (size_t)L.F + 2 * N) * sizeof(double) + N * sizeof(float);
    if (lds > 64 * 1024) FSN_TRY_RESERVE_LDS("improved pool synthesis", improved_pool_synthesis_kernel<false>, lds);
    hipLaunchKernelGGL(improved_pool_synthesis_kernel<false>, dim3(n), dim3(256), lds, s, static_cast<char*>(state), L, capacity,
                       slots, n, mask, tail_samples, window, out, 0, 0);
    return fsn_check_launch("improved_pool_synthesis_kernel");
}
