// Improved FullSubNet's glue for recordings of any length under the offline norms (fsn_improved_segment_*,
// fsn_api_improved_segment.hip): what improved_stream_kernels.hip does under the causal norms, for the model in segments of k
// frames t0 .. t0 + k - 1.  The reference divides twice by ONE mean per utterance (improved_fullsubnet/model.py:124-150 in
// front of the full-band model, :402-440 in front of every section, over the unfolded windows of the noisy magnitude AND of
// the full-band output), so the means are gathered in passes of their own, as fp64 sums in the state blob's fb_sum [B] and
// sb_sum [sections][B]:
//   stat      pass 1: every frame's sum of mag ** fdrc over the first Fm bins joins fb_sum[b]
//   front     pass 2: comp = mag ** fdrc and fb_in = comp / den.  den is float(fb_sum[b] / (Fm T_b)) + eps from the finished
//             sum (mode kOffline), or the running mean exactly as improved_stream_front_kernel forms it, fb_sum carried by this
//             kernel (mode kCumulative).  Pass 3 runs it again for comp alone (mode kCompOnly)
//   sums      pass 2, behind the full-band block: every section's sum over all units and window columns of a frame joins
//             sb_sum[i][b]; the block's output goes to the caller's plane [k][B][Fm], unpadded in B
//   sections  pass 3: every section's windows divided by float(sb_sum[i][b] / (N_i W_i T_b)) + eps
//   divisors  both kinds of divisor as the passes form them
// total[b] = T_b is row b's own frame count (device memory).  A frame at or past T_b adds nothing to any sum and its
// compressed magnitude is zero wherever it is an input (mag is not read there); what the blocks make of it is finite and
// never used.
// The rules of improved_stream_kernels.hip hold: a frame's own sum has a fixed shape (every thread adds its entries in index
// order, a butterfly per wave, the four waves in order), the fp64 carry advances frame by frame in frame order, one workgroup
// owns a state field, and nothing depends on where a call begins or ends - two segmentations of a recording give the same
// bits.
#include "improved_glue.h"

using namespace fsn_improved_glue;

namespace {

enum FrontMode { kOffline = 0, kCumulative = 1, kCompOnly = 2 };

__device__ __forceinline__ int row_total(const int* total, int b) {  // never below one frame: no count is zero
    const int t = total[b];
    return t < 1 ? 1 : t;
}
// float(sum / count) + eps: the reference's fp32 operations on the exactly carried sum
__device__ __forceinline__ float offline_den(double sum, double count) { return (float)(sum / count) + kFsnEpsilon; }
// this call's frames that lie inside a row of `tot` frames
__device__ __forceinline__ int frames_inside(int tot, long t0, int k) {
    const long left = (long)tot - t0;
    return left <= 0 ? 0 : left < k ? (int)left : k;
}
__device__ __forceinline__ float compress(float m, int sqrt_mode) { return sqrt_mode ? sqrtf(m) : m; }

// One workgroup per row b; its frames inside the row in turn.
__global__ __launch_bounds__(256) void improved_segment_stat_kernel(const float* __restrict__ mag, double* __restrict__ fb_sum,
                                                                    const int* __restrict__ total, const FsnImprovedStream a) {
    __shared__ double part[4];
    const int b = blockIdx.x;
    const int n = frames_inside(row_total(total, b), a.t0, a.k);
    double run = fb_sum[b];
    for (int t = 0; t < n; ++t) {
        double s = 0.0;
        for (int f = threadIdx.x; f < a.Fm; f += 256) s += (double)compress(mag[((size_t)b * a.F + f) * a.k + t], a.sqrt_mode);
        __syncthreads();  // the frame before has read `part`
        s = block_sum(s, part);
        if (threadIdx.x == 0) run += s;
    }
    if (threadIdx.x == 0) fb_sum[b] = run;
}

// One workgroup per (padded) row b; the frames in turn.  comp, fb_in [k][Bp][FmP], zero in the padding.
__global__ __launch_bounds__(256) void improved_segment_front_kernel(const float* __restrict__ mag, float* __restrict__ comp,
                                                                     float* __restrict__ fb_in, double* __restrict__ fb_sum,
                                                                     long* __restrict__ steps, const int* __restrict__ total,
                                                                     int mode, const FsnImprovedStream a) {
    __shared__ double part[4];
    __shared__ float den_s;
    const int b = blockIdx.x;
    if (b >= a.B) {  // padding rows: zeros
        for (int t = 0; t < a.k; ++t)
            for (int f = threadIdx.x; f < a.FmP; f += 256) {
                const size_t i = ((size_t)t * a.Bp + b) * a.FmP + f;
                comp[i] = 0.f;
                if (mode != kCompOnly) fb_in[i] = 0.f;
            }
        return;
    }
    const int tot = row_total(total, b);
    const int n = frames_inside(tot, a.t0, a.k);
    double run = mode == kCompOnly ? 0.0 : fb_sum[b];
    float den = mode == kOffline ? offline_den(run, (double)a.Fm * (double)tot) : 1.f;
    for (int t = 0; t < a.k; ++t) {
        const size_t row = ((size_t)t * a.Bp + b) * a.FmP;
        const bool inside = t < n;
        double s = 0.0;
        for (int f = threadIdx.x; f < a.Fm; f += 256) {
            const float v = inside ? compress(mag[((size_t)b * a.F + f) * a.k + t], a.sqrt_mode) : 0.f;
            comp[row + f] = v;
            s += (double)v;
        }
        if (mode == kCumulative) {  // the same for the whole workgroup
            s = block_sum(s, part);
            if (threadIdx.x == 0) {
                if (inside) run += s;
                den_s = (float)(run / ((double)a.Fm * ((double)a.t0 + t + 1.0))) + kFsnEpsilon;
            }
            __syncthreads();
            den = den_s;
        }
        for (int f = threadIdx.x; f < a.FmP; f += 256) {
            if (f >= a.Fm) comp[row + f] = 0.f;
            if (mode != kCompOnly) fb_in[row + f] = f < a.Fm ? comp[row + f] / den : 0.f;  // this thread's own store above
        }
    }
    if (threadIdx.x == 0 && mode != kCompOnly) {
        if (mode == kCumulative) fb_sum[b] = run;
        steps[b] = a.t0 + a.k;
    }
}

// One workgroup per (row b, section i); the frames in turn, a frame's two spectra staged in LDS.  Section 0's workgroup also
// copies the full-band output of its row to the caller's plane.
__global__ __launch_bounds__(256) void improved_segment_sums_kernel(const float* __restrict__ comp, const float* __restrict__ fb_ws,
                                                                    long ld_fb, float* __restrict__ fb_out,
                                                                    double* __restrict__ sb_sum, const int* __restrict__ total,
                                                                    const FsnImprovedStream a) {
    __shared__ float bins[2 * kFsnImprovedMaxBins];
    __shared__ double part[4];
    const int b = blockIdx.x, i = blockIdx.y;
    const FsnImprovedSection& q = a.s[i];
    const int E = q.units * q.W;
    const int n = frames_inside(row_total(total, b), a.t0, a.k);
    double run = sb_sum[(size_t)i * a.B + b];
    for (int t = 0; t < a.k; ++t) {
        if (t >= n && i != 0) break;  // past the row's end only the copy is left (the same for the whole workgroup)
        __syncthreads();  // the frame before is read
        const size_t r = (size_t)t * a.Bp + b;
        for (int f = threadIdx.x; f < a.Fm; f += 256) {
            const float v = fb_ws[r * ld_fb + f];
            bins[f] = comp[r * a.FmP + f];
            bins[a.Fm + f] = v;
            if (i == 0) fb_out[((size_t)t * a.B + b) * a.Fm + f] = v;
        }
        if (t >= n) continue;
        __syncthreads();
        double s = 0.0;
        for (int e = threadIdx.x; e < E; e += 256) s += (double)section_entry(bins, q, a.Fm, e);
        s = block_sum(s, part);
        if (threadIdx.x == 0) run += s;
    }
    if (threadIdx.x == 0) sb_sum[(size_t)i * a.B + b] = run;
}

// One workgroup per (row b, section i): improved_stream_sections_kernel with the one divisor of the finished sum.  comp
// [k][Bp][FmP] (this call's front kernel), fb_out [k][B][Fm] (the caller's plane).
__global__ __launch_bounds__(256) void improved_segment_sections_kernel(const float* __restrict__ comp,
                                                                        const float* __restrict__ fb_out,
                                                                        const double* __restrict__ sb_sum,
                                                                        const int* __restrict__ total, const FsnImprovedStream a) {
    __shared__ float bins[2 * kFsnImprovedMaxBins];
    const int b = blockIdx.x, i = blockIdx.y;
    const FsnImprovedSection& q = a.s[i];
    const int E = q.units * q.W, pad = q.Ip - q.W;
    const size_t row0 = (size_t)b * q.units;
    const float den = offline_den(sb_sum[(size_t)i * a.B + b], (double)E * (double)row_total(total, b));
    for (int t = 0; t < a.k; ++t) {
        __syncthreads();  // the frame before is read
        for (int f = threadIdx.x; f < a.Fm; f += 256) {
            bins[f] = comp[((size_t)t * a.Bp + b) * a.FmP + f];
            bins[a.Fm + f] = fb_out[((size_t)t * a.B + b) * a.Fm + f];
        }
        __syncthreads();
        float* x = q.x + ((size_t)t * q.Np + row0) * q.Ip;
        for (int e = threadIdx.x; e < E; e += 256) {
            const int u = e / q.W;
            x[(size_t)u * q.Ip + (e - u * q.W)] = section_entry(bins, q, a.Fm, e) / den;
        }
        for (int e = threadIdx.x; e < q.units * pad; e += 256) {  // the padded columns of this row's units
            const int u = e / pad;
            x[(size_t)u * q.Ip + q.W + (e - u * pad)] = 0.f;
        }
        if (b == 0) {  // the padded rows of the section
            float* z = q.x + ((size_t)t * q.Np + (size_t)a.B * q.units) * q.Ip;
            const int n = (q.Np - a.B * q.units) * q.Ip;
            for (int e = threadIdx.x; e < n; e += 256) z[e] = 0.f;
        }
    }
}

// One thread per (b, 0 the full-band divisor | 1 + i section i's)
__global__ __launch_bounds__(256) void improved_segment_divisors_kernel(const double* __restrict__ fb_sum,
                                                                        const double* __restrict__ sb_sum,
                                                                        const int* __restrict__ total, float* __restrict__ den_fb,
                                                                        float* __restrict__ den_sb, const FsnImprovedStream a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.B * (a.n + 1)) return;
    const int b = j % a.B, i = j / a.B - 1;
    const double tot = (double)row_total(total, b);
    if (i < 0) den_fb[b] = offline_den(fb_sum[b], (double)a.Fm * tot);
    else den_sb[(size_t)i * a.B + b] = offline_den(sb_sum[(size_t)i * a.B + b], (double)(a.s[i].units * a.s[i].W) * tot);
}

// the statistic and the divisors run without a workspace: what they read of the record
int check_rows(const FsnImprovedStream& a, const char* what) {
    bool ok = a.B >= 1 && a.F >= 2 && a.Fm == a.F - 1 && a.k >= 1 && a.t0 >= 0 && a.n >= 1 && a.n <= 8 &&
              (a.sqrt_mode == 0 || a.sqrt_mode == 1);
    for (int i = 0; ok && i < a.n; ++i) ok = a.s[i].units >= 1 && a.s[i].W >= 1;
    if (!ok) {
        fsn_set_error("%s: geometry outside the kernel (rows, bins, frames >= 1, 1 .. 8 sections)", what);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

}  // namespace

int fsn_launch_improved_segment_stat(const float* mag, double* fb_sum, const int* total, const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_rows(a, "improved segment statistic");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(improved_segment_stat_kernel, dim3((unsigned)a.B), dim3(256), 0, s, mag, fb_sum, total, a);
    return fsn_check_launch("improved_segment_stat_kernel");
}

int fsn_launch_improved_segment_front(int mode, const float* mag, float* comp, float* fb_in, double* fb_sum, long* steps,
                                      const int* total, const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "improved segment front");
    if (rc != FSN_OK) return rc;
    if (mode < kOffline || mode > kCompOnly || !mag || !comp || !total || (mode != kCompOnly && (!fb_in || !fb_sum || !steps))) {
        fsn_set_error("improved segment front: mode %d outside 0 .. 2, or a NULL array the mode reads or writes", mode);
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(improved_segment_front_kernel, dim3((unsigned)a.Bp), dim3(256), 0, s, mag, comp, fb_in, fb_sum, steps, total,
                       mode, a);
    return fsn_check_launch("improved_segment_front_kernel");
}

int fsn_launch_improved_segment_sums(const float* comp, const float* fb_ws, long ld_fb, float* fb_out, double* sb_sum,
                                     const int* total, const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "improved segment sums");
    if (rc != FSN_OK) return rc;
    if (ld_fb < a.Fm) {
        fsn_set_error("improved segment sums: full-band row stride %ld below the %d bins", ld_fb, a.Fm);
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(improved_segment_sums_kernel, dim3((unsigned)a.B, (unsigned)a.n), dim3(256), 0, s, comp, fb_ws, ld_fb, fb_out,
                       sb_sum, total, a);
    return fsn_check_launch("improved_segment_sums_kernel");
}

int fsn_launch_improved_segment_sections(const float* comp, const float* fb_out, const double* sb_sum, const int* total,
                                         const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "improved segment sections");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(improved_segment_sections_kernel, dim3((unsigned)a.B, (unsigned)a.n), dim3(256), 0, s, comp, fb_out, sb_sum,
                       total, a);
    return fsn_check_launch("improved_segment_sections_kernel");
}

int fsn_launch_improved_segment_divisors(const double* fb_sum, const double* sb_sum, const int* total, float* den_fb, float* den_sb,
                                         const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_rows(a, "improved segment divisors");
    if (rc != FSN_OK) return rc;
    const int n = a.B * (a.n + 1);
    hipLaunchKernelGGL(improved_segment_divisors_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, fb_sum, sb_sum, total,
                       den_fb, den_sb, a);
    return fsn_check_launch("improved_segment_divisors_kernel");
}
