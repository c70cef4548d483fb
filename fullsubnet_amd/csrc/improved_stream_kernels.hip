// Improved FullSubNet's glue with carried state (fsn_improved_stream_step, fsn_api_improved_stream.hip): what
// section_kernels.hip and norm_kernels.hip do for a whole utterance, for k more model steps t0 .. t0 + k - 1 of B streams in
// lockstep.  Tensors are time-major ([k][rows][columns], the layout the stateful layer entry takes).  Three kernels:
//   front     improved_fullsubnet/model.py:565-567 under cumulative_laplace_norm: mag ** fdrc without the last bin, and that
//             divided by the running mean of the stream's Fm (t + 1) values so far
//   sections  model.py:402-440 for every section in one launch: unit u of the band sees the bins lower + u c - n ..
//             lower + (u + 1) c + n - 1 of the compressed magnitude and of the full-band output (mirrored at both ends of
//             the spectrum, the unfolded tensor never formed), divided by the running mean of the section's N W (t + 1)
//             entries so far: cumulative_laplace_norm of the [B, N, 1, W, T] input seen as [B, 1, N W, T]
//   mask      model.py:443-449, 575: the sections' output rows in bin order as the mask [B][2][F][k], last bin zero
// The running sums are fp64 and continue frame by frame from the state; a frame's own sum has a fixed shape (every thread adds
// its entries in index order, a butterfly per wave, the four waves in order), so nothing depends on where a call begins or
// ends and two chunkings of a stream give the same bits.  The count the divisors start from is t0 for all rows, or each
// row's own (FsnImprovedStream::t0_rows: the streaming pool, fsn_api_improved_stream_pool.hip).  One workgroup owns a state field: none is read by one workgroup and
// written by another.
#include "improved_glue.h"

using namespace fsn_improved_glue;

namespace {

// One workgroup per (padded) row b; the frames in turn.
__global__ __launch_bounds__(256) void improved_stream_front_kernel(const float* __restrict__ mag, float* __restrict__ comp,
                                                                    float* __restrict__ fb_in, double* __restrict__ fb_sum,
                                                                    long* __restrict__ steps, const FsnImprovedStream a) {
    __shared__ double part[4];
    __shared__ float den_s;
    const int b = blockIdx.x;
    if (b >= a.B) {  // padding rows: zeros
        for (int t = 0; t < a.k; ++t)
            for (int f = threadIdx.x; f < a.FmP; f += 256) {
                const size_t i = ((size_t)t * a.Bp + b) * a.FmP + f;
                comp[i] = 0.f;
                fb_in[i] = 0.f;
            }
        return;
    }
    const long t0_row = a.t0_rows ? a.t0_rows[b] : a.t0;  // uniform over the workgroup
    const bool idle = t0_row < 0;                          // a pool row of no session: zeros in, a fresh stream's count
    const long t0 = idle ? 0 : t0_row;
    double run = fb_sum[b];
    for (int t = 0; t < a.k; ++t) {
        const size_t row = ((size_t)t * a.Bp + b) * a.FmP;
        double s = 0.0;
        for (int f = threadIdx.x; f < a.Fm; f += 256) {
            const float m = idle ? 0.f : mag[((size_t)b * a.F + f) * a.k + t];
            const float v = a.sqrt_mode ? sqrtf(m) : m;
            comp[row + f] = v;
            s += (double)v;
        }
        s = block_sum(s, part);
        if (threadIdx.x == 0) {
            run += s;
            den_s = (float)(run / ((double)a.Fm * ((double)t0 + t + 1.0))) + kFsnEpsilon;
        }
        __syncthreads();
        const float den = den_s;
        for (int f = threadIdx.x; f < a.FmP; f += 256) {
            if (f < a.Fm) fb_in[row + f] = comp[row + f] / den;  // this thread's own store above
            else comp[row + f] = 0.f, fb_in[row + f] = 0.f;
        }
    }
    if (threadIdx.x == 0) {
        fb_sum[b] = run;
        steps[b] = t0 + a.k;
    }
}

// One workgroup per (stream b, section i); the frames in turn, a frame's two spectra staged in LDS.
__global__ __launch_bounds__(256) void improved_stream_sections_kernel(const float* __restrict__ comp,
                                                                       const float* __restrict__ fb_out, long ld_fb,
                                                                       double* __restrict__ sb_sum, const FsnImprovedStream a) {
    __shared__ float bins[2 * kFsnImprovedMaxBins];
    __shared__ double part[4];
    __shared__ float den_s;
    const int b = blockIdx.x, i = blockIdx.y;
    const FsnImprovedSection& q = a.s[i];
    const int E = q.units * q.W, pad = q.Ip - q.W;
    const size_t row0 = (size_t)b * q.units;
    const long t0_row = a.t0_rows ? a.t0_rows[b] : a.t0;
    const long t0 = t0_row < 0 ? 0 : t0_row;
    double run = sb_sum[(size_t)i * a.B + b];
    for (int t = 0; t < a.k; ++t) {
        __syncthreads();  // the frame before is read
        const size_t r = (size_t)t * a.Bp + b;
        for (int f = threadIdx.x; f < a.Fm; f += 256) {
            bins[f] = comp[r * a.FmP + f];
            bins[a.Fm + f] = fb_out[r * ld_fb + f];
        }
        __syncthreads();
        double s = 0.0;
        for (int e = threadIdx.x; e < E; e += 256) s += (double)section_entry(bins, q, a.Fm, e);
        s = block_sum(s, part);
        if (threadIdx.x == 0) {
            run += s;
            den_s = (float)(run / ((double)E * ((double)t0 + t + 1.0))) + kFsnEpsilon;
        }
        __syncthreads();
        const float den = den_s;
        float* x = q.x + ((size_t)t * q.Np + row0) * q.Ip;
        for (int e = threadIdx.x; e < E; e += 256) {
            const int u = e / q.W;
            x[(size_t)u * q.Ip + (e - u * q.W)] = section_entry(bins, q, a.Fm, e) / den;
        }
        for (int e = threadIdx.x; e < q.units * pad; e += 256) {  // the padded columns of this stream's rows
            const int u = e / pad;
            x[(size_t)u * q.Ip + q.W + (e - u * pad)] = 0.f;
        }
        if (b == 0) {  // the padded rows of the section
            float* z = q.x + ((size_t)t * q.Np + (size_t)a.B * q.units) * q.Ip;
            const int n = (q.Np - a.B * q.units) * q.Ip;
            for (int e = threadIdx.x; e < n; e += 256) z[e] = 0.f;
        }
    }
    if (threadIdx.x == 0) sb_sum[(size_t)i * a.B + b] = run;
}

// One thread per (b, component, bin), all k frames.
__global__ __launch_bounds__(256) void improved_stream_mask_kernel(float* __restrict__ mask, const FsnImprovedStream a) {
    const long n = (long)a.B * 2 * a.F;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = (int)(i % a.F), comp = (int)((i / a.F) & 1), b = (int)(i / (2 * a.F));
    float* out = mask + (size_t)i * a.k;
    const float* src = nullptr;
    size_t step = 0;
    for (int j = 0; j < a.n; ++j) {
        const FsnImprovedSection& q = a.s[j];
        if (f < q.lower || f >= q.lower + q.units * q.sc) continue;
        const int u = (f - q.lower) / q.sc, cc = (f - q.lower) - u * q.sc;
        src = q.o + ((size_t)b * q.units + u) * (2 * q.sc) + comp * q.sc + cc;
        step = (size_t)q.Np * 2 * q.sc;
    }
    for (int t = 0; t < a.k; ++t) out[t] = src ? src[(size_t)t * step] : 0.f;  // the last bin: no section covers it
}

// grid (blocks, pairs): pair blockIdx.y, float4 by float4 (every count is a multiple of 16 rows x 64 units)
__global__ __launch_bounds__(256) void improved_stream_keep_kernel(const FsnImprovedKeep a) {
    const int j = blockIdx.y;
    const float4* src = reinterpret_cast<const float4*>(a.src[j]);
    float4* dst = reinterpret_cast<float4*>(a.dst[j]);
    const long n4 = a.count[j] / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace

int fsn_launch_improved_stream_front(const float* mag, float* comp, float* fb_in, double* fb_sum, long* steps,
                                     const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "improved stream front");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(improved_stream_front_kernel, dim3((unsigned)a.Bp), dim3(256), 0, s, mag, comp, fb_in, fb_sum, steps, a);
    return fsn_check_launch("improved_stream_front_kernel");
}

int fsn_launch_improved_stream_sections(const float* comp, const float* fb_out, long ld_fb, double* sb_sum,
                                        const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "improved stream sections");
    if (rc != FSN_OK) return rc;
    if (ld_fb < a.Fm) {
        fsn_set_error("improved stream sections: full-band row stride %ld below the %d bins", ld_fb, a.Fm);
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(improved_stream_sections_kernel, dim3((unsigned)a.B, (unsigned)a.n), dim3(256), 0, s, comp, fb_out, ld_fb,
                       sb_sum, a);
    return fsn_check_launch("improved_stream_sections_kernel");
}

int fsn_launch_improved_stream_mask(float* mask, const FsnImprovedStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "improved stream mask");
    if (rc != FSN_OK) return rc;
    const long n = (long)a.B * 2 * a.F;
    hipLaunchKernelGGL(improved_stream_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mask, a);
    return fsn_check_launch("improved_stream_mask_kernel");
}

int fsn_launch_improved_stream_keep(const FsnImprovedKeep& a, hipStream_t s) {
    bool ok = a.n >= 1 && a.n <= 8;
    long most = 0;
    for (int j = 0; ok && j < a.n; ++j) {
        ok = a.dst[j] && a.src[j] && a.count[j] >= 4 && a.count[j] % 4 == 0 && ((uintptr_t)a.dst[j] | (uintptr_t)a.src[j]) % 16 == 0;
        most = a.count[j] > most ? a.count[j] : most;
    }
    if (!ok) {
        fsn_set_error("improved stream keep: 1 .. 8 pairs of 16-byte aligned arrays, counts multiples of 4");
        return FSN_ERR_ARG;
    }
    const long blocks = (most / 4 + 255) / 256;
    hipLaunchKernelGGL(improved_stream_keep_kernel, dim3((unsigned)(blocks < 64 ? blocks : 64), (unsigned)a.n), dim3(256), 0, s, a);
    return fsn_check_launch("improved_stream_keep_kernel");
}
