// Fast FullSubNet's glue for recordings of any length under the offline norm (fsn_fast_segment_*, fsn_api_fast_stream.hip):
// what fast_stream_kernels.hip does under the causal norm, for the model in segments of k steps t0 .. t0 + k - 1.
// offline_laplace_norm (base_model.py:204-218) divides by ONE mean per utterance and the model applies it twice
// (model.py:170,187), so the means are gathered in passes of their own; the kernels here are the stages that read or write
// the two fp64 accumulators of the state blob:
//   mel_stat        pass 1: every frame's 64-band sum (the butterfly of fast_stream_mel_norm_kernel) joins acc_mel[b]
//   mel_norm        pass 2: mel / den_mel[b], one divisor per row from the finished sum and the row's own step count
//   units<false>    pass 2, the statistic form: the unit windows and the running block sum of fast_stream_units_kernel on a
//                   block-sum field of its own; every low-rate frame that completes at a step t < total[b] - and the closing
//                   short block at step total[b] - 1, which real_time_downsampling averages over the frames it has
//                   (model.py:117-127) - adds the fp64 sum of its 64 W fp32 values to acc_unit[b].  Nothing is written out
//   units<true>     pass 3, the emit form: the low-rate frames of whole blocks that complete in the segment, divided by
//                   den_unit[b]; the closing short block feeds nothing (up-sampling never reads it)
//   divisors        both divisors as the passes form them
// Every sum is formed in an order that depends on the frames alone: a frame's sum has a fixed shape, the frames join the
// accumulator in frame order.  Two segmentations of a recording therefore give the same bits.  One workgroup owns a row's
// state fields.  total[b] = T_b + look_ahead is the row's own step count (device memory); a row of a ragged batch runs on
// to the longest row's end and adds nothing to its sums from its step total[b] on.
#include "fsn_common.h"

namespace {

constexpr int kMels = 64;           // num_mels: one wave of bands (the launchers refuse anything else)
constexpr int kUnitsPerLane = 8;    // window columns per lane: 4 lanes per band, W <= 32
constexpr int kStatFrames = 256;    // frames the mel statistic scans per pass
constexpr int kUnitFrames = 16;     // frames the units kernel stages per pass
constexpr float kOfflineEps = 1e-5f;  // offline_laplace_norm's epsilon

__device__ __forceinline__ int segment_reflect(int j, int M) {
    j = j < 0 ? -j : j;
    return j > M - 1 ? 2 * (M - 1) - j : j;
}
__device__ __forceinline__ int segment_total(const int* total, int b) {  // never below one step: no count is zero
    const int t = total[b];
    return t < 1 ? 1 : t;
}
// float(sum / count) + 1e-5f, the reference's fp32 operations on the exactly carried sum
__device__ __forceinline__ float segment_den_mel(double sum, int total) {
    return (float)(sum / ((double)kMels * (double)total)) + kOfflineEps;
}
__device__ __forceinline__ float segment_den_unit(double sum, int total, int shrink, int W) {
    const int Ts = 1 + (total - 1 + shrink - 1) / shrink;  // real_time_downsampling's frame count, the closing block included
    return (float)(sum / ((double)kMels * (double)W * (double)Ts)) + kOfflineEps;
}

// One workgroup per row b.  Waves take the frames of a pass in turn: lane = band, the frame's sum by a butterfly (every
// lane ends with the same fp64 value); thread 0 then continues the accumulator frame by frame.
__global__ __launch_bounds__(256) void fast_segment_mel_stat_kernel(const float* __restrict__ mel, double* __restrict__ acc_mel,
                                                                    const FsnFastStream a) {
    __shared__ double fsum[kStatFrames];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double run = acc_mel[b];
    for (int c0 = 0; c0 < a.k; c0 += kStatFrames) {
        const int n = a.k - c0 < kStatFrames ? a.k - c0 : kStatFrames;
        __syncthreads();
        for (int t = wave; t < n; t += 4) {
            double v = (double)mel[((size_t)(c0 + t) * a.Bp + b) * kMels + lane];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
            if (lane == 0) fsum[t] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int t = 0; t < n; ++t) run += fsum[t];
    }
    if (threadIdx.x == 0) acc_mel[b] = run;
}

// out = mel / den_mel[b], rows beyond B zero
__global__ __launch_bounds__(256) void fast_segment_mel_norm_kernel(const float* __restrict__ mel, float* __restrict__ out,
                                                                    const double* __restrict__ acc_mel,
                                                                    const int* __restrict__ total, long n, const FsnFastStream a) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int b = (int)((i / kMels) % a.Bp);
    out[i] = b < a.B ? mel[i] / segment_den_mel(acc_mel[b], segment_total(total, b)) : 0.f;
}

// One workgroup per row b; thread (m, q) = (tid / 4, tid % 4) owns columns w = q, q + 4, .. of band m's window, as in
// fast_stream_units_kernel: their block sums live in registers for the whole call and go back to `partial` at its end.
// kEmit false: `acc_unit` is continued, `units` is not touched.  kEmit true: `acc_unit` is read, `units` is written.
template <bool kEmit>
__global__ __launch_bounds__(256) void fast_segment_units_kernel(const float* __restrict__ mel, const float* __restrict__ enc,
                                                                 long ld_enc, float* __restrict__ partial,
                                                                 double* __restrict__ acc_unit, const int* __restrict__ total,
                                                                 float* __restrict__ units, const FsnFastStream a) {
    __shared__ float band[kUnitFrames][2 * kMels];  // a frame's mel bands, then its encoder outputs
    __shared__ double wsum[kUnitFrames][4];         // the low-rate frames of a pass: one sum per wave
    const int b = blockIdx.x, m = threadIdx.x >> 2, q = threadIdx.x & 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w_mel = 2 * a.n_mel + 1, W = a.W;
    const size_t row = (size_t)b * kMels + m;
    const int tot = segment_total(total, b);
    float part[kUnitsPerLane];
    int src[kUnitsPerLane];
#pragma unroll
    for (int i = 0; i < kUnitsPerLane; ++i) {
        const int w = q + 4 * i;
        part[i] = 0.f;
        src[i] = 0;
        if (w < W) {
            part[i] = partial[row * W + w];
            src[i] = w < w_mel ? segment_reflect(m - a.n_mel + w, kMels) : kMels + segment_reflect(m - a.n_enc + (w - w_mel), kMels);
        }
    }
    double run = kEmit ? 0.0 : acc_unit[b];
    const float den = kEmit ? segment_den_unit(acc_unit[b], tot, a.shrink, W) : 1.f;
    int done = 0;  // low-rate frames this call has completed (emit form)
    for (int c0 = 0; c0 < a.k; c0 += kUnitFrames) {
        const int n = a.k - c0 < kUnitFrames ? a.k - c0 : kUnitFrames;
        __syncthreads();
        for (int i = threadIdx.x; i < n * 2 * kMels; i += 256) {
            const int t = i / (2 * kMels), c = i % (2 * kMels);
            const size_t r = (size_t)(c0 + t) * a.Bp + b;
            band[t][c] = c < kMels ? mel[r * kMels + c] : enc[r * ld_enc + (c - kMels)];
        }
        __syncthreads();
        int summed = 0;  // low-rate frames of this pass that join the sum (statistic form)
        for (int t = 0; t < n; ++t) {
            const long step = (long)a.t0 + c0 + t;
            if (!kEmit && step >= tot) break;  // past the row's end: nothing more joins its sum (the same for the whole workgroup)
#pragma unroll
            for (int i = 0; i < kUnitsPerLane; ++i) part[i] += band[t][src[i]];  // frame order: 0 + u is u
            const bool whole = step % a.shrink == 0;
            // the closing block of the row, shorter than `shrink`: it counts in the mean and feeds nothing
            const bool closing = !kEmit && !whole && step == (long)tot - 1;
            if (!whole && !closing) continue;
            // a whole block: step 0 is its own frame, a later one the mean of `shrink` steps; the closing one of what it has
            const int frames = closing ? (int)(step % a.shrink) : (step > 0 ? a.shrink : 1);
            float v[kUnitsPerLane];
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < kUnitsPerLane; ++i) {
                v[i] = frames > 1 ? part[i] / (float)frames : part[i];
                if (q + 4 * i < W) s += (double)v[i];
                part[i] = 0.f;
            }
            if (kEmit) {
                float* o = units + ((size_t)done * a.Np + row) * a.Wp;
#pragma unroll
                for (int i = 0; i < kUnitsPerLane; ++i)
                    if (q + 4 * i < W) o[q + 4 * i] = v[i] / den;
                for (int w = W + q; w < a.Wp; w += 4) o[w] = 0.f;
                ++done;
            } else {
#pragma unroll
                for (int mm = 32; mm >= 1; mm >>= 1) s += __shfl_xor(s, mm, 64);
                if (lane == 0) wsum[summed][wave] = s;
                ++summed;
            }
        }
        if (!kEmit) {
            __syncthreads();
            for (int j = 0; j < summed; ++j) run += ((wsum[j][0] + wsum[j][1]) + wsum[j][2]) + wsum[j][3];  // in every thread alike
        }
    }
#pragma unroll
    for (int i = 0; i < kUnitsPerLane; ++i)
        if (q + 4 * i < W) partial[row * W + q + 4 * i] = part[i];
    if (!kEmit && threadIdx.x == 0) acc_unit[b] = run;
}

__global__ __launch_bounds__(256) void fast_segment_divisors_kernel(const double* __restrict__ acc_mel,
                                                                    const double* __restrict__ acc_unit,
                                                                    const int* __restrict__ total, float* __restrict__ den_mel,
                                                                    float* __restrict__ den_unit, int B, int shrink, int W) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int tot = segment_total(total, b);
    den_mel[b] = segment_den_mel(acc_mel[b], tot);
    den_unit[b] = segment_den_unit(acc_unit[b], tot, shrink, W);
}

int check_geometry(const FsnFastStream& a, const char* what) {
    if (a.M != kMels || a.B < 1 || a.Bp < a.B || a.k < 1 || a.t0 < 0 || a.shrink < 1 || a.n_mel < 0 || a.n_enc < 0 ||
        a.W != 2 * a.n_mel + 1 + 2 * a.n_enc + 1 || a.W > 4 * kUnitsPerLane || a.Wp < a.W || (long)a.Np < (long)a.B * kMels ||
        a.n_low != fsn_fast_stream_low_frames(a.t0, a.k, a.shrink)) {
        fsn_set_error("%s: geometry outside the kernel (64 bands, unit width <= 32, padded sizes not below the sizes)", what);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

}  // namespace

int fsn_launch_fast_segment_mel_stat(const float* mel, double* acc_mel, const FsnFastStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast segment mel statistic");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(fast_segment_mel_stat_kernel, dim3((unsigned)a.B), dim3(256), 0, s, mel, acc_mel, a);
    return fsn_check_launch("fast_segment_mel_stat_kernel");
}

int fsn_launch_fast_segment_mel_norm(const float* mel, float* out, const double* acc_mel, const int* total, const FsnFastStream& a,
                                     hipStream_t s) {
    const int rc = check_geometry(a, "fast segment mel norm");
    if (rc != FSN_OK) return rc;
    const long n = (long)a.k * a.Bp * kMels;
    hipLaunchKernelGGL(fast_segment_mel_norm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mel, out, acc_mel, total, n,
                       a);
    return fsn_check_launch("fast_segment_mel_norm_kernel");
}

int fsn_launch_fast_segment_units(bool emit, const float* mel, const float* enc, long ld_enc, float* partial, double* acc_unit,
                                  const int* total, float* units, const FsnFastStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast segment units");
    if (rc != FSN_OK) return rc;
    if (ld_enc < kMels || (emit && !units)) {
        fsn_set_error("fast segment units: encoder row stride %ld below 64, or the emit form without an output", ld_enc);
        return FSN_ERR_ARG;
    }
    if (emit)
        hipLaunchKernelGGL(fast_segment_units_kernel<true>, dim3((unsigned)a.B), dim3(256), 0, s, mel, enc, ld_enc, partial, acc_unit,
                           total, units, a);
    else
        hipLaunchKernelGGL(fast_segment_units_kernel<false>, dim3((unsigned)a.B), dim3(256), 0, s, mel, enc, ld_enc, partial,
                           acc_unit, total, units, a);
    return fsn_check_launch("fast_segment_units_kernel");
}

int fsn_launch_fast_segment_divisors(const double* acc_mel, const double* acc_unit, const int* total, float* den_mel,
                                     float* den_unit, int B, int shrink, int W, hipStream_t s) {
    if (B < 1 || shrink < 1 || W < 2) {
        fsn_set_error("fast segment divisors: need B, shrink >= 1 and a unit width >= 2");
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(fast_segment_divisors_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, acc_mel, acc_unit, total,
                       den_mel, den_unit, B, shrink, W);
    return fsn_check_launch("fast_segment_divisors_kernel");
}
