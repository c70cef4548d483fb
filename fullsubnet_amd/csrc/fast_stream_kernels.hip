// Fast FullSubNet's glue with carried state (fsn_fast_stream_step, fsn_api_fast_stream.hip): what fast_glue_kernels.hip does
// for a whole utterance, for k more model steps t0 .. t0 + k - 1 of B streams in lockstep.  Tensors are time-major as there
// ([k][Bp][columns]); the three kernels are the stages of the step that read or write the state blob:
//   mel_norm        cumulative_laplace_norm (base_model.py:221-251) of the mel spectrum in front of the encoder: step t is
//                   divided by the running mean of the stream's num_mels (t + 1) values so far; the sum is carried in fp64
//   units           the unit windows of mel and encoder output (reflection at the band edges, the unfolded tensor never
//                   formed), real_time_downsampling (model.py:108-129) as a running block sum that continues from t0's
//                   phase, and the cumulative norm of the low-rate frames: low-rate frame 0 is step 0's unit tensor, frame
//                   j >= 1 the mean over steps (j - 1) s + 1 .. j s, complete at step j s and divided by the running mean
//                   of the row's W (j + 1) values.  Only the frames that complete in this call are written
//   decoder_input   real_time_upsampling (model.py:131-140) and the concatenation: step t takes the bottleneck's output of
//                   low-rate frame t / s - one of this call's, or the one held in the state from an earlier call
// Every sum is formed in an order that depends on the frames alone, never on where a call begins or ends: the block sum is
// added frame by frame in fp32, the norms' sums frame by frame in fp64 from per-frame sums of a fixed shape.  Two chunkings
// of a stream therefore give the same bits.  One workgroup owns a stream's state fields, so no field is read by one
// workgroup and written by another.
#include "fsn_common.h"

namespace {

constexpr int kMels = 64;         // num_mels: one wave of bands (the launchers refuse anything else)
constexpr int kUnitsPerLane = 8;  // window columns per lane: 4 lanes per band, W <= 32
constexpr int kNormFrames = 256;  // frames the mel norm scans per pass
constexpr int kUnitFrames = 16;   // frames the units kernel stages per pass

__device__ __forceinline__ int stream_reflect(int j, int M) {
    j = j < 0 ? -j : j;
    return j > M - 1 ? 2 * (M - 1) - j : j;
}

// One workgroup per (padded) row b.  Waves take the frames of a pass in turn: lane = band, the frame's sum by a butterfly
// (every lane ends with the same fp64 value, whatever its position); thread 0 then continues the running sum frame by frame.
__global__ __launch_bounds__(256) void fast_stream_mel_norm_kernel(const float* __restrict__ mel, float* __restrict__ out,
                                                                   double* __restrict__ mel_sum, const FsnFastStream a) {
    __shared__ double fsum[kNormFrames];
    __shared__ float den[kNormFrames];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (b >= a.B) {  // padding rows: zeros
        for (int t = wave; t < a.k; t += 4) out[((size_t)t * a.Bp + b) * kMels + lane] = 0.f;
        return;
    }
    double run = mel_sum[b];
    for (int c0 = 0; c0 < a.k; c0 += kNormFrames) {
        const int n = a.k - c0 < kNormFrames ? a.k - c0 : kNormFrames;
        for (int t = wave; t < n; t += 4) {
            double v = (double)mel[((size_t)(c0 + t) * a.Bp + b) * kMels + lane];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
            if (lane == 0) fsum[t] = v;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int t = 0; t < n; ++t) {
                run += fsum[t];
                den[t] = (float)(run / ((double)kMels * ((double)a.t0 + c0 + t + 1.0))) + kFsnEpsilon;
            }
        }
        __syncthreads();
        for (int t = wave; t < n; t += 4) {
            const size_t i = ((size_t)(c0 + t) * a.Bp + b) * kMels + lane;
            out[i] = mel[i] / den[t];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) mel_sum[b] = run;
}

// One workgroup per stream b; thread (m, q) = (tid / 4, tid % 4) owns columns w = q, q + 4, .. of band m's window: their
// block sums live in registers for the whole call and go back to `partial` at its end.
__global__ __launch_bounds__(256) void fast_stream_units_kernel(const float* __restrict__ mel, const float* __restrict__ enc,
                                                                long ld_enc, float* __restrict__ partial,
                                                                double* __restrict__ unit_sum, float* __restrict__ units,
                                                                const FsnFastStream a) {
    __shared__ float band[kUnitFrames][2 * kMels];  // a frame's mel bands, then its encoder outputs
    const int b = blockIdx.x, m = threadIdx.x >> 2, q = threadIdx.x & 3;
    const int w_mel = 2 * a.n_mel + 1, W = a.W;
    const size_t row = (size_t)b * kMels + m;
    float part[kUnitsPerLane];
    int src[kUnitsPerLane];
#pragma unroll
    for (int i = 0; i < kUnitsPerLane; ++i) {
        const int w = q + 4 * i;
        part[i] = 0.f;
        src[i] = 0;
        if (w < W) {
            part[i] = partial[row * W + w];
            src[i] = w < w_mel ? stream_reflect(m - a.n_mel + w, kMels) : kMels + stream_reflect(m - a.n_enc + (w - w_mel), kMels);
        }
    }
    double run = unit_sum[row];
    int done = 0;  // low-rate frames this call has completed
    for (int c0 = 0; c0 < a.k; c0 += kUnitFrames) {
        const int n = a.k - c0 < kUnitFrames ? a.k - c0 : kUnitFrames;
        __syncthreads();
        for (int i = threadIdx.x; i < n * 2 * kMels; i += 256) {
            const int t = i / (2 * kMels), c = i % (2 * kMels);
            const size_t r = (size_t)(c0 + t) * a.Bp + b;
            band[t][c] = c < kMels ? mel[r * kMels + c] : enc[r * ld_enc + (c - kMels)];
        }
        __syncthreads();
        for (int t = 0; t < n; ++t) {
            const long step = (long)a.t0 + c0 + t;
#pragma unroll
            for (int i = 0; i < kUnitsPerLane; ++i) part[i] += band[t][src[i]];  // frame order: 0 + u is u
            if (step % a.shrink != 0) continue;                                  // (the same for the whole workgroup)
            // the block is whole: step 0 is its own frame, a later one the mean of `shrink` steps
            const bool mean = step > 0 && a.shrink > 1;
            float v[kUnitsPerLane];
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < kUnitsPerLane; ++i) {
                v[i] = mean ? part[i] / (float)a.shrink : part[i];
                if (q + 4 * i < W) s += (double)v[i];
                part[i] = 0.f;
            }
            s += __shfl_xor(s, 1, 64);  // the four lanes of a band: (s0 + s1) + (s2 + s3) in each of them
            s += __shfl_xor(s, 2, 64);
            run += s;
            const float den = (float)(run / ((double)W * ((double)(step / a.shrink) + 1.0))) + kFsnEpsilon;
            float* o = units + ((size_t)done * a.Np + row) * a.Wp;
#pragma unroll
            for (int i = 0; i < kUnitsPerLane; ++i)
                if (q + 4 * i < W) o[q + 4 * i] = v[i] / den;
            for (int w = W + q; w < a.Wp; w += 4) o[w] = 0.f;
            ++done;
        }
    }
#pragma unroll
    for (int i = 0; i < kUnitsPerLane; ++i)
        if (q + 4 * i < W) partial[row * W + q + 4 * i] = part[i];
    if (q == 0) unit_sum[row] = run;
}

// One thread per (row b, column c) of the decoder's input, all k steps: the thread of (b, M + m) is the only one that reads
// or writes held[b][m].
__global__ __launch_bounds__(256) void fast_stream_decoder_input_kernel(const float* __restrict__ enc, long ld_enc,
                                                                        const float* __restrict__ slow, float* __restrict__ held,
                                                                        float* __restrict__ out, const FsnFastStream a) {
    const long per_t = (long)a.Bp * 2 * kMels;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_t) return;
    const int b = (int)(i / (2 * kMels)), c = (int)(i % (2 * kMels));
    if (b >= a.B) {
        for (int t = 0; t < a.k; ++t) out[(size_t)t * per_t + i] = 0.f;
        return;
    }
    if (c < kMels) {
        for (int t = 0; t < a.k; ++t) out[(size_t)t * per_t + i] = enc[((size_t)t * a.Bp + b) * ld_enc + c];
        return;
    }
    const size_t row = (size_t)b * kMels + (c - kMels);
    const float carried = held[row];
    const long j0 = ((long)a.t0 + a.shrink - 1) / a.shrink;  // the first low-rate frame that completes in this call
    for (int t = 0; t < a.k; ++t) {
        const long j = ((long)a.t0 + t) / a.shrink - j0;  // < n_low: frame j0 + j completed at step (j0 + j) shrink <= t0 + t
        out[(size_t)t * per_t + i] = j >= 0 ? slow[(size_t)j * a.Np + row] : carried;
    }
    if (a.n_low > 0) held[row] = slow[(size_t)(a.n_low - 1) * a.Np + row];
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

int fsn_launch_fast_stream_mel_norm(const float* mel, float* out, double* mel_sum, const FsnFastStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast stream mel norm");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(fast_stream_mel_norm_kernel, dim3((unsigned)a.Bp), dim3(256), 0, s, mel, out, mel_sum, a);
    return fsn_check_launch("fast_stream_mel_norm_kernel");
}

int fsn_launch_fast_stream_units(const float* mel, const float* enc, long ld_enc, float* partial, double* unit_sum,
                                 float* units, const FsnFastStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast stream units");
    if (rc != FSN_OK) return rc;
    if (ld_enc < kMels) {
        fsn_set_error("fast stream units: encoder row stride %ld below 64", ld_enc);
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(fast_stream_units_kernel, dim3((unsigned)a.B), dim3(256), 0, s, mel, enc, ld_enc, partial, unit_sum, units,
                       a);
    return fsn_check_launch("fast_stream_units_kernel");
}

int fsn_launch_fast_stream_decoder_input(const float* enc, long ld_enc, const float* slow, float* held, float* out,
                                         const FsnFastStream& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast stream decoder input");
    if (rc != FSN_OK) return rc;
    if (ld_enc < kMels) {
        fsn_set_error("fast stream decoder input: encoder row stride %ld below 64", ld_enc);
        return FSN_ERR_ARG;
    }
    const long per_t = (long)a.Bp * 2 * kMels;
    hipLaunchKernelGGL(fast_stream_decoder_input_kernel, dim3((unsigned)((per_t + 255) / 256)), dim3(256), 0, s, enc, ld_enc, slow,
                       held, out, a);
    return fsn_check_launch("fast_stream_decoder_input_kernel");
}
