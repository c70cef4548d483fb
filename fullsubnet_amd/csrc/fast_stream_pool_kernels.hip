// Streaming pool for Fast FullSubNet (fsn_fast_stream_pool_*): the model step of fsn_fast_stream_step over a SUBSET of the
// slots of a pool whose sessions open, advance and close on their own - and therefore stand at different phases of a
// down-sampling block.
//
// The pool's state is one record per slot (FsnFastPoolLayout, fsn_common.h).  A step (fsn_api_fast_stream.hip)
//   1. checks the caller's order: the slots that complete hi = ceil(k / shrink) low-rate frames from their own count must be
//      rows [0, n_long) of the list, the ones that complete lo = k / shrink the rest (fast_pool_check_kernel),
//   2. gathers the listed slots' (h, c) rows into compact tiles (pad rows and rows of an id outside the pool are zeros, so
//      every row the recurrent kernels touch is finite),
//   3. runs the lockstep entry's sequence on the compact rows.  The three stages that touch the norms' sums, the open block
//      and the held output are the kernels of fast_stream_kernels.hip with t0 and the state taken from each row's record -
//      every formula, sum order and fp64 / fp32 choice is that file's, restated here line by line - and the bottleneck runs
//      lo steps on all rows, then one more on the rows of the first n_long slots, a prefix of the same tiles,
//   4. scatters the rows back and advances the listed slots' step counts.
// Slots that are not listed are never written.  One workgroup (or thread) owns a record's field in every kernel; all copies
// move 16 bytes per lane, coalesced along H.  When the order check fails no kernel here writes a record.
#include "fsn_common.h"

namespace {

constexpr int kMels = 64;         // num_mels: one wave of bands (the entry refuses anything else)
constexpr int kUnitsPerLane = 8;  // window columns per lane: 4 lanes per band, W <= 32
constexpr int kNormFrames = 256;  // frames the mel norm scans per pass
constexpr int kUnitFrames = 16;   // frames the units kernel stages per pass

// the record of slots[i], or NULL for i >= n or an id outside the pool (such a row is skipped by every kernel)
__device__ __forceinline__ char* record_of(const FsnFastPool& a, int i) {
    if (i >= a.n) return nullptr;
    const int slot = a.slots[i];
    return (slot >= 0 && slot < a.capacity) ? a.state + (size_t)slot * a.L.slot_bytes : nullptr;
}
__device__ __forceinline__ int steps_of(const FsnFastPool& a, const char* rec) {
    return *reinterpret_cast<const int*>(rec + a.L.steps);
}
// multiples of shrink in [t0, t0 + k) (fsn_fast_stream_low_frames, in 64 bits)
__device__ __forceinline__ int low_frames(long t0, int k, int shrink) {
    return (int)((t0 + k - 1) / shrink - (t0 > 0 ? (t0 - 1) / shrink : -1));
}
__device__ __forceinline__ int pool_reflect(int j, int M) {
    j = j < 0 ? -j : j;
    return j > M - 1 ? 2 * (M - 1) - j : j;
}

// ---- the caller's order ----------------------------------------------------------------------------------------------------
// One workgroup.  *status becomes 0, or 1 when a listed, valid slot stands on the wrong side of n_long (or its count would
// pass 2^31 - 1).
__global__ __launch_bounds__(256) void fast_pool_check_kernel(const FsnFastPool a) {
    int bad = 0;
    for (int i = threadIdx.x; i < a.n; i += 256) {
        const char* rec = record_of(a, i);
        if (!rec) continue;
        const int t0 = steps_of(a, rec);
        if (t0 < 0 || (long)t0 + a.k > 2147483647L) {
            bad = 1;
            continue;
        }
        const bool is_long = low_frames(t0, a.k, a.shrink) == a.hi;
        bad |= is_long != (i < a.n_long);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) *a.status = bad ? 1u : 0u;
}

// ---- (h, c) rows of the listed slots <-> compact tiles ---------------------------------------------------------------------
// Encoder and decoder layers: one row per slot.  blockIdx.y is the array (2 layer + h | c); a thread moves one f32x4 of the
// widest layer's row (512 floats), the narrower ones leave their surplus threads idle.  Gather fills all Bp rows; scatter
// writes the listed, valid ones and advances the slot's step count by k (the last kernel of a step: nothing reads the
// count after it).
template <bool SCATTER>
__global__ __launch_bounds__(256) void fast_pool_pairs_kernel(const FsnFastPool a, const FsnFastPoolTiles t) {
    const int arr = blockIdx.y, H4 = fsn_fast_pair_h(arr / 2) / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(idx / 128), c4 = (int)(idx % 128);
    if (row >= a.Bp || c4 >= H4) return;
    if (SCATTER && *a.status != 0u) return;
    char* rec = record_of(a, row);
    f32x4* tile = reinterpret_cast<f32x4*>(t.pair[arr]) + (size_t)row * H4 + c4;
    if (SCATTER) {
        if (!rec) return;
        *(reinterpret_cast<f32x4*>(rec + a.L.pair[arr]) + c4) = *tile;
        if (arr == 0 && c4 == 0) *reinterpret_cast<int*>(rec + a.L.steps) += a.k;
    } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rec) v = *(reinterpret_cast<const f32x4*>(rec + a.L.pair[arr]) + c4);
        *tile = v;
    }
}

// Bottleneck layers: 64 rows per slot, the first slots_run listed slots.  blockIdx.y is the array (2 layer + h | c).
template <bool SCATTER>
__global__ __launch_bounds__(256) void fast_pool_bn_kernel(const FsnFastPool a, const FsnFastPoolTiles t, int slots_run) {
    const int arr = blockIdx.y, H4 = a.L.H / 4;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long row = idx / H4;
    const int c4 = (int)(idx % H4);
    if (row >= (long)slots_run * kMels) return;
    if (SCATTER && *a.status != 0u) return;
    const int i = (int)(row / kMels), m = (int)(row % kMels);
    char* rec = record_of(a, i);
    f32x4* tile = reinterpret_cast<f32x4*>(t.bn[arr / 2][arr % 2]) + (size_t)row * H4 + c4;
    if (SCATTER) {
        if (rec) *(reinterpret_cast<f32x4*>(rec + a.L.bn[arr / 2][arr % 2]) + (size_t)m * H4 + c4) = *tile;
    } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rec) v = *(reinterpret_cast<const f32x4*>(rec + a.L.bn[arr / 2][arr % 2]) + (size_t)m * H4 + c4);
        *tile = v;
    }
}

// ---- fast_stream_mel_norm_kernel per slot ----------------------------------------------------------------------------------
// One workgroup per (padded) row b; a pad row and a skipped row give zeros.
__global__ __launch_bounds__(256) void fast_pool_mel_norm_kernel(const float* __restrict__ mel, float* __restrict__ out,
                                                                 const FsnFastPool a) {
    __shared__ double fsum[kNormFrames];
    __shared__ float den[kNormFrames];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* rec = *a.status == 0u ? record_of(a, b) : nullptr;  // uniform over the workgroup
    if (!rec) {
        for (int t = wave; t < a.k; t += 4) out[((size_t)t * a.Bp + b) * kMels + lane] = 0.f;
        return;
    }
    double* mel_sum = reinterpret_cast<double*>(rec + a.L.mel_sum);
    const int t0 = steps_of(a, rec);
    double run = *mel_sum;
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
                den[t] = (float)(run / ((double)kMels * ((double)t0 + c0 + t + 1.0))) + kFsnEpsilon;
            }
        }
        __syncthreads();
        for (int t = wave; t < n; t += 4) {
            const size_t i = ((size_t)(c0 + t) * a.Bp + b) * kMels + lane;
            out[i] = mel[i] / den[t];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *mel_sum = run;
}

// ---- fast_stream_units_kernel per slot -------------------------------------------------------------------------------------
// One workgroup per listed row b; thread (m, q) = (tid / 4, tid % 4) owns columns w = q, q + 4, .. of band m's window.  The
// frames the slot completes go to ordinals 0 .. of units [ordinal][Np][Wp]: lo of them, or hi for b < n_long (the order
// check's guarantee; the host sized `units` for hi ordinals of all rows).  A skipped row's unit rows are zeros.
__global__ __launch_bounds__(256) void fast_pool_units_kernel(const float* __restrict__ mel, const float* __restrict__ enc,
                                                              long ld_enc, float* __restrict__ units, const FsnFastPool a) {
    __shared__ float band[kUnitFrames][2 * kMels];  // a frame's mel bands, then its encoder outputs
    const int b = blockIdx.x, m = threadIdx.x >> 2, q = threadIdx.x & 3;
    const int w_mel = 2 * a.n_mel + 1, W = a.W;
    const size_t row = (size_t)b * kMels + m;
    if (*a.status != 0u) return;
    char* rec = record_of(a, b);  // uniform over the workgroup
    if (!rec) {
        const int ords = a.lo + (b < a.n_long && a.hi > a.lo ? 1 : 0);
        for (int j = 0; j < ords; ++j)
            for (int w = q; w < a.Wp; w += 4) units[((size_t)j * a.Np + row) * a.Wp + w] = 0.f;
        return;
    }
    float* partial = reinterpret_cast<float*>(rec + a.L.partial) + (size_t)m * W;
    double* unit_sum = reinterpret_cast<double*>(rec + a.L.unit_sum) + m;
    const int t0 = steps_of(a, rec);
    float part[kUnitsPerLane];
    int src[kUnitsPerLane];
#pragma unroll
    for (int i = 0; i < kUnitsPerLane; ++i) {
        const int w = q + 4 * i;
        part[i] = 0.f;
        src[i] = 0;
        if (w < W) {
            part[i] = partial[w];
            src[i] = w < w_mel ? pool_reflect(m - a.n_mel + w, kMels) : kMels + pool_reflect(m - a.n_enc + (w - w_mel), kMels);
        }
    }
    double run = *unit_sum;
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
            const long step = (long)t0 + c0 + t;
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
        if (q + 4 * i < W) partial[q + 4 * i] = part[i];
    if (q == 0) *unit_sum = run;
}

// ---- fast_stream_decoder_input_kernel per slot -----------------------------------------------------------------------------
// One thread per (row b, column c) of the decoder's input, all k steps: the thread of (b, M + m) is the only one that reads
// or writes the record's held[m].  A pad row and a skipped row give zeros.
__global__ __launch_bounds__(256) void fast_pool_decoder_input_kernel(const float* __restrict__ enc, long ld_enc,
                                                                      const float* __restrict__ slow, float* __restrict__ out,
                                                                      const FsnFastPool a) {
    const long per_t = (long)a.Bp * 2 * kMels;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= per_t) return;
    const int b = (int)(i / (2 * kMels)), c = (int)(i % (2 * kMels));
    char* rec = *a.status == 0u ? record_of(a, b) : nullptr;
    if (!rec) {
        for (int t = 0; t < a.k; ++t) out[(size_t)t * per_t + i] = 0.f;
        return;
    }
    if (c < kMels) {
        for (int t = 0; t < a.k; ++t) out[(size_t)t * per_t + i] = enc[((size_t)t * a.Bp + b) * ld_enc + c];
        return;
    }
    const size_t row = (size_t)b * kMels + (c - kMels);
    float* held = reinterpret_cast<float*>(rec + a.L.held) + (c - kMels);
    const int t0 = steps_of(a, rec);
    const int n_low = low_frames(t0, a.k, a.shrink);
    const float carried = *held;
    const long j0 = ((long)t0 + a.shrink - 1) / a.shrink;  // the first low-rate frame that completes in this call
    for (int t = 0; t < a.k; ++t) {
        const long j = ((long)t0 + t) / a.shrink - j0;  // < n_low: frame j0 + j completed at step (j0 + j) shrink <= t0 + t
        out[(size_t)t * per_t + i] = j >= 0 ? slow[(size_t)j * a.Np + row] : carried;
    }
    if (n_low > 0) *held = slow[(size_t)(n_low - 1) * a.Np + row];
}

int check_geometry(const FsnFastPool& a, const char* what) {
    if (!a.state || !a.slots || !a.status || a.capacity < 1 || a.n < 1 || a.n > a.capacity || a.n_long < 0 || a.n_long > a.n ||
        a.k < 1 || a.Bp < a.n || a.Bp % 16 || a.Np != a.n * kMels || a.shrink < 1 || a.n_mel < 0 || a.n_enc < 0 ||
        a.W != 2 * a.n_mel + 1 + 2 * a.n_enc + 1 || a.W != a.L.W || a.W > 4 * kUnitsPerLane || a.Wp < a.W ||
        a.lo != a.k / a.shrink || a.hi != (a.k + a.shrink - 1) / a.shrink || (a.hi == a.lo && a.n_long != a.n) ||
        a.L.H % 4 || a.L.layers < 1 || a.L.layers > 2) {
        fsn_set_error("%s: geometry outside the kernel (64 bands, unit width <= 32, n_long within n, padded sizes not below the sizes)",
                      what);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

}  // namespace

int fsn_launch_fast_pool_check(const FsnFastPool& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast pool order check");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(fast_pool_check_kernel, dim3(1), dim3(256), 0, s, a);
    return fsn_check_launch("fast_pool_check_kernel");
}

static int pool_pairs(bool scatter, const FsnFastPool& a, const FsnFastPoolTiles& t, hipStream_t s) {
    const int rc = check_geometry(a, "fast pool rows");
    if (rc != FSN_OK) return rc;
    const dim3 grid((unsigned)(((long)a.Bp * 128 + 255) / 256), 8);
    if (scatter)
        hipLaunchKernelGGL(fast_pool_pairs_kernel<true>, grid, dim3(256), 0, s, a, t);
    else
        hipLaunchKernelGGL(fast_pool_pairs_kernel<false>, grid, dim3(256), 0, s, a, t);
    return fsn_check_launch("fast_pool_pairs_kernel");
}
int fsn_launch_fast_pool_gather_pairs(const FsnFastPool& a, const FsnFastPoolTiles& t, hipStream_t s) {
    return pool_pairs(false, a, t, s);
}
int fsn_launch_fast_pool_scatter_pairs(const FsnFastPool& a, const FsnFastPoolTiles& t, hipStream_t s) {
    return pool_pairs(true, a, t, s);
}

static int pool_bn(bool scatter, const FsnFastPool& a, const FsnFastPoolTiles& t, int slots_run, hipStream_t s) {
    const int rc = check_geometry(a, "fast pool bottleneck rows");
    if (rc != FSN_OK) return rc;
    if (slots_run < 1 || slots_run > a.n) {
        fsn_set_error("fast pool bottleneck rows: %d slots of %d", slots_run, a.n);
        return FSN_ERR_ARG;
    }
    const long threads = (long)slots_run * kMels * (a.L.H / 4);
    const dim3 grid((unsigned)((threads + 255) / 256), 2 * a.L.layers);
    if (scatter)
        hipLaunchKernelGGL(fast_pool_bn_kernel<true>, grid, dim3(256), 0, s, a, t, slots_run);
    else
        hipLaunchKernelGGL(fast_pool_bn_kernel<false>, grid, dim3(256), 0, s, a, t, slots_run);
    return fsn_check_launch("fast_pool_bn_kernel");
}
int fsn_launch_fast_pool_gather_bn(const FsnFastPool& a, const FsnFastPoolTiles& t, int slots_run, hipStream_t s) {
    return pool_bn(false, a, t, slots_run, s);
}
int fsn_launch_fast_pool_scatter_bn(const FsnFastPool& a, const FsnFastPoolTiles& t, int slots_run, hipStream_t s) {
    return pool_bn(true, a, t, slots_run, s);
}

int fsn_launch_fast_pool_mel_norm(const float* mel, float* out, const FsnFastPool& a, hipStream_t s) {
    const int rc = check_geometry(a, "fast pool mel norm");
    if (rc != FSN_OK) return rc;
    hipLaunchKernelGGL(fast_pool_mel_norm_kernel, dim3((unsigned)a.Bp), dim3(256), 0, s, mel, out, a);
    return fsn_check_launch("fast_pool_mel_norm_kernel");
}

int fsn_launch_fast_pool_units(const float* mel, const float* enc, long ld_enc, float* units, const FsnFastPool& a,
                               hipStream_t s) {
    const int rc = check_geometry(a, "fast pool units");
    if (rc != FSN_OK) return rc;
    if (ld_enc < kMels) {
        fsn_set_error("fast pool units: encoder row stride %ld below 64", ld_enc);
        return FSN_ERR_ARG;
    }
    hipLaunchKernelGGL(fast_pool_units_kernel, dim3((unsigned)a.n), dim3(256), 0, s, mel, enc, ld_enc, units, a);
    return fsn_check_launch("fast_pool_units_kernel");
}

int fsn_launch_fast_pool_decoder_input(const float* enc, long ld_enc, const float* slow, float* out, const FsnFastPool& a,
                                       hipStream_t s) {
    const int rc = check_geometry(a, "fast pool decoder input");
    if (rc != FSN_OK) return rc;
    if (ld_enc < kMels) {
        fsn_set_error("fast pool decoder input: encoder row stride %ld below 64", ld_enc);
        return FSN_ERR_ARG;
    }
    const long per_t = (long)a.Bp * 2 * kMels;
    hipLaunchKernelGGL(fast_pool_decoder_input_kernel, dim3((unsigned)((per_t + 255) / 256)), dim3(256), 0, s, enc, ld_enc, slow, out,
                       a);
    return fsn_check_launch("fast_pool_decoder_input_kernel");
}
