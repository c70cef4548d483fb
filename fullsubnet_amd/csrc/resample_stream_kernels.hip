// The streaming form of the resampler (fsn_resample_stream_*, include/fsn_hip.h): sessions that receive their input chunk
// by chunk and whose outputs are, bit for bit, those of fsn_resample on the whole utterance.  DESIGN 9d pins it.
//
//   resample_stream_kernel        grid (tiles, n): workgroup (g, i) takes outputs k0 + g tile .. of item i, one per thread,
//                                 stages the inputs under them in LDS - from the slot's history, from the chunk, zeros
//                                 before the session's start and behind the chunk - and, when it is worth staging, the
//                                 polyphase table; zeros behind the item's count up to O_max.  Workgroup (0, i) also
//                                 leaves the session's new history behind                                        -> y, state
//   resample_stream_reset_kernel  grid (n): zeroes the listed slots
//
// Output k has phase (k d + H) mod u and newest input q = (k d + H) / u; its sum runs over poly[phase][j] x[q - j],
// j = 0 .. J - 1, an fp64 fma chain from 0.0 in that order, one rounding to fp32 at the store: the loop of resample_kernel
// (resample_kernels.hip), duplicated here so that the offline kernel is left alone.  The table is the one
// resample_taps_kernel forms, so the products are the same numbers.
//
// A slot is two history buffers of J - 1 samples.  Buffer `parity` holds the session's last J - 1 samples before this
// chunk (all zeros: a fresh session, x[m] = 0 for m < 0) and is only read; the other buffer receives the last J - 1
// samples after it.  No workgroup reads what another writes in the same launch: no flags, no atomics.  Everything an item
// says is clamped on the device (slot, chunk length, count), since the host cannot read the table.
#include "fsn_common.h"

namespace {

constexpr int kThreads = kFsnResampleStreamThreads;

// x[m] of a session: its history below n_before, the chunk from there, zeros outside both
__device__ __forceinline__ float stream_sample(long m, long n_before, int n_chunk, int hist, const float* __restrict__ old,
                                               const float* __restrict__ chunk) {
    if (m >= n_before) return m - n_before < n_chunk ? chunk[m - n_before] : 0.f;
    const long back = n_before - m;  // 1: the newest sample of the history
    return back <= hist ? old[hist - back] : 0.f;
}

// Dynamic LDS: [u][Js] doubles when TAPS_LDS, then p.stretch floats.
template <bool TAPS_LDS>
__global__ __launch_bounds__(kThreads) void resample_stream_kernel(FsnResampleStreamPlan p, const double* __restrict__ poly,
                                                                   float* __restrict__ slots, int capacity,
                                                                   const fsn_resample_stream_item* __restrict__ items,
                                                                   const float* __restrict__ x, int C_max,
                                                                   float* __restrict__ y, int O_max) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    float* xs = reinterpret_cast<float*>(lds + (TAPS_LDS ? (size_t)p.u * p.Js : 0));
    const int i = blockIdx.y;
    const fsn_resample_stream_item it = items[i];
    constexpr long long kMaxPosition = 1ll << 40;  // a position times u or d (<= 4096) stays far inside 64 bits
    const bool listed = it.slot >= 0 && it.slot < capacity && it.n_before >= 0 && it.n_before < kMaxPosition && it.k0 >= 0 &&
                        it.k0 < kMaxPosition;
    int n_chunk = it.n_chunk < 0 ? 0 : (it.n_chunk > C_max ? C_max : (int)it.n_chunk);
    int count = it.count < 0 ? 0 : (it.count > O_max ? O_max : (int)it.count);
    if (!listed) n_chunk = count = 0;
    const float* chunk = x + (long)i * C_max;
    float* yr = y + (long)i * O_max;
    const int hist = p.J - 1;
    const float* old = slots + (listed ? (long)it.slot * p.slot_floats + (it.parity & 1 ? hist : 0) : 0);
    const long nb = it.n_before;

    if (blockIdx.x == 0 && listed && n_chunk > 0 && !it.final && hist > 0) {
        // the last J - 1 samples after this chunk, into the buffer nobody reads in this launch
        float* fresh = slots + (long)it.slot * p.slot_floats + (it.parity & 1 ? 0 : hist);
        for (int e = threadIdx.x; e < hist; e += kThreads)
            fresh[e] = stream_sample(nb + n_chunk - hist + e, nb, n_chunk, hist, old, chunk);
    }

    const int T0 = blockIdx.x * p.tile;  // < O_max + tile
    const int t = threadIdx.x;
    if (T0 >= count) {  // the whole tile lies behind the item's outputs: zeros
        if (t < p.tile && T0 + t < O_max) yr[T0 + t] = 0.f;
        return;
    }
    if (p.u == 1 && p.d == 1) {  // the chunk bit for bit: output k is sample k
        if (t < p.tile && T0 + t < O_max) yr[T0 + t] = T0 + t < count ? stream_sample(it.k0 + T0 + t, nb, n_chunk, 0, old, chunk) : 0.f;
        return;
    }
    // inputs m_a .. m_b: from the oldest sample under the tile's first output to the newest under its last
    const long K0 = it.k0 + T0;
    const long m_a = (K0 * p.d + p.H) / p.u - hist;
    const long m_b = ((K0 + p.tile - 1) * p.d + p.H) / p.u;
    const int staged = (int)(m_b - m_a + 1);  // <= p.stretch (fsn_api_resample.hip, stream_plan)
    for (int e = t; e < staged; e += kThreads) xs[e] = stream_sample(m_a + e, nb, n_chunk, hist, old, chunk);
    if (TAPS_LDS)
        for (int e = t; e < p.u * p.Js; e += kThreads) lds[e] = poly[e];
    __syncthreads();
    if (t >= p.tile || T0 + t >= O_max) return;
    if (T0 + t >= count) {
        yr[T0 + t] = 0.f;
        return;
    }
    const double* table = TAPS_LDS ? lds : poly;
    const long c = (K0 + t) * p.d + p.H;
    const long q = c / p.u;
    const int phase = (int)(c - q * p.u);
    const double* row = table + (long)phase * p.Js;
    const float* xq = xs + (int)(q - m_a);  // x[q]; x[q - j] is staged down to j = J - 1
    double acc = 0.0;
    for (int j = 0; j < p.J; ++j) acc = fma(row[j], (double)xq[-j], acc);
    yr[T0 + t] = (float)acc;
}

__global__ __launch_bounds__(256) void resample_stream_reset_kernel(float* __restrict__ slots, int slot_floats, int capacity,
                                                                    const int* __restrict__ ids) {
    const int slot = ids[blockIdx.x];
    if (slot < 0 || slot >= capacity) return;
    float* s = slots + (long)slot * slot_floats;
    for (int e = threadIdx.x; e < slot_floats; e += 256) s[e] = 0.f;
}

}  // namespace

int fsn_launch_resample_stream(const FsnResampleStreamPlan& p, const double* poly, float* slots, int capacity,
                               const fsn_resample_stream_item* items, int n, const float* x, int C_max, float* y, int O_max,
                               hipStream_t s) {
    const size_t table = p.taps_in_lds ? (size_t)p.u * p.Js * sizeof(double) : 0;
    const size_t lds = table + (size_t)p.stretch * sizeof(float);
    if (lds > kFsnResampleLdsBytes) {
        fsn_set_error("fsn_launch_resample_stream: %zu bytes of LDS, a workgroup holds %zu", lds, kFsnResampleLdsBytes);
        return FSN_ERR_ARG;
    }
    const dim3 grid((O_max + p.tile - 1) / p.tile, n);
    if (p.taps_in_lds) {
        if (lds > 64 * 1024) FSN_TRY_RESERVE_LDS("resample_stream_kernel", resample_stream_kernel<true>, lds);
        hipLaunchKernelGGL(resample_stream_kernel<true>, grid, dim3(kThreads), lds, s, p, poly, slots, capacity, items, x, C_max, y,
                           O_max);
    } else {
        if (lds > 64 * 1024) FSN_TRY_RESERVE_LDS("resample_stream_kernel", resample_stream_kernel<false>, lds);
        hipLaunchKernelGGL(resample_stream_kernel<false>, grid, dim3(kThreads), lds, s, p, poly, slots, capacity, items, x, C_max,
                           y, O_max);
    }
    return fsn_check_launch("resample_stream_kernel");
}

int fsn_launch_resample_stream_reset(const FsnResampleStreamPlan& p, float* slots, int capacity, const int* ids, int n,
                                     hipStream_t s) {
    hipLaunchKernelGGL(resample_stream_reset_kernel, dim3(n), dim3(256), 0, s, slots, p.slot_floats, capacity, ids);
    return fsn_check_launch("resample_stream_reset_kernel");
}
