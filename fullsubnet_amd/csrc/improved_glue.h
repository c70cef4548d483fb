// Device pieces shared by Improved FullSubNet's stateful glue kernels (improved_stream_kernels.hip under the causal norms,
// improved_segment_kernels.hip under the offline ones): the mirror at the spectrum's ends, the fixed-shape workgroup sum and
// an entry of a section's window.  Included by those two kernel files only.
#pragma once

#include "fsn_common.h"

namespace fsn_improved_glue {

__device__ __forceinline__ int bin_reflect(int j, int Fm) {
    j = j < 0 ? -j : j;
    return j > Fm - 1 ? 2 * (Fm - 1) - j : j;
}

// The workgroup's sum of one double per thread, in a fixed order; valid in thread 0 (call from all 256 threads).
__device__ __forceinline__ double block_sum(double v, double* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// entry e = u W + w of a section's input: bins[0 .. Fm) the compressed magnitude, bins[Fm .. 2 Fm) the full-band output
__device__ __forceinline__ float section_entry(const float* bins, const FsnImprovedSection& q, int Fm, int e) {
    const int u = e / q.W, w = e - u * q.W, w_sb = q.sc + 2 * q.sn;
    if (w < w_sb) return bins[bin_reflect(q.lower + u * q.sc - q.sn + w, Fm)];
    return bins[Fm + bin_reflect(q.lower + u * q.fc - q.fn + (w - w_sb), Fm)];
}

// what every launcher of the two files checks before it launches
inline int check_geometry(const FsnImprovedStream& a, const char* what) {
    bool ok = a.B >= 1 && a.Bp >= a.B && a.F >= 2 && a.Fm == a.F - 1 && a.Fm <= kFsnImprovedMaxBins && a.FmP >= a.Fm && a.k >= 1 &&
              a.t0 >= 0 && a.n >= 1 && a.n <= 8 && (a.sqrt_mode == 0 || a.sqrt_mode == 1);
    for (int i = 0; ok && i < a.n; ++i) {
        const FsnImprovedSection& q = a.s[i];
        ok = q.lower >= 0 && q.units >= 1 && q.sc >= 1 && q.fc >= 1 && (long)q.lower + (long)q.units * q.sc <= a.Fm &&
             (long)q.lower + (long)q.units * q.fc <= a.Fm && q.sn >= 0 && q.fn >= 0 && q.sn <= a.Fm - 1 && q.fn <= a.Fm - 1 &&
             q.W == q.sc + 2 * q.sn + q.fc + 2 * q.fn && q.Ip >= q.W && (long)q.Np >= (long)a.B * q.units && q.x && q.o;
    }
    if (!ok) {
        fsn_set_error("%s: geometry outside the kernel (at most %d bins, 1 .. 8 sections inside them, padded sizes not below the sizes)",
                      what, kFsnImprovedMaxBins);
        return FSN_ERR_ARG;
    }
    return FSN_OK;
}

}  // namespace fsn_improved_glue
