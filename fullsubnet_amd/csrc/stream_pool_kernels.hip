// Streaming pool (fsn_fullsubnet_stream_pool_*): the model step of fsn_fullsubnet_stream_step over a SUBSET of the
// slots of a pool whose sessions open, advance and close on their own.
//
// The pool's state is one record per slot (FsnPoolLayout, fsn_common.h): (h, c) of the four LSTM layers, the two running
// fp64 norm sums, the slot's own step count and the transform state of fft_kernels.hip's pool kernels.  A step
//   1. gathers the listed slots' (h, c) rows into compact [Npad][H] tiles (pad rows and rows of an id outside the pool are
//      zeros, so every row the recurrent kernels touch is finite),
//   2. runs the lockstep entry's sequence on the compact rows, with the cumulative-norm denominators taken per row from the
//      slot's own carry and step count (the two kernels below),
//   3. scatters the rows back and advances the listed slots' step counts.
// Slots that are not listed are never written.  All copies move 16 bytes per lane, coalesced along H.
#include "fsn_common.h"

namespace {

// ---- (h, c) rows of the listed slots <-> compact tiles ------------------------------------------------------------------
// which == 0: the full-band model (one row of Hf per slot), 1: the sub-band model (F rows of Hs per slot).  blockIdx.y is the
// array (h0, h1, c0, c1); a thread moves one f32x4.  Gather fills all Npad rows; scatter writes the listed, valid ones and,
// for the sub-band model, advances the slot's step count by k (the last kernel of a step: nothing reads the count after it).
struct PoolTiles {
    float* p[4];
};
template <bool SCATTER>
__global__ __launch_bounds__(256) void pool_rows_kernel(char* __restrict__ state, FsnPoolLayout L, int capacity,
                                                        const int* __restrict__ slots, int n, int which, PoolTiles tiles,
                                                        int Npad, int k) {
    const int H = which ? L.Hs : L.Hf, rps = which ? L.F : 1, H4 = H / 4;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long row = idx / H4;
    const int c4 = (int)(idx % H4), arr = blockIdx.y;
    if (row >= Npad) return;
    const int i = (int)(row / rps), r = (int)(row % rps);
    char* rec = fsn_pool_record(state, L, capacity, slots, n, i);
    f32x4* tile = reinterpret_cast<f32x4*>(tiles.p[arr] + row * H) + c4;
    if (SCATTER) {
        if (!rec) return;
        f32x4* dst = reinterpret_cast<f32x4*>(rec + (which ? L.sb[arr] : L.fb[arr])) + (long)r * H4 + c4;
        *dst = *tile;
        if (which && arr == 0 && r == 0 && c4 == 0) *reinterpret_cast<int*>(rec + L.steps) += k;
    } else {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rec) v = *(reinterpret_cast<const f32x4*>(rec + (which ? L.sb[arr] : L.fb[arr])) + (long)r * H4 + c4);
        *tile = v;
    }
}

// ---- cumulative_laplace_norm with the carry and t0 of each row's slot ---------------------------------------------------
// cumulative_den_fb_kernel (elementwise_kernels.hip) per slot: den[i][t] = (carry + sum_{tau<=t} sum_f mag[i][tau][f]) /
// (F (t0 + t + 1)) + EPSILON, the same fp64 running sum.  One block per listed row; a skipped row gets den = 1.
__global__ __launch_bounds__(256) void pool_den_fb_kernel(const float* __restrict__ mag, float* __restrict__ den,
                                                          char* __restrict__ state, FsnPoolLayout L, int capacity,
                                                          const int* __restrict__ slots, int k) {
    __shared__ double scratch[4];
    const int i = blockIdx.x, F = L.F, FP = L.FP;
    char* rec = fsn_pool_record(state, L, capacity, slots, gridDim.x, i);
    if (!rec) {  // uniform over the block
        for (int t = threadIdx.x; t < k; t += blockDim.x) den[(long)i * k + t] = 1.0f;
        return;
    }
    double* carry = reinterpret_cast<double*>(rec + L.fb_sum);
    const int t0 = *reinterpret_cast<const int*>(rec + L.steps);
    double run = *carry;
    for (int t = 0; t < k; ++t) {
        double acc = 0.0;
        for (int f = threadIdx.x; f < F; f += blockDim.x) acc += (double)mag[((long)i * k + t) * FP + f];
        run += fsn_block_sum(acc, scratch);
        if (threadIdx.x == 0) den[(long)i * k + t] = (float)(run / ((double)F * (t0 + t + 1))) + kFsnEpsilon;
    }
    if (threadIdx.x == 0) *carry = run;
}

// cumulative_den_sb_kernel per slot: row nrow = i F + f of the compact order, den stored [k][Npad].  Pad rows and skipped
// rows get den = 1 (the input projection masks them; the value only has to be finite).
__global__ __launch_bounds__(256) void pool_den_sb_kernel(const float* __restrict__ mag, const float* __restrict__ fb_out,
                                                          float* __restrict__ den, char* __restrict__ state,
                                                          FsnPoolLayout L, int capacity, const int* __restrict__ slots,
                                                          int n, int k, int nb, int Npad) {
    const long nrow = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (nrow >= Npad) return;
    const int F = L.F, FP = L.FP;
    const int i = (int)(nrow / F), f = (int)(nrow % F);
    char* rec = fsn_pool_record(state, L, capacity, slots, n, i);
    if (!rec) {
        for (int t = 0; t < k; ++t) den[(long)t * Npad + nrow] = 1.0f;
        return;
    }
    double* carry = reinterpret_cast<double*>(rec + L.sb_sum) + f;
    const int t0 = *reinterpret_cast<const int*>(rec + L.steps);
    double run = *carry;
    for (int t = 0; t < k; ++t) {
        const float* row = mag + ((long)i * k + t) * FP;
        double acc = (double)fb_out[((long)i * k + t) * FP + f];
        for (int j = -nb; j <= nb; ++j) acc += (double)row[fsn_reflect_idx(f + j, F)];
        run += acc;
        den[(long)t * Npad + nrow] = (float)(run / ((double)(2 * nb + 2) * (t0 + t + 1))) + kFsnEpsilon;
    }
    *carry = run;
}

// the listed slots' records back to all zeros (a fresh slot), 16 bytes per lane; blockIdx.y is the row of `slots`
__global__ __launch_bounds__(256) void pool_reset_kernel(char* __restrict__ state, FsnPoolLayout L, int capacity,
                                                         const int* __restrict__ slots) {
    char* rec = fsn_pool_record(state, L, capacity, slots, gridDim.y, blockIdx.y);
    if (!rec) return;
    const size_t n16 = L.slot_bytes / 16;
    fsn_u32x4* p = reinterpret_cast<fsn_u32x4*>(rec);
    const fsn_u32x4 z = {0u, 0u, 0u, 0u};
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n16; j += (size_t)gridDim.x * blockDim.x) p[j] = z;
}

}  // namespace

static int pool_rows(bool scatter, void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, int which,
                     float* h0, float* h1, float* c0, float* c1, int Npad, int k, hipStream_t s) {
    PoolTiles t{{h0, h1, c0, c1}};
    const long threads = (long)Npad * ((which ? L.Hs : L.Hf) / 4);
    const dim3 grid((unsigned)((threads + 255) / 256), 4);
    if (scatter)
        hipLaunchKernelGGL(pool_rows_kernel<true>, grid, dim3(256), 0, s, static_cast<char*>(state), L, capacity, slots, n,
                           which, t, Npad, k);
    else
        hipLaunchKernelGGL(pool_rows_kernel<false>, grid, dim3(256), 0, s, static_cast<char*>(state), L, capacity, slots, n,
                           which, t, Npad, k);
    return fsn_check_launch("pool_rows_kernel");
}
int fsn_launch_pool_gather(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, int which, float* h0,
                           float* h1, float* c0, float* c1, int Npad, hipStream_t s) {
    return pool_rows(false, state, L, capacity, slots, n, which, h0, h1, c0, c1, Npad, 0, s);
}
int fsn_launch_pool_scatter(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, int which, float* h0,
                            float* h1, float* c0, float* c1, int Npad, int k, hipStream_t s) {
    return pool_rows(true, state, L, capacity, slots, n, which, h0, h1, c0, c1, Npad, k, s);
}
int fsn_launch_pool_den_fb(const float* mag, float* den, void* state, const FsnPoolLayout& L, int capacity, const int* slots,
                           int n, int k, hipStream_t s) {
    hipLaunchKernelGGL(pool_den_fb_kernel, dim3(n), dim3(256), 0, s, mag, den, static_cast<char*>(state), L, capacity, slots,
                       k);
    return fsn_check_launch("pool_den_fb_kernel");
}
int fsn_launch_pool_den_sb(const float* mag, const float* fb_out, float* den, void* state, const FsnPoolLayout& L,
                           int capacity, const int* slots, int n, int k, int nb, int Npad, hipStream_t s) {
    hipLaunchKernelGGL(pool_den_sb_kernel, dim3((unsigned)((Npad + 255) / 256)), dim3(256), 0, s, mag, fb_out, den,
                       static_cast<char*>(state), L, capacity, slots, n, k, nb, Npad);
    return fsn_check_launch("pool_den_sb_kernel");
}
int fsn_launch_pool_reset(void* state, const FsnPoolLayout& L, int capacity, const int* slots, int n, hipStream_t s) {
    const size_t n16 = L.slot_bytes / 16;
    const unsigned bx = (unsigned)((n16 + 255) / 256 < 256 ? (n16 + 255) / 256 : 256);
    hipLaunchKernelGGL(pool_reset_kernel, dim3(bx, n), dim3(256), 0, s, static_cast<char*>(state), L, capacity, slots);
    return fsn_check_launch("pool_reset_kernel");
}
