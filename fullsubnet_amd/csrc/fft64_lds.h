// fp64 complex transforms in LDS by a workgroup of kFftThreads threads: shared by the FFT convolution of mix_kernels.hip and
// the 512-point spectra of stoi_kernels.hip.  Radix 2, decimation in frequency forwards (natural in, bit-reversed out) and
// decimation in time backwards (bit-reversed in, natural out), so nothing is ever reordered; twiddles from sincospi of
// exact arguments.  Device code only; include it inside the file's unnamed namespace.
#pragma once

struct cd {
    double x, y;
};
__device__ __forceinline__ cd cadd(cd a, cd b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cd csub(cd a, cd b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cd cmul(cd a, cd b) { return {fma(a.x, b.x, -(a.y * b.y)), fma(a.x, b.y, a.y * b.x)}; }

__device__ __forceinline__ int bitrev(int v, int bits) { return bits == 0 ? 0 : (int)(__brev((unsigned)v) >> (32 - bits)); }

constexpr int kFftThreads = 256;

// tw[j] = e^(-2 pi i j / M), j < M / 2
__device__ __forceinline__ void fill_twiddles(cd* tw, int M) {
    for (int j = threadIdx.x; j < (M >> 1); j += kFftThreads) {
        double s, c;
        sincospi(-2.0 * (double)j / (double)M, &s, &c);
        tw[j] = cd{c, s};
    }
}

// `rows` transforms of M = 2^logM points each, a[r * M + i], in place, by the whole workgroup.  Forward: decimation in
// frequency, natural order in, bit-reversed out.  Inverse (unscaled): decimation in time, bit-reversed in, natural out.
// Ends with a barrier; the caller has one between its fill of `a` / `tw` and the call.
template <bool INV>
__device__ __forceinline__ void lds_fft(cd* a, const cd* tw, int M, int logM, int rows) {
    const int half = M >> 1, total = rows * half;
    for (int st = 0; st < logM; ++st) {
        const int lh = INV ? st : logM - 1 - st;  // log2 of the butterfly span h
        const int h = 1 << lh;
        for (int j = threadIdx.x; j < total; j += kFftThreads) {
            const int r = j / half, jj = j - r * half;
            const int pos = jj & (h - 1);
            const int i0 = r * M + ((jj >> lh) << (lh + 1)) + pos, i1 = i0 + h;
            cd w = tw[pos << (logM - 1 - lh)];  // W_2h^pos
            const cd u = a[i0], v = a[i1];
            if (INV) {
                w.y = -w.y;
                const cd t = cmul(v, w);
                a[i0] = cadd(u, t);
                a[i1] = csub(u, t);
            } else {
                a[i0] = cadd(u, v);
                a[i1] = cmul(csub(u, v), w);
            }
        }
        __syncthreads();
    }
}
