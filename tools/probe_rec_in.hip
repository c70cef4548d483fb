// Timing probe for lstm_rec_in_kernel (not part of the library): the shipped instantiations stand-alone at config 2's shape
// (four row tiles per workgroup on 256 workgroups).  The variants that priced the hidden sequence's stores and the input
// gather are on record in profiles/r05_rec_probes.md.
#include <cstdio>
#include <cstdlib>
#include "../fullsubnet_amd/csrc/lstm_rec_in_kernels.hip"
void fsn_set_error(const char*, ...) {}
int fsn_check_launch(const char*) { return hipGetLastError() == hipSuccess ? 0 : -3; }
FsnCallScope::FsnCallScope(void*) : prev(-1), switched(false) {}
FsnCallScope::~FsnCallScope() {}
__global__ void fill_kernel(float* p, size_t n, unsigned seed, float scale, float offset) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned x = (unsigned)i * 747796405u + seed; x ^= x >> 16; x *= 2246822519u; x ^= x >> 13;
        p[i] = ((x & 0xffff) / 32768.0f - 1.0f) * scale + offset;
    }
}
template <bool GRU, int KX, bool ROWSIN>
float run(const FsnSbInput& xin, const float* w, float* hseq, int Tp, int Npad) {
    constexpr int H = 384, RT = 4, UG = 2, NW = H / (16 * UG);
    const size_t lds = ((size_t)RT * 16 * (H + 4) + (size_t)2 * RT * 16 * (16 * KX + 4)) * sizeof(float);
    auto kern = lstm_rec_in_kernel<H, RT, UG, GRU, KX, ROWSIN>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float best = 1e30f;
    for (int it = 0; it < 7; ++it) {
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL(kern, dim3(256), dim3(NW * 64), lds, 0, xin, w, (unsigned)(4 * H * 16 * KX), hseq, Tp, Npad);
        hipEventRecord(e1, 0); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); if (it > 0 && ms < best) best = ms;
    }
    return best;
}
int main(int argc, char** argv) {
    const int Tp = argc > 1 ? atoi(argv[1]) : 190;
    const int H = 384, tiles = 1028, Npad = tiles * 16, F = 257, FP = 272, B = 64;
    float *mag, *fb, *den, *rows, *w, *bias, *hseq;
    hipMalloc(&mag, (size_t)B * Tp * FP * 4);
    hipMalloc(&fb, (size_t)B * Tp * FP * 4);
    hipMalloc(&den, 256);
    hipMalloc(&rows, (size_t)Tp * Npad * 32 * 4);
    hipMalloc(&w, (size_t)(4 * H * 32 + 4 * H * H) * 4);
    hipMalloc(&bias, 4 * H * 4);
    hipMalloc(&hseq, (size_t)Tp * Npad * H * 4);
    fill_kernel<<<1024, 256>>>(mag, (size_t)B * Tp * FP, 1, 0.5f, 0.6f);
    fill_kernel<<<1024, 256>>>(fb, (size_t)B * Tp * FP, 5, 0.5f, 0.6f);
    fill_kernel<<<1, 64>>>(den, 64, 6, 0.1f, 0.7f);
    fill_kernel<<<1024, 256>>>(rows, (size_t)Tp * Npad * 32, 7, 1.0f, 0.f);
    fill_kernel<<<256, 256>>>(w, (size_t)(4 * H * 32 + 4 * H * H), 2, 0.05f, 0.f);
    fill_kernel<<<8, 256>>>(bias, 4 * H, 3, 0.1f, 0.f);
    hipDeviceSynchronize();
    FsnSbInput xin{};  // the gathered sub-band input
    xin.mag = mag; xin.fb_out = fb; xin.den = den; xin.wih_p = w; xin.bias = bias; xin.den_mode = 0; xin.den_stride = 0;
    xin.B = B; xin.Tp = Tp; xin.F = F; xin.FP = FP; xin.N = B * F; xin.nb = 15; xin.kin_chunks = 2; xin.x_rows = nullptr; xin.row0 = 0;
    FsnSbInput xr = xin;  // the plain row-major input, 32 columns in memory (one or two chunks of them used)
    xr.x_rows = rows; xr.x_ld = 32; xr.x_step = Npad;
    printf("lstm_rec_in_kernel<384,4,2,..> x 256 workgroups, %d steps\n", Tp);
#define FORM(NAME, GRU, KX, ROWSIN, XIN, WORK)                                                                       \
    {                                                                                                                \
        const double flops = 2.0 * 256 * 64 * (16.0 * KX + 384.0) * 1536 * Tp * WORK;                                 \
        const float ms = run<GRU, KX, ROWSIN>(XIN, w, hseq, Tp, Npad);                                               \
        printf("  %-44s: %.3f ms = %.1f TFLOP/s (ideal at 157.3: %.3f ms)\n", NAME, ms, flops / ms / 1e9, flops / 157.3e9); \
    }
    FORM("LSTM, gathered sub-band input (K = 32)", false, 2, false, xin, 1.0)
    FORM("LSTM, row-major input, two chunks", false, 2, true, xr, 1.0)
    FORM("LSTM, row-major input, one chunk", false, 1, true, xr, 1.0)
    FORM("GRU (four-gate cell), row-major, two chunks", true, 2, true, xr, 0.75)
    FORM("GRU (four-gate cell), row-major, one chunk", true, 1, true, xr, 0.75)
#undef FORM
    return 0;
}
