// Timing probe for fb_chain_kernel (not part of the library): the shipped kernel stand-alone on random operands.  Where a
// step of the full-band chain spends its time - the ablations that priced its ingredients one at a time - is on record in
// profiles/r02_chain_probe.md; the ablated variants are in git history before the commit that retired the kernel's
// experiment switches.
#include <cstdio>
#include <cstdlib>
#include "../fullsubnet_amd/csrc/fb_chain_kernels.hip"
void fsn_set_error(const char*, ...) {}
bool fsn_persistent_allowed() { return true; }
bool fsn_grid_fits(const void*, int, unsigned) { return true; }
void fsn_persist_admit(const void*, int, unsigned) {}
unsigned long long fsn_spin_ticks() { return 1ull << 31; }
unsigned* fsn_ctx_sticky() { return nullptr; }
int fsn_check_launch(const char*) { return hipGetLastError() == hipSuccess ? 0 : -3; }
int fsn_launch_zero_words(unsigned* p, size_t n, hipStream_t s) { return hipMemsetAsync(p, 0, n * 4, s) == hipSuccess ? 0 : -3; }
__global__ void fill_kernel(float* p, size_t n, unsigned seed, float scale, float offset) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned x = (unsigned)i * 747796405u + seed; x ^= x >> 16; x *= 2246822519u; x ^= x >> 13;
        p[i] = ((x & 0xffff) / 32768.0f - 1.0f) * scale + offset;
    }
}
template <int KS>
float run(ChainArgs a) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float best = 1e30f;
    for (int it = 0; it < 4; ++it) {
        hipMemsetAsync(a.flags, 0, fsn_fb_chain_flag_words() * 4, 0);
        hipEventRecord(e0, 0);
        hipLaunchKernelGGL((fb_chain_kernel<512, KS>), dim3(2 * 128), dim3(256), 0, 0, a);
        hipEventRecord(e1, 0); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1); if (it > 0 && ms < best) best = ms;
    }
    return best;
}
template <int KS>
void report(ChainArgs a, int Tp) {
    const float t0 = run<KS>(a);
    unsigned st = 0; hipMemcpy(&st, a.status, 4, hipMemcpyDeviceToHost);
    printf("fb_chain_kernel<KS=%d>, %d row tiles, %d steps: %.3f ms = %.2f us per step, status %u\n", KS, a.RT, Tp, t0, 1e3 * t0 / Tp, st);
}
int main(int argc, char** argv) {
    const int Tp = argc > 1 ? atoi(argv[1]) : 190, Npad = argc > 2 ? atoi(argv[2]) : 64;
    const int H = 512;
    float *gx0, *w, *b1, *ex, *hseq; unsigned* flags;
    hipMalloc(&gx0, (size_t)Tp * Npad * 4 * H * 4); hipMalloc(&w, (size_t)3 * 4 * H * H * 4); hipMalloc(&b1, 4 * H * 4);
    hipMalloc(&ex, fsn_fb_chain_exchange_floats(Tp, Npad) * 4); hipMalloc(&hseq, (size_t)Tp * Npad * H * 4);
    hipMalloc(&flags, fsn_fb_chain_flag_words() * 4);
    fill_kernel<<<1024, 256>>>(gx0, (size_t)Tp * Npad * 4 * H, 1, 1.0f, 0.f);
    fill_kernel<<<1024, 256>>>(w, (size_t)3 * 4 * H * H, 2, 0.05f, 0.f);
    fill_kernel<<<8, 256>>>(b1, 4 * H, 3, 0.1f, 0.f);
    hipDeviceSynchronize();
    ChainArgs a{};
    a.gx0 = gx0; a.whh0_p = w; a.wih1_p = w + (size_t)4 * H * H; a.whh1_p = w + (size_t)8 * H * H; a.b1 = b1;
    a.hx0 = ex; a.hx1 = ex + (size_t)Tp * Npad * H; a.gx1 = ex + (size_t)2 * Tp * Npad * H; a.hseq1 = hseq;
    a.flags = flags; a.status = flags + fsn_fb_chain_status_word(); a.spin_ticks = 1ull << 31; a.Tp = Tp; a.RT = Npad / 16; a.Npad = Npad;
    if (a.RT == 1) report<4>(a, Tp);
    else if (a.RT == 2) report<2>(a, Tp);
    else report<1>(a, Tp);
    return 0;
}
