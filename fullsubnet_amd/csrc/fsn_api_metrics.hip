// C ABI of the validation metrics on the device: fsn_stoi, its size query and fsn_si_sdr
// (include/fsn_hip.h "validation metrics on the device"; kernels: stoi_kernels.hip).
#include <math.h>
#include <stddef.h>

#include "fsn_api_internal.h"

namespace {

constexpr int kBands = 15, kSeg = 30, kCorrThreads = 256;

// The plan of a call: host arithmetic on its three numbers.  false (message set): an argument is out of range.
bool stoi_plan(const char* who, int B, int L_max, int sr, FsnStoiPlan* p) {
    if (B < 1 || L_max < 1) {
        fsn_set_error("%s: B = %d, L_max = %d: both must be at least 1", who, B, L_max);
        return false;
    }
    int up, down;
    if (sr == 10000) {
        up = down = 1;
    } else if (sr == 16000) {
        up = 5, down = 8;
    } else if (sr == 48000) {
        up = 5, down = 24;
    } else {
        fsn_set_error("%s: sr = %d: the sample rates are 10000, 16000 and 48000", who, sr);
        return false;
    }
    p->B = B;
    p->L_max = L_max;
    p->up = up;
    p->down = down;
    // L = ceil(52 / (28.714 fc / 10)) with fc = 1 / (2 max(up, down)): 290 at 16 kHz, 870 at 48 kHz
    p->half = sr == 10000 ? 0 : (int)ceil(52.0 / (28.714 * (1.0 / (2.0 * (double)down)) / 10.0));
    p->n10_max = fsn_stoi_n10(L_max, up, down, p->half);
    p->nf_max = fsn_stoi_frames(p->n10_max);
    p->m_max = p->nf_max > 1 ? p->nf_max - 1 : 1;
    const int j_max = p->m_max >= kSeg ? p->m_max - (kSeg - 1) : 1;
    p->j_blocks = (j_max + kCorrThreads - 1) / kCorrThreads;
    return true;
}

// the workspace, carved in this order (every array 256-byte aligned); base NULL: only the size is wanted
size_t stoi_carve(const FsnStoiPlan& p, void* base, FsnStoiBuffers* w) {
    Carver ws(base);
    const size_t nf = p.nf_max > 0 ? p.nf_max : 1;
    w->taps = ws.take<double>(2 * (size_t)p.half + 1);
    w->rs = ws.take<double>((size_t)p.B * 2 * p.n10_max);
    w->energy = ws.take<double>((size_t)p.B * nf);
    w->kept = ws.take<int>((size_t)p.B * nf);
    w->n_kept = ws.take<int>(p.B);
    w->tob = ws.take<double>((size_t)p.B * 2 * kBands * p.m_max);
    w->partial = ws.take<double>((size_t)p.B * kBands * p.j_blocks);
    return fsn_round_up_sz(ws.off, 256);
}

}  // namespace

extern "C" size_t fsn_stoi_workspace_bytes(int B, int L_max, int sr) {
    FsnStoiPlan p;
    FsnStoiBuffers w;
    if (!stoi_plan("fsn_stoi_workspace_bytes", B, L_max, sr, &p)) return 0;
    return stoi_carve(p, nullptr, &w);
}

extern "C" int fsn_stoi(const float* clean, const float* estimate, const int* lengths, int B, int L_max, int sr, double* d,
                        void* workspace, size_t workspace_bytes, void* stream) {
    FsnStoiPlan p;
    FsnStoiBuffers w;
    if (!stoi_plan("fsn_stoi", B, L_max, sr, &p)) return FSN_ERR_ARG;
    FSN_REQUIRE(clean && estimate && d, "fsn_stoi: NULL pointer argument");
    FSN_REQUIRE(workspace, "fsn_stoi: NULL workspace");
    FSN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "fsn_stoi: the workspace must be 256-byte aligned");
    const size_t least = stoi_carve(p, workspace, &w);
    FSN_REQUIRE(workspace_bytes >= least, "fsn_stoi: workspace of %zu bytes, at least %zu are needed", workspace_bytes, least);
    FsnCallScope scope(stream);
    return fsn_launch_stoi(clean, estimate, lengths, p, w, d, static_cast<hipStream_t>(stream));
}

extern "C" int fsn_si_sdr(const float* reference, const float* estimate, const int* lengths, int B, int L_max, double* out_db,
                          void* stream) {
    FSN_REQUIRE(B >= 1 && L_max >= 1, "fsn_si_sdr: B = %d, L_max = %d: both must be at least 1", B, L_max);
    FSN_REQUIRE(reference && estimate && out_db, "fsn_si_sdr: NULL pointer argument");
    FsnCallScope scope(stream);
    return fsn_launch_si_sdr(reference, estimate, lengths, B, L_max, out_db, static_cast<hipStream_t>(stream));
}
