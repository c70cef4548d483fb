// C ABI of the sample-rate conversion on the device: fsn_resample, its size and length queries, fsn_resample_taps
// (include/fsn_hip.h "sample-rate conversion on the device"; kernels: resample_kernels.hip).
#include <limits.h>
#include <math.h>
#include <stddef.h>

#include "fsn_api_internal.h"

namespace {

int gcd_of(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

// The plan of a call: host arithmetic on the rates and the design.  false (message set): a request out of range.
bool resample_plan(const char* who, int sr_in, int sr_out, int zeros, double beta, double rolloff, FsnResamplePlan* p) {
    if (sr_in < 1 || sr_out < 1) {
        fsn_set_error("%s: sr_in = %d, sr_out = %d: both rates must be positive", who, sr_in, sr_out);
        return false;
    }
    if (zeros < 1) {
        fsn_set_error("%s: zeros = %d: at least 1", who, zeros);
        return false;
    }
    if (!(beta >= 0.0 && beta <= FSN_RESAMPLE_MAX_BETA)) {  // the taps kernel sums I0's series over 512 terms
        fsn_set_error("%s: beta = %g: must lie in [0, %d]", who, beta, FSN_RESAMPLE_MAX_BETA);
        return false;
    }
    if (!(rolloff > 0.0 && rolloff <= 1.0)) {
        fsn_set_error("%s: rolloff = %g: must lie in (0, 1]", who, rolloff);
        return false;
    }
    const int g = gcd_of(sr_in, sr_out);
    const int u = sr_out / g, d = sr_in / g;
    const int P = u > d ? u : d;
    if (P > FSN_RESAMPLE_MAX_P) {
        fsn_set_error("%s: %d -> %d Hz is the ratio %d / %d: max(up, down) may be at most %d", who, sr_in, sr_out, u, d,
                      FSN_RESAMPLE_MAX_P);
        return false;
    }
    const long taps = 2L * zeros * P + 1;
    if (taps > FSN_RESAMPLE_MAX_TAPS) {
        fsn_set_error("%s: zeros = %d at the ratio %d / %d is a filter of %ld taps: at most %d", who, zeros, u, d, taps,
                      FSN_RESAMPLE_MAX_TAPS);
        return false;
    }
    p->u = u;
    p->d = d;
    p->H = zeros * P;
    p->taps = (int)taps;
    p->J = (p->taps + u - 1) / u;
    p->Js = p->J | 1;  // odd: the rows of consecutive phases start in different LDS banks
    p->beta = beta;
    p->rolloff = rolloff;
    // the largest pass S = u c (c <= 1024 / u: two rounds of the workgroup's threads, so that a tile is worth the table it
    // stages) whose tile of 8 S outputs needs no more input than a workgroup stages
    for (int c = 2 * kFsnResampleThreads / u > 1 ? 2 * kFsnResampleThreads / u : 1;; c /= 2) {
        p->S = u * c;
        p->tile = kFsnResampleOutPerThread * p->S;
        const long stretch = (long)(p->tile - 1) * d / u + p->J + 1;
        if (stretch <= kFsnResampleMaxStretch) {
            p->stretch = (int)stretch;
            break;
        }
        if (c == 1) {
            fsn_set_error("%s: the ratio %d / %d with %ld taps needs %ld input samples under %d outputs: a workgroup stages at "
                          "most %d",
                          who, u, d, taps, stretch, p->tile, kFsnResampleMaxStretch);
            return false;
        }
    }
    p->taps_in_lds =
        (size_t)u * p->Js * sizeof(double) + (size_t)p->stretch * sizeof(float) <= kFsnResampleLdsBytes ? 1 : 0;
    return true;
}

struct ResampleBuffers {
    double* h;     // [taps] natural order
    double* poly;  // [u][Js] polyphase order
};
size_t resample_carve(const FsnResamplePlan& p, void* base, ResampleBuffers* w) {
    Carver ws(base);
    w->h = ws.take<double>((size_t)p.taps);
    w->poly = ws.take<double>((size_t)p.u * p.Js);
    return fsn_round_up_sz(ws.off, 256);
}

}  // namespace

extern "C" long fsn_resample_out_length(long n, int sr_in, int sr_out) {
    if (sr_in < 1 || sr_out < 1 || n < 0) {
        fsn_set_error("fsn_resample_out_length: n = %ld, sr_in = %d, sr_out = %d: the rates must be positive, n at least 0", n,
                      sr_in, sr_out);
        return -1;
    }
    const int g = gcd_of(sr_in, sr_out);
    return fsn_resample_n_out(n, sr_out / g, sr_in / g);
}

extern "C" size_t fsn_resample_workspace_bytes(int sr_in, int sr_out, int zeros, double beta, double rolloff) {
    FsnResamplePlan p;
    ResampleBuffers w;
    if (!resample_plan("fsn_resample_workspace_bytes", sr_in, sr_out, zeros, beta, rolloff, &p)) return 0;
    return resample_carve(p, nullptr, &w);
}

extern "C" int fsn_debug_resample_plan(int sr_in, int sr_out, int zeros, int* out, int n) {
    FsnResamplePlan p;
    if (!resample_plan("fsn_debug_resample_plan", sr_in, sr_out, zeros, 5.0, 1.0, &p)) return FSN_ERR_ARG;
    // the longest row one workgroup covers: the largest n with ceil(n u / d) <= tile
    const long tile_inputs = (long)p.tile * p.d / p.u;
    const int v[10] = {p.u, p.d, p.H, p.taps, p.J, p.Js, p.tile, (int)tile_inputs, p.stretch, p.taps_in_lds};
    FSN_REQUIRE(out && n >= 1 && n <= 10, "fsn_debug_resample_plan: out = %p, n = %d: 1 to 10 values", (void*)out, n);
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return FSN_OK;
}

extern "C" int fsn_resample_taps(int sr_in, int sr_out, int zeros, double beta, double rolloff, double* h, size_t h_count,
                                 void* stream) {
    FsnResamplePlan p;
    if (!resample_plan("fsn_resample_taps", sr_in, sr_out, zeros, beta, rolloff, &p)) return FSN_ERR_ARG;
    FSN_REQUIRE(h, "fsn_resample_taps: NULL pointer argument");
    FSN_REQUIRE(h_count >= (size_t)p.taps, "fsn_resample_taps: room for %zu taps, the filter has %d", h_count, p.taps);
    FsnCallScope scope(stream);
    return fsn_launch_resample_taps(p, h, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" int fsn_resample(const float* x, const int* lengths, int B, int L_max, int sr_in, int sr_out, int zeros, double beta,
                            double rolloff, float* y, int L_out_max, int* out_lengths, void* workspace,
                            size_t workspace_bytes, void* stream) {
    FsnResamplePlan p;
    ResampleBuffers w;
    if (!resample_plan("fsn_resample", sr_in, sr_out, zeros, beta, rolloff, &p)) return FSN_ERR_ARG;
    FSN_REQUIRE(B >= 1 && B <= 65535 && L_max >= 1, "fsn_resample: B = %d, L_max = %d: B in [1, 65535], L_max at least 1", B,
                L_max);
    FSN_REQUIRE(x && y, "fsn_resample: NULL pointer argument");
    FSN_REQUIRE(x != y, "fsn_resample: y must not alias x");
    const long longest = fsn_resample_n_out(L_max, p.u, p.d);
    FSN_REQUIRE(L_out_max >= longest, "fsn_resample: L_out_max = %d, a row of L_max = %d samples has %ld at %d -> %d Hz",
                L_out_max, L_max, longest, sr_in, sr_out);
    FSN_REQUIRE(workspace, "fsn_resample: NULL workspace");
    FSN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "fsn_resample: the workspace must be 256-byte aligned");
    const size_t least = resample_carve(p, workspace, &w);
    FSN_REQUIRE(workspace_bytes >= least, "fsn_resample: workspace of %zu bytes, at least %zu are needed", workspace_bytes,
                least);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    FsnCallScope scope(stream);
    if (p.u != 1 || p.d != 1) FSN_TRY(fsn_launch_resample_taps(p, w.h, w.poly, s));
    return fsn_launch_resample(x, lengths, B, L_max, p, w.poly, y, L_out_max, out_lengths, s);
}
