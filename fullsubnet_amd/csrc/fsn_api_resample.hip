// C ABI of the sample-rate conversion on the device: fsn_resample, its size and length queries, fsn_resample_taps
// (include/fsn_hip.h "sample-rate conversion on the device"; kernels: resample_kernels.hip), and of its streaming form,
// fsn_resample_stream_* ("sample-rate conversion of streams"; kernels: resample_stream_kernels.hip).
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

// ---- streams (include/fsn_hip.h "sample-rate conversion of streams"; kernels: resample_stream_kernels.hip) -------------
namespace {

// The streaming plan of a ratio and a filter length: whatever fsn_resample refuses of them is refused here (beta and
// rolloff shape the taps, not the plan: fsn_resample_stream_init checks them).
bool stream_plan(const char* who, int sr_in, int sr_out, int zeros, FsnResamplePlan* offline, FsnResampleStreamPlan* p) {
    if (!resample_plan(who, sr_in, sr_out, zeros, offline->beta, offline->rolloff, offline)) return false;
    const bool copy = offline->u == 1 && offline->d == 1;
    p->u = offline->u;
    p->d = offline->d;
    p->H = copy ? 0 : offline->H;
    p->J = copy ? 1 : offline->J;
    p->Js = copy ? 1 : offline->Js;
    for (int tile = kFsnResampleStreamThreads;; tile /= 2) {
        const long stretch = (long)(tile - 1) * p->d / p->u + p->J + 1;
        if (stretch <= kFsnResampleStreamMaxStretch) {
            p->tile = tile;
            p->stretch = (int)stretch;
            break;
        }
        if (tile == 1) {
            fsn_set_error("%s: %d taps per phase at the ratio %d / %d: a workgroup stages at most %d input samples", who, p->J,
                          p->u, p->d, kFsnResampleStreamMaxStretch);
            return false;
        }
    }
    // staging the table costs u Js loads; the tile reads tile J entries of it
    const size_t table = (size_t)p->u * p->Js * sizeof(double);
    p->taps_in_lds = !copy && table + (size_t)p->stretch * sizeof(float) <= kFsnResampleLdsBytes &&
                             (long)p->u * p->Js <= (long)p->tile * p->J
                         ? 1
                         : 0;
    p->slot_floats = fsn_round_up(2 * (p->J - 1) > 1 ? 2 * (p->J - 1) : 1, 64);
    return true;
}

struct StreamBlob {
    double* h;     // [taps] natural order (what resample_taps_kernel sums over)
    double* poly;  // [u][Js]
    float* slots;  // [capacity][slot_floats]
};
size_t stream_carve(const FsnResamplePlan& offline, const FsnResampleStreamPlan& p, int capacity, void* base, StreamBlob* b) {
    Carver c(base);
    b->h = c.take<double>((size_t)offline.taps);
    b->poly = c.take<double>((size_t)offline.u * offline.Js);
    b->slots = c.take<float>((size_t)capacity * p.slot_floats);
    return fsn_round_up_sz(c.off, 256);
}

// the checks every call on a blob shares; beta / rolloff as given (init) or the defaults (they do not enter the layout)
int stream_call(const char* who, void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros, double beta,
                double rolloff, FsnResamplePlan* offline, FsnResampleStreamPlan* p, StreamBlob* b) {
    offline->beta = beta;
    offline->rolloff = rolloff;
    if (!stream_plan(who, sr_in, sr_out, zeros, offline, p)) return FSN_ERR_ARG;
    FSN_REQUIRE(capacity >= 1 && capacity <= 65535, "%s: capacity = %d: 1 to 65535 sessions", who, capacity);
    FSN_REQUIRE(state, "%s: NULL state", who);
    FSN_REQUIRE((reinterpret_cast<uintptr_t>(state) & 255) == 0, "%s: the state must be 256-byte aligned", who);
    const size_t want = stream_carve(*offline, *p, capacity, state, b);
    FSN_REQUIRE(state_bytes == want, "%s: a state of %zu bytes, %d sessions at %d -> %d Hz with zeros = %d have %zu", who,
                state_bytes, capacity, sr_in, sr_out, zeros, want);
    return FSN_OK;
}

}  // namespace

extern "C" long fsn_resample_stream_ready(long n_in, int final, int sr_in, int sr_out, int zeros) {
    FsnResamplePlan offline;
    FsnResampleStreamPlan p;
    offline.beta = 5.0;
    offline.rolloff = 1.0;
    if (!stream_plan("fsn_resample_stream_ready", sr_in, sr_out, zeros, &offline, &p)) return -1;
    if (n_in < 0) {
        fsn_set_error("fsn_resample_stream_ready: n_in = %ld", n_in);
        return -1;
    }
    if (final) return fsn_resample_n_out(n_in, p.u, p.d);
    return n_in * p.u <= p.H ? 0 : (n_in * p.u - p.H - 1) / p.d + 1;
}

extern "C" size_t fsn_resample_stream_state_bytes(int sr_in, int sr_out, int zeros, int capacity) {
    FsnResamplePlan offline;
    FsnResampleStreamPlan p;
    StreamBlob b;
    offline.beta = 5.0;
    offline.rolloff = 1.0;
    if (!stream_plan("fsn_resample_stream_state_bytes", sr_in, sr_out, zeros, &offline, &p)) return 0;
    if (capacity < 1 || capacity > 65535) {
        fsn_set_error("fsn_resample_stream_state_bytes: capacity = %d: 1 to 65535 sessions", capacity);
        return 0;
    }
    return stream_carve(offline, p, capacity, nullptr, &b);
}

extern "C" int fsn_resample_stream_init(void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros,
                                        double beta, double rolloff, void* stream) {
    FsnResamplePlan offline;
    FsnResampleStreamPlan p;
    StreamBlob b;
    FSN_TRY(stream_call("fsn_resample_stream_init", state, state_bytes, capacity, sr_in, sr_out, zeros, beta, rolloff, &offline,
                        &p, &b));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    FsnCallScope scope(stream);
    if (p.u != 1 || p.d != 1) FSN_TRY(fsn_launch_resample_taps(offline, b.h, b.poly, s));
    return fsn_launch_zero_words(reinterpret_cast<unsigned*>(b.slots), (size_t)capacity * p.slot_floats, s);
}

extern "C" int fsn_resample_stream_push(void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros,
                                        const fsn_resample_stream_item* items, int n, const float* x, int C_max, float* y,
                                        int O_max, void* stream) {
    FsnResamplePlan offline;
    FsnResampleStreamPlan p;
    StreamBlob b;
    FSN_TRY(stream_call("fsn_resample_stream_push", state, state_bytes, capacity, sr_in, sr_out, zeros, 5.0, 1.0, &offline, &p,
                        &b));
    FSN_REQUIRE(n >= 1 && n <= capacity, "fsn_resample_stream_push: n = %d sessions of %d", n, capacity);
    FSN_REQUIRE(items && x && y, "fsn_resample_stream_push: NULL pointer argument");
    FSN_REQUIRE(x != y, "fsn_resample_stream_push: y must not alias x");
    FSN_REQUIRE(C_max >= 1 && C_max <= (1 << 30) && O_max >= 1 && O_max <= (1 << 30),
                "fsn_resample_stream_push: C_max = %d, O_max = %d: both in [1, 2^30]", C_max, O_max);
    FsnCallScope scope(stream);
    return fsn_launch_resample_stream(p, b.poly, b.slots, capacity, items, n, x, C_max, y, O_max, static_cast<hipStream_t>(stream));
}

extern "C" int fsn_resample_stream_reset(void* state, size_t state_bytes, int capacity, int sr_in, int sr_out, int zeros,
                                         const int* slots, int n, void* stream) {
    FsnResamplePlan offline;
    FsnResampleStreamPlan p;
    StreamBlob b;
    FSN_TRY(stream_call("fsn_resample_stream_reset", state, state_bytes, capacity, sr_in, sr_out, zeros, 5.0, 1.0, &offline, &p,
                        &b));
    FSN_REQUIRE(n >= 1 && n <= capacity, "fsn_resample_stream_reset: n = %d sessions of %d", n, capacity);
    FSN_REQUIRE(slots, "fsn_resample_stream_reset: NULL pointer argument");
    FsnCallScope scope(stream);
    return fsn_launch_resample_stream_reset(p, b.slots, capacity, slots, n, static_cast<hipStream_t>(stream));
}
