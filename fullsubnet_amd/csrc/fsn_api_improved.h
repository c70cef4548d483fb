// Host-side pieces shared by the two files of Improved FullSubNet's stateful C ABI - fsn_api_improved_stream.hip (the causal
// step) and fsn_api_improved_segment.hip (the offline norms in passes over segments): the configuration check, the packed
// weights' layout, the state blob, the workspace, the geometry record of the glue kernels and the host sequences of a block
// and of the sections' blocks.  Both files run the same blocks on the same blob; only the glue between them differs.
#pragma once

#include "fsn_api_internal.h"

namespace fsn_improved {

constexpr int kMaxWindow = 240;  // padded columns of a section's window (the tile of fsn_improved_section_input)

inline int sec_units(const fsn_improved_section& q) { return (q.upper - q.lower) / q.sb_center; }
inline int sec_width(const fsn_improved_section& q) {
    return q.sb_center + 2 * q.sb_neighbors + q.fb_center + 2 * q.fb_neighbors;
}

inline int check_cfg(const fsn_improved_cfg* c) {
    FSN_REQUIRE(c, "NULL configuration");
    FSN_REQUIRE(c->cell == 0, "improved stream: built for LSTM cells (cell %d; GRU blocks do not stream)", c->cell);
    FSN_REQUIRE(c->fdrc == 0.5f || c->fdrc == 1.0f, "improved stream: fdrc %g, the step takes 0.5 or 1", (double)c->fdrc);
    FSN_REQUIRE(c->F >= 3 && c->F - 1 <= kFsnImprovedMaxBins, "improved stream: F %d outside 3 .. %d", c->F, kFsnImprovedMaxBins + 1);
    FSN_REQUIRE(c->num_sections >= 2 && c->num_sections <= FSN_IMPROVED_MAX_SECTIONS, "improved stream: %d sections, the step takes 2 .. %d",
                c->num_sections, FSN_IMPROVED_MAX_SECTIONS);
    FSN_REQUIRE(c->fb_hidden >= 64 && c->fb_hidden <= 1024 && c->fb_hidden % 64 == 0 && c->sb_hidden >= 64 && c->sb_hidden <= 1024 &&
                    c->sb_hidden % 64 == 0,
                "improved stream: hidden sizes (%d, %d) must be multiples of 64 in 64 .. 1024 (pad them with zero weights)",
                c->fb_hidden, c->sb_hidden);
    FSN_REQUIRE((c->fb_activation == 0 || c->fb_activation == 1) && (c->sb_activation == 0 || c->sb_activation == 1),
                "improved stream: output activations (%d, %d), the step takes 0 (none) or 1 (ReLU)", c->fb_activation, c->sb_activation);
    const int Fm = c->F - 1;
    int next = 0;
    for (int i = 0; i < c->num_sections; ++i) {
        const fsn_improved_section& q = c->sec[i];
        FSN_REQUIRE(q.lower == next && q.upper > q.lower && q.upper <= Fm,
                    "improved stream: section %d covers [%d, %d), the sections must tile [0, %d) in order", i, q.lower, q.upper, Fm);
        next = q.upper;
        FSN_REQUIRE(q.sb_center >= 1 && q.fb_center >= 1 && q.sb_neighbors >= 0 && q.fb_neighbors >= 0 && q.sb_neighbors < Fm &&
                        q.fb_neighbors < Fm,
                    "improved stream: section %d: centres must be >= 1 and neighbours in 0 .. %d", i, Fm - 1);
        const int band = q.upper - q.lower;
        FSN_REQUIRE(band % q.sb_center == 0 && band % q.fb_center == 0 && band / q.sb_center == band / q.fb_center,
                    "improved stream: section %d: unit counts of the noisy and the fb window differ (%d bins by %d and by %d)", i, band,
                    q.sb_center, q.fb_center);
        FSN_REQUIRE(fsn_round_up(sec_width(q), 16) <= kMaxWindow, "improved stream: section %d: a window of %d columns, beyond %d padded columns",
                    i, sec_width(q), kMaxWindow);
    }
    FSN_REQUIRE(next == Fm, "improved stream: the sections end at bin %d, they must tile [0, %d)", next, Fm);
    return FSN_OK;
}
inline int check_stream(const fsn_improved_cfg* c, int B, int k) {
    FSN_TRY(check_cfg(c));
    FSN_REQUIRE(B >= 1 && B <= 4096 && k >= 1 && k <= 4096, "improved stream: batch %d / frames %d out of range", B, k);
    return FSN_OK;
}

// ---- packed weights: float offsets into the blob ------------------------------------------------------------------------
struct Layer {
    int I, H;
    size_t off;
};
struct Linear {
    int I, O;
    size_t w, b;
};
struct Block {
    Layer l0, l1;
    Linear fc;
};
struct Packed {
    Block fb, sb[FSN_IMPROVED_MAX_SECTIONS];
    size_t total;
};
inline Packed packed_layout(const fsn_improved_cfg* c) {
    Packed p{};
    size_t off = 0;
    auto block = [&](int I, int H, int O) {
        Block b{};
        b.l0 = Layer{I, H, off};
        off += fsn_round_up_sz(fsn_lstm_layer_packed_bytes(I, H) / sizeof(float), 64);
        b.l1 = Layer{H, H, off};
        off += fsn_round_up_sz(fsn_lstm_layer_packed_bytes(H, H) / sizeof(float), 64);
        b.fc = Linear{H, O, off, 0};
        off += fsn_round_up_sz((size_t)fsn_round_up(O, 16) * fsn_round_up(H, 16), 64);
        b.fc.b = off;
        off += fsn_round_up_sz((size_t)fsn_round_up(O, 16), 64);
        return b;
    };
    p.fb = block(c->F - 1, c->fb_hidden, c->F - 1);
    for (int i = 0; i < c->num_sections; ++i) p.sb[i] = block(sec_width(c->sec[i]), c->sb_hidden, 2 * c->sec[i].sb_center);
    p.total = off;
    return p;
}

// ---- the state blob and the workspace -------------------------------------------------------------------------------------
struct State {
    float* fb[4];                                // h, c of layer 0, h, c of layer 1: [Bp][fb_hidden]
    float* sb[FSN_IMPROVED_MAX_SECTIONS][4];     // the same of every section: [Np_i][sb_hidden]
    double *fb_sum, *sb_sum;                     // [B], [sections][B]
    long* steps;                                 // [B]
};
inline int sec_rows(const fsn_improved_cfg* c, int i, int B) { return fsn_round_up(B * sec_units(c->sec[i]), 16); }
inline State state_carve(Carver& cv, const fsn_improved_cfg* c, int B) {
    State st{};
    const size_t Bp = fsn_round_up(B, 16);
    for (int a = 0; a < 4; ++a) st.fb[a] = cv.take<float>(Bp * c->fb_hidden);
    for (int i = 0; i < c->num_sections; ++i)
        for (int a = 0; a < 4; ++a) st.sb[i][a] = cv.take<float>((size_t)sec_rows(c, i, B) * c->sb_hidden);
    st.fb_sum = cv.take<double>((size_t)B);
    st.sb_sum = cv.take<double>((size_t)c->num_sections * B);
    st.steps = cv.take<long>((size_t)B);
    return st;
}
struct SecWs {
    float *x, *gx, *hs_a, *hs_b, *out;
};
struct Ws {
    float *comp, *fb_in, *gx, *hs_a, *hs_b, *fb_out;
    SecWs sb[FSN_IMPROVED_MAX_SECTIONS];  // every section its own buffers: they run side by side
};
inline Ws ws_carve(Carver& cv, const fsn_improved_cfg* c, int B, int k) {
    Ws w{};
    const size_t Bp = fsn_round_up(B, 16), Fm = c->F - 1, FmP = fsn_round_up(c->F - 1, 16), kk = k, H = c->fb_hidden;
    w.comp = cv.take<float>(kk * Bp * FmP);
    w.fb_in = cv.take<float>(kk * Bp * FmP);
    w.gx = cv.take<float>(kk * Bp * 4 * H);
    w.hs_a = cv.take<float>(kk * Bp * H);
    w.hs_b = cv.take<float>(kk * Bp * H);
    w.fb_out = cv.take<float>(kk * Bp * Fm);
    for (int i = 0; i < c->num_sections; ++i) {
        const size_t Np = sec_rows(c, i, B), Ip = fsn_round_up(sec_width(c->sec[i]), 16), Hs = c->sb_hidden;
        w.sb[i].x = cv.take<float>(kk * Np * Ip);
        w.sb[i].gx = cv.take<float>(kk * Np * 4 * Hs);
        w.sb[i].hs_a = cv.take<float>(kk * Np * Hs);
        w.sb[i].hs_b = cv.take<float>(kk * Np * Hs);
        w.sb[i].out = cv.take<float>(kk * Np * 2 * c->sec[i].sb_center);
    }
    return w;
}

// the record the glue kernels take: k frames from frame t0 on, every section's window and buffers
inline FsnImprovedStream stream_geometry(const fsn_improved_cfg* cfg, int B, int k, long t0, const Ws& w) {
    FsnImprovedStream g{};
    g.B = B;
    g.Bp = fsn_round_up(B, 16);
    g.F = cfg->F;
    g.Fm = cfg->F - 1;
    g.FmP = fsn_round_up(cfg->F - 1, 16);
    g.k = k;
    g.sqrt_mode = cfg->fdrc == 0.5f ? 1 : 0;
    g.n = cfg->num_sections;
    g.t0 = t0;
    for (int i = 0; i < cfg->num_sections; ++i) {
        const fsn_improved_section& q = cfg->sec[i];
        FsnImprovedSection& d = g.s[i];
        d.lower = q.lower;
        d.units = sec_units(q);
        d.sc = q.sb_center;
        d.sn = q.sb_neighbors;
        d.fc = q.fb_center;
        d.fn = q.fb_neighbors;
        d.W = sec_width(q);
        d.Np = sec_rows(cfg, i, B);
        d.Ip = fsn_round_up(d.W, 16);
        d.x = w.sb[i].x;
        d.o = w.sb[i].out;
    }
    return g;
}

// T more steps of both layers of a block on N rows from its (h, c), updated in place, and its output layer:
// x [T][N][ldx] -> out [T N][O]
inline int run_block(const Block& b, const float* pk, const float* x, long ldx, int T, int N, float* const* hc, float* gx, float* hs_a,
                     float* hs_b, float* out, bool relu, void* stream) {
    FSN_TRY(fsn_lstm_layer_forward_state(x, ldx, pk + b.l0.off, T, N, b.l0.I, b.l0.H, hs_a, hc[0], hc[1], gx,
                                         fsn_lstm_layer_state_workspace_bytes(T, N, b.l0.H), stream));
    FSN_TRY(fsn_lstm_layer_forward_state(hs_a, b.l0.H, pk + b.l1.off, T, N, b.l1.I, b.l1.H, hs_b, hc[2], hc[3], gx,
                                         fsn_lstm_layer_state_workspace_bytes(T, N, b.l1.H), stream));
    const int rows = T * N;
    return fsn_launch_gemm(gemm_a_rows(hs_b, b.fc.I, rows), pk + b.fc.w, gemm_c_rows(out, b.fc.O, rows, b.fc.O, pk + b.fc.b, relu),
                           rows / 16, fsn_round_up(b.fc.O, 16) / 16, fsn_round_up(b.fc.I, 16) / 16, static_cast<hipStream_t>(stream));
}

// the sections' blocks, form 0: section 0, 2, .. on the caller's stream and 1, 3, .. beside them on the record's auxiliary
// stream
inline int run_sections_chains(const fsn_improved_cfg* cfg, const Packed& p, const float* pk, const State& st, const Ws& w,
                               const FsnImprovedStream& g, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream), aux = nullptr;
    FSN_TRY(aux_fork(s, &aux));
    for (int i = 0; i < g.n; ++i)
        FSN_TRY(run_block(p.sb[i], pk, w.sb[i].x, g.s[i].Ip, g.k, g.s[i].Np, st.sb[i], w.sb[i].gx, w.sb[i].hs_a, w.sb[i].hs_b,
                          w.sb[i].out, cfg->sb_activation == 1, i % 2 ? aux : stream));
    CallScope back(stream);  // the layer entries above left the thread on the stream they ran on last
    return aux_join(s);
}
// form 1: what fsn_lstm_layer_forward_state issues per section - the projection GEMM, a step launch per frame, the copy
// of the last h into the state - with the step launches of all sections as one and the copies as one
inline bool multi_takes(const FsnImprovedStream& g) {
    for (int i = 0; i < g.n; ++i)
        if (g.s[i].Np / 16 >= 64) return false;  // from 64 row tiles on the per-section launch is another kernel
    return true;
}
inline int run_sections_multi(const fsn_improved_cfg* cfg, const Packed& p, const float* pk, const State& st, const Ws& w,
                              const FsnImprovedStream& g, hipStream_t s) {
    const int H = cfg->sb_hidden, T = g.k;
    for (int layer = 0; layer < 2; ++layer) {
        FsnStepSets sets{};
        FsnImprovedKeep keep{};
        sets.n = keep.n = g.n;
        int tile0 = 0;
        for (int i = 0; i < g.n; ++i) {
            const Layer& l = layer ? p.sb[i].l1 : p.sb[i].l0;
            const LayerPacked lp = layer_packed_layout(l.I, l.H);
            const int N = g.s[i].Np;
            const float* x = layer ? w.sb[i].hs_a : w.sb[i].x;
            FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, layer ? H : g.s[i].Ip), pk + l.off + lp.wih,
                                    gemm_c_frag(w.sb[i].gx, pk + l.off + lp.bias), T * (N / 16), 4 * H / 16, fsn_round_up(l.I, 16) / 16, s));
            FsnStepSet& q = sets.s[i];
            q.gx = w.sb[i].gx;
            q.whh_p = pk + l.off + lp.whh;
            q.c = st.sb[i][2 * layer + 1];
            q.tile0 = tile0;
            q.tiles = N / 16;
            tile0 += q.tiles;
            float* hs = layer ? w.sb[i].hs_b : w.sb[i].hs_a;
            keep.dst[i] = st.sb[i][2 * layer];
            keep.src[i] = hs + (size_t)(T - 1) * N * H;
            keep.count[i] = (long)N * H;
        }
        for (int t = 0; t < T; ++t) {
            for (int i = 0; i < g.n; ++i) {
                const size_t step = (size_t)g.s[i].Np * H;
                float* hs = layer ? w.sb[i].hs_b : w.sb[i].hs_a;
                sets.s[i].h_prev = t ? hs + (t - 1) * step : st.sb[i][2 * layer];
                sets.s[i].h_out = hs + t * step;
                sets.s[i].gx_rt0 = (long)t * sets.s[i].tiles;
            }
            FSN_TRY(fsn_launch_lstm_step_multi(sets, H, s));
        }
        FSN_TRY(fsn_launch_improved_stream_keep(keep, s));
    }
    for (int i = 0; i < g.n; ++i) {
        const Linear& fc = p.sb[i].fc;
        const int rows = T * g.s[i].Np;
        FSN_TRY(fsn_launch_gemm(gemm_a_rows(w.sb[i].hs_b, fc.I, rows), pk + fc.w,
                                gemm_c_rows(w.sb[i].out, fc.O, rows, fc.O, pk + fc.b, cfg->sb_activation == 1), rows / 16,
                                fsn_round_up(fc.O, 16) / 16, fsn_round_up(fc.I, 16) / 16, s));
    }
    return FSN_OK;
}
// whichever form fsn_debug_improved_stream_form selects
inline int run_sections(const fsn_improved_cfg* cfg, const Packed& p, const float* pk, const State& st, const Ws& w,
                        const FsnImprovedStream& g, void* stream) {
    if (fsn_debug_improved_stream_form(-1) == 1 && multi_takes(g))
        return run_sections_multi(cfg, p, pk, st, w, g, static_cast<hipStream_t>(stream));
    return run_sections_chains(cfg, p, pk, st, w, g, stream);
}

}  // namespace fsn_improved
