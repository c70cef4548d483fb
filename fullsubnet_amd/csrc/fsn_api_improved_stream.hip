// C ABI of libfsn_hip.so, Improved FullSubNet as a stream: the packed weights, the state blob and the host sequence of
// fsn_improved_stream_step (k more model steps with carried state; include/fsn_hip.h states the contract, DESIGN "Improved
// FullSubNet as a stream" the section norm).  The recurrences run on the stateful layer entry
// (fsn_lstm_layer_forward_state on weights packed once by fsn_lstm_layer_pack), the output layers on the linear GEMM, and
// everything between them on improved_stream_kernels.hip.
#include <atomic>

#include "fsn_api_internal.h"

namespace {

// how the sections' blocks run: 0 a chain of stateful layer launches per section, half of the sections beside the other half
// on the auxiliary stream; 1 one step launch per layer and frame over the row tiles of all sections
// (lstm_step_multi_kernel).  The two give the same bits.  Measured at 48 kHz, k = 1 (profiles/improved_stream.md, DESIGN
// 9g): fewer launches do not pay - the chains on two streams take 0.40 ms, the multi-set form on one 0.48 - so 0 is the
// default and 1 is kept for the test that holds the two to each other.
std::atomic<int> g_form{0};

constexpr int kMaxWindow = 240;  // padded columns of a section's window (the tile of fsn_improved_section_input)
constexpr int kMaxBins = 4096;   // F - 1 the sections kernel stages (improved_stream_kernels.hip)

int sec_units(const fsn_improved_section& q) { return (q.upper - q.lower) / q.sb_center; }
int sec_width(const fsn_improved_section& q) {
    return q.sb_center + 2 * q.sb_neighbors + q.fb_center + 2 * q.fb_neighbors;
}

int check_cfg(const fsn_improved_cfg* c) {
    FSN_REQUIRE(c, "NULL configuration");
    FSN_REQUIRE(c->cell == 0, "improved stream: built for LSTM cells (cell %d; GRU blocks do not stream)", c->cell);
    FSN_REQUIRE(c->fdrc == 0.5f || c->fdrc == 1.0f, "improved stream: fdrc %g, the step takes 0.5 or 1", (double)c->fdrc);
    FSN_REQUIRE(c->F >= 3 && c->F - 1 <= kMaxBins, "improved stream: F %d outside 3 .. %d", c->F, kMaxBins + 1);
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
int check_stream(const fsn_improved_cfg* c, int B, int k) {
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
Packed packed_layout(const fsn_improved_cfg* c) {
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
int sec_rows(const fsn_improved_cfg* c, int i, int B) { return fsn_round_up(B * sec_units(c->sec[i]), 16); }
State state_carve(Carver& cv, const fsn_improved_cfg* c, int B) {
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
Ws ws_carve(Carver& cv, const fsn_improved_cfg* c, int B, int k) {
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

int pack_block(const Block& b, const float* const* t, float* pk, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    FSN_TRY(fsn_lstm_layer_pack(t[0], t[1], t[2], t[3], b.l0.I, b.l0.H, pk + b.l0.off, fsn_lstm_layer_packed_bytes(b.l0.I, b.l0.H), stream));
    FSN_TRY(fsn_lstm_layer_pack(t[4], t[5], t[6], t[7], b.l1.I, b.l1.H, pk + b.l1.off, fsn_lstm_layer_packed_bytes(b.l1.I, b.l1.H), stream));
    const int Ip = fsn_round_up(b.fc.I, 16), Op = fsn_round_up(b.fc.O, 16);
    FSN_TRY(fsn_launch_pack(t[8], pk + b.fc.w, b.fc.O, b.fc.I, Op, Ip, s));
    return fsn_launch_bias_sum(t[9], nullptr, pk + b.fc.b, b.fc.O, Op, s);
}
// T more steps of both layers of a block on N rows from its (h, c), updated in place, and its output layer:
// x [T][N][ldx] -> out [T N][O]
int run_block(const Block& b, const float* pk, const float* x, long ldx, int T, int N, float* const* hc, float* gx, float* hs_a,
              float* hs_b, float* out, bool relu, void* stream) {
    FSN_TRY(fsn_lstm_layer_forward_state(x, ldx, pk + b.l0.off, T, N, b.l0.I, b.l0.H, hs_a, hc[0], hc[1], gx,
                                         fsn_lstm_layer_state_workspace_bytes(T, N, b.l0.H), stream));
    FSN_TRY(fsn_lstm_layer_forward_state(hs_a, b.l0.H, pk + b.l1.off, T, N, b.l1.I, b.l1.H, hs_b, hc[2], hc[3], gx,
                                         fsn_lstm_layer_state_workspace_bytes(T, N, b.l1.H), stream));
    const int rows = T * N;
    return fsn_launch_gemm(gemm_a_rows(hs_b, b.fc.I, rows), pk + b.fc.w, gemm_c_rows(out, b.fc.O, rows, b.fc.O, pk + b.fc.b, relu),
                           rows / 16, fsn_round_up(b.fc.O, 16) / 16, fsn_round_up(b.fc.I, 16) / 16, static_cast<hipStream_t>(stream));
}

// (d), form 0: section 0, 2, .. on the caller's stream and 1, 3, .. beside them on the record's auxiliary stream
int run_sections_chains(const fsn_improved_cfg* cfg, const Packed& p, const float* pk, const State& st, const Ws& w,
                        const FsnImprovedStream& g, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream), aux = nullptr;
    FSN_TRY(aux_fork(s, &aux));
    for (int i = 0; i < g.n; ++i)
        FSN_TRY(run_block(p.sb[i], pk, w.sb[i].x, g.s[i].Ip, g.k, g.s[i].Np, st.sb[i], w.sb[i].gx, w.sb[i].hs_a, w.sb[i].hs_b,
                          w.sb[i].out, cfg->sb_activation == 1, i % 2 ? aux : stream));
    CallScope back(stream);  // the layer entries above left the thread on the stream they ran on last
    return aux_join(s);
}
// (d), form 1: what fsn_lstm_layer_forward_state issues per section - the projection GEMM, a step launch per frame, the copy
// of the last h into the state - with the step launches of all sections as one and the copies as one
bool multi_takes(const FsnImprovedStream& g) {
    for (int i = 0; i < g.n; ++i)
        if (g.s[i].Np / 16 >= 64) return false;  // from 64 row tiles on the per-section launch is another kernel
    return true;
}
int run_sections_multi(const fsn_improved_cfg* cfg, const Packed& p, const float* pk, const State& st, const Ws& w,
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

}  // namespace

// test hook: 0 / 1 selects how the sections' blocks run (see g_form), anything else changes nothing; returns the form in use
extern "C" int fsn_debug_improved_stream_form(int form) {
    if (form == 0 || form == 1) g_form = form;
    return g_form;
}

extern "C" size_t fsn_improved_stream_packed_bytes(const fsn_improved_cfg* cfg) {
    if (check_cfg(cfg) != FSN_OK) return 0;
    return fsn_round_up_sz(packed_layout(cfg).total * sizeof(float), 256);
}

extern "C" int fsn_improved_stream_pack(const fsn_improved_cfg* cfg, const fsn_improved_params* w, void* packed, size_t packed_bytes,
                                        void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_cfg(cfg));
    FSN_REQUIRE(w && packed, "NULL pointer argument");
    for (int j = 0; j < 10; ++j) {
        FSN_REQUIRE(w->fb[j], "improved stream pack: NULL weight tensor");
        for (int i = 0; i < cfg->num_sections; ++i) FSN_REQUIRE(w->sb[i][j], "improved stream pack: NULL weight tensor");
    }
    if (packed_bytes < fsn_improved_stream_packed_bytes(cfg)) {
        fsn_set_error("improved stream pack: buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    const Packed p = packed_layout(cfg);
    float* pk = static_cast<float*>(packed);
    FSN_TRY(pack_block(p.fb, w->fb, pk, stream));
    for (int i = 0; i < cfg->num_sections; ++i) FSN_TRY(pack_block(p.sb[i], w->sb[i], pk, stream));
    return FSN_OK;
}

extern "C" size_t fsn_improved_stream_state_bytes(const fsn_improved_cfg* cfg, int B) {
    if (check_stream(cfg, B, 1) != FSN_OK) return 0;
    Carver cv(nullptr);
    state_carve(cv, cfg, B);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" size_t fsn_improved_stream_workspace_bytes(const fsn_improved_cfg* cfg, int B, int k) {
    if (check_stream(cfg, B, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    ws_carve(cv, cfg, B, k);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_debug_improved_stream_state_layout(const fsn_improved_cfg* cfg, int B, long* out, int n) {
    if (!out || n < 50 || check_stream(cfg, B, 1) != FSN_OK) return -1;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);  // never dereferenced: only differences are taken
    Carver cv(base);
    const State st = state_carve(cv, cfg, B);
    auto at = [&](const void* p) { return p ? (long)(static_cast<const char*>(p) - base) : -1L; };
    for (int a = 0; a < 4; ++a) out[a] = at(st.fb[a]);
    for (int i = 0; i < FSN_IMPROVED_MAX_SECTIONS; ++i) {
        for (int a = 0; a < 4; ++a) out[4 + 4 * i + a] = at(st.sb[i][a]);
        out[40 + i] = i < cfg->num_sections ? sec_rows(cfg, i, B) : -1;
    }
    out[36] = at(st.fb_sum);
    out[37] = at(st.sb_sum);
    out[38] = at(st.steps);
    out[39] = fsn_round_up(B, 16);
    out[48] = cfg->num_sections;
    out[49] = (long)fsn_round_up_sz(cv.off, 256);
    return 0;
}

// The order of a call: front and full-band norm, the full-band block, the windows and norms of all sections, the sections'
// blocks (each on buffers of its own) and the mask.  Launches and copies at k = 1 with S sections: 2 glue + 7 for the
// full-band block (per layer the projection GEMM, the step and the state copy; the output GEMM) + the mask = 10, and for the
// sections 7 S as chains (form 0) or 3 S + 4 with the multi-set step (form 1: per layer S projections, one step, one copy
// kernel; S output GEMMs).
extern "C" int fsn_improved_stream_step(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                        long steps_done, const float* mag, int B, int k, float* mask, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_stream(cfg, B, k));
    FSN_REQUIRE(packed && state && mag && mask && workspace && steps_done >= 0, "NULL pointer argument / negative step count");
    FSN_REQUIRE(steps_done <= (1L << 52), "improved stream: step count beyond 2^52");
    if (state_bytes < fsn_improved_stream_state_bytes(cfg, B) || workspace_bytes < fsn_improved_stream_workspace_bytes(cfg, B, k)) {
        fsn_set_error("improved stream: state / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->F, Fm = F - 1, FmP = fsn_round_up(Fm, 16), Bp = fsn_round_up(B, 16), S = cfg->num_sections;
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const State st = state_carve(cs, cfg, B);
    const Ws w = ws_carve(cw, cfg, B, k);
    FsnImprovedStream g{};
    g.B = B;
    g.Bp = Bp;
    g.F = F;
    g.Fm = Fm;
    g.FmP = FmP;
    g.k = k;
    g.sqrt_mode = cfg->fdrc == 0.5f ? 1 : 0;
    g.n = S;
    g.t0 = steps_done;
    for (int i = 0; i < S; ++i) {
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
    // (a) - (b) model.py:565-568
    FSN_TRY(fsn_launch_improved_stream_front(mag, w.comp, w.fb_in, st.fb_sum, st.steps, g, s));
    FSN_TRY(run_block(p.fb, pk, w.fb_in, FmP, k, Bp, st.fb, w.gx, w.hs_a, w.hs_b, w.fb_out, cfg->fb_activation == 1, stream));
    // (c) - (d) model.py:402-449
    FSN_TRY(fsn_launch_improved_stream_sections(w.comp, w.fb_out, Fm, st.sb_sum, g, s));
    if (g_form == 1 && multi_takes(g)) FSN_TRY(run_sections_multi(cfg, p, pk, st, w, g, s));
    else FSN_TRY(run_sections_chains(cfg, p, pk, st, w, g, stream));
    // (e) model.py:443-449, 575
    return fsn_launch_improved_stream_mask(mask, g, s);
}
