// C ABI of libfsn_hip.so, Improved FullSubNet as a stream: the packed weights, the state blob and the host sequence of
// fsn_improved_stream_step (k more model steps with carried state; include/fsn_hip.h states the contract, DESIGN "Improved
// FullSubNet as a stream" the section norm).  The recurrences run on the stateful layer entry
// (fsn_lstm_layer_forward_state on weights packed once by fsn_lstm_layer_pack), the output layers on the linear GEMM, and
// everything between them on improved_stream_kernels.hip.
#include <atomic>

#include "fsn_api_improved.h"

using namespace fsn_improved;

namespace {

// how the sections' blocks run: 0 a chain of stateful layer launches per section, half of the sections beside the other half
// on the auxiliary stream; 1 one step launch per layer and frame over the row tiles of all sections
// (lstm_step_multi_kernel).  The two give the same bits.  Measured at 48 kHz, k = 1 (profiles/improved_stream.md, DESIGN
// 9g): fewer launches do not pay - the chains on two streams take 0.40 ms, the multi-set form on one 0.48 - so 0 is the
// default and 1 is kept for the test that holds the two to each other.
std::atomic<int> g_form{0};

int pack_block(const Block& b, const float* const* t, float* pk, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    FSN_TRY(fsn_lstm_layer_pack(t[0], t[1], t[2], t[3], b.l0.I, b.l0.H, pk + b.l0.off, fsn_lstm_layer_packed_bytes(b.l0.I, b.l0.H), stream));
    FSN_TRY(fsn_lstm_layer_pack(t[4], t[5], t[6], t[7], b.l1.I, b.l1.H, pk + b.l1.off, fsn_lstm_layer_packed_bytes(b.l1.I, b.l1.H), stream));
    const int Ip = fsn_round_up(b.fc.I, 16), Op = fsn_round_up(b.fc.O, 16);
    FSN_TRY(fsn_launch_pack(t[8], pk + b.fc.w, b.fc.O, b.fc.I, Op, Ip, s));
    return fsn_launch_bias_sum(t[9], nullptr, pk + b.fc.b, b.fc.O, Op, s);
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
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const State st = state_carve(cs, cfg, B);
    const Ws w = ws_carve(cw, cfg, B, k);
    const FsnImprovedStream g = stream_geometry(cfg, B, k, steps_done, w);
    // (a) - (b) model.py:565-568
    FSN_TRY(fsn_launch_improved_stream_front(mag, w.comp, w.fb_in, st.fb_sum, st.steps, g, s));
    FSN_TRY(run_block(p.fb, pk, w.fb_in, g.FmP, k, g.Bp, st.fb, w.gx, w.hs_a, w.hs_b, w.fb_out, cfg->fb_activation == 1, stream));
    // (c) - (d) model.py:402-449
    FSN_TRY(fsn_launch_improved_stream_sections(w.comp, w.fb_out, g.Fm, st.sb_sum, g, s));
    FSN_TRY(run_sections(cfg, p, pk, st, w, g, stream));
    // (e) model.py:443-449, 575
    return fsn_launch_improved_stream_mask(mask, g, s);
}
