// C ABI of libfsn_hip.so, Improved FullSubNet's streaming pool: fsn_improved_stream_step over a subset of the slots of a pool
// whose sessions are not in lockstep, and the frame transforms around it (include/fsn_hip.h states the contract, DESIGN 9h
// the record and what is bit-equal).  A step is the lockstep entry's own host sequence (fsn_api_improved.h: run_block,
// run_sections, state_carve, ws_carve, stream_geometry) on a compact state that improved_stream_pool_kernels.hip gathers from
// and scatters to the listed records; the glue kernels take every row's divisor count from the gathered counts.
#include "fsn_api_improved.h"

using namespace fsn_improved;

namespace {

constexpr int kMaxCapacity = 4096;

int check_pool(const fsn_improved_cfg* c, int capacity) {
    FSN_TRY(check_cfg(c));
    FSN_REQUIRE(capacity >= 1 && capacity <= kMaxCapacity, "improved streaming pool: capacity %d outside 1 .. %d", capacity, kMaxCapacity);
    return FSN_OK;
}
FsnImprovedPoolLayout pool_layout(const fsn_improved_cfg* c) {
    int units[FSN_IMPROVED_MAX_SECTIONS] = {};
    for (int i = 0; i < c->num_sections; ++i) units[i] = sec_units(c->sec[i]);
    return fsn_improved_pool_layout(c->F, c->fb_hidden, c->sb_hidden, c->num_sections, units);
}
int check_pool_call(const fsn_improved_cfg* c, const void* state, size_t state_bytes, int capacity, const int* slots, int n) {
    FSN_TRY(check_pool(c, capacity));
    FSN_REQUIRE(state && slots, "NULL pointer argument");
    FSN_REQUIRE(n >= 1 && n <= capacity, "improved streaming pool: %d slots listed, need 1 .. capacity = %d", n, capacity);
    if (state_bytes < (size_t)capacity * pool_layout(c).slot_bytes) {
        fsn_set_error("improved streaming pool: state buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}
// behind the lockstep entry's workspace: the compact state (its layout at B = n) and every row's own count
struct PoolWs {
    State st;
    long* t0;
};
PoolWs pool_ws_carve(Carver& cv, const fsn_improved_cfg* c, int n) {
    PoolWs p{};
    p.st = state_carve(cv, c, n);
    p.t0 = cv.take<long>((size_t)n);
    return p;
}
int check_pool_fft(const fsn_improved_cfg* c, int n_fft, int hop) {
    FSN_REQUIRE(n_fft >= 4 && n_fft <= 4096 && n_fft % 2 == 0 && hop * 2 == n_fft,
                "improved streaming pool: the transform is built for an even n_fft in 4 .. 4096 with hop = n_fft / 2 (got %d/%d)", n_fft, hop);
    FSN_REQUIRE(c->F == n_fft / 2 + 1, "F %d != n_fft/2+1", c->F);
    return FSN_OK;
}

}  // namespace

extern "C" size_t fsn_improved_stream_pool_state_bytes(const fsn_improved_cfg* cfg, int capacity) {
    if (check_pool(cfg, capacity) != FSN_OK) return 0;
    return (size_t)capacity * pool_layout(cfg).slot_bytes;
}

extern "C" size_t fsn_improved_stream_pool_workspace_bytes(const fsn_improved_cfg* cfg, int n, int k) {
    if (check_stream(cfg, n, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    ws_carve(cv, cfg, n, k);
    pool_ws_carve(cv, cfg, n);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_improved_stream_pool_reset(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                              const int* slots, int n, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FsnPoolLayout L{};  // the FullSubNet pool's reset kernel: it reads slot_bytes alone
    L.slot_bytes = pool_layout(cfg).slot_bytes;
    return fsn_launch_pool_reset(state, L, capacity, slots, n, static_cast<hipStream_t>(stream));
}

// The order of a call: gather; the lockstep entry's five stages (front and full-band norm, the full-band block, the windows
// and norms of all sections, the sections' blocks, the mask) on the compact state; scatter.  Two launches more than
// fsn_improved_stream_step at B = n.
extern "C" int fsn_improved_stream_pool_step(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                             int capacity, const int* slots, int n, const float* mag, int k, float* mask_out,
                                             void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_stream(cfg, n, k));
    FSN_REQUIRE(packed && mag && mask_out && workspace, "NULL pointer argument");
    if (workspace_bytes < fsn_improved_stream_pool_workspace_bytes(cfg, n, k)) {
        fsn_set_error("improved streaming pool: workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cw(workspace);
    const Ws w = ws_carve(cw, cfg, n, k);
    const PoolWs pw = pool_ws_carve(cw, cfg, n);
    const State& st = pw.st;
    FsnImprovedStream g = stream_geometry(cfg, n, k, 0, w);
    g.t0_rows = pw.t0;
    FsnImprovedPool q{};
    q.state = static_cast<char*>(state);
    q.L = pool_layout(cfg);
    q.slots = slots;
    q.capacity = capacity;
    q.n = n;
    q.k = k;
    q.rows[0] = g.Bp;
    for (int a = 0; a < 4; ++a) q.tile[0][a] = st.fb[a];
    for (int i = 0; i < cfg->num_sections; ++i) {
        q.rows[1 + i] = g.s[i].Np;
        for (int a = 0; a < 4; ++a) q.tile[1 + i][a] = st.sb[i][a];
    }
    q.fb_sum = st.fb_sum;
    q.sb_sum = st.sb_sum;
    q.t0 = pw.t0;
    // 1. the listed records -> the compact state
    FSN_TRY(fsn_launch_improved_pool_gather(q, s));
    // 2. - 4. fsn_improved_stream_step's sequence, every row's divisors from its own count
    FSN_TRY(fsn_launch_improved_stream_front(mag, w.comp, w.fb_in, st.fb_sum, st.steps, g, s));
    FSN_TRY(run_block(p.fb, pk, w.fb_in, g.FmP, k, g.Bp, st.fb, w.gx, w.hs_a, w.hs_b, w.fb_out, cfg->fb_activation == 1, stream));
    FSN_TRY(fsn_launch_improved_stream_sections(w.comp, w.fb_out, g.Fm, st.sb_sum, g, s));
    FSN_TRY(run_sections(cfg, p, pk, st, w, g, stream));
    FSN_TRY(fsn_launch_improved_stream_mask(mask_out, g, s));
    // 5. last: it advances the listed slots' step counts
    return fsn_launch_improved_pool_scatter(q, s);
}

extern "C" int fsn_improved_stream_pool_analysis(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                                 const int* slots, int n, const float* hops, const float* prime,
                                                 const int* frame_no, int n_fft, int hop, const float* window, float* mag,
                                                 void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_pool_fft(cfg, n_fft, hop));
    FSN_REQUIRE(hops && frame_no && window && mag, "NULL pointer argument");
    return fsn_launch_improved_pool_analysis(state, pool_layout(cfg), capacity, slots, n, hops, prime, frame_no, window, mag,
                                             static_cast<hipStream_t>(stream));
}

extern "C" int fsn_improved_stream_pool_synthesis(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                                  const int* slots, int n, const float* mask, const int* tail_samples, int n_fft,
                                                  int hop, const float* window, float* out, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_pool_fft(cfg, n_fft, hop));
    FSN_REQUIRE(mask && tail_samples && window && out, "NULL pointer argument");
    return fsn_launch_improved_pool_synthesis(state, pool_layout(cfg), capacity, slots, n, mask, tail_samples, window, out,
                                              static_cast<hipStream_t>(stream));
}

// test hook (host only): where the fields of one record lie, from the function the entries lay it out with
extern "C" int fsn_debug_improved_stream_pool_layout(const fsn_improved_cfg* cfg, long* out, int n) {
    if (!out || n < 58 || check_pool(cfg, 1) != FSN_OK) return -1;
    const FsnImprovedPoolLayout L = pool_layout(cfg);
    for (int a = 0; a < 4; ++a) out[a] = (long)L.fb[a];
    for (int i = 0; i < FSN_IMPROVED_MAX_SECTIONS; ++i) {
        for (int a = 0; a < 4; ++a) out[4 + 4 * i + a] = i < L.n ? (long)L.sb[i][a] : -1;
        out[50 + i] = i < L.n ? L.units[i] : -1;
    }
    const size_t rest[9] = {L.fb_sum, L.sb_sum, L.steps, L.in_tail, L.ola_tail, L.spec_re, L.spec_im, L.frame, L.slot_bytes};
    for (int i = 0; i < 9; ++i) out[36 + i] = (long)rest[i];
    const int dims[5] = {L.F, L.hop, L.Hf, L.Hs, L.n};
    for (int i = 0; i < 5; ++i) out[45 + i] = dims[i];
    return 0;
}
