// C ABI of libfsn_hip.so, Improved FullSubNet on recordings of any length under the offline norms: fsn_improved_segment_*
// (include/fsn_hip.h states the contract, DESIGN 9g "Recordings of any length (`fsn_improved_segment_*`, ...)" the passes).
// The weights, the state blob, the workspace and the blocks' host sequences are those of fsn_improved_stream_step
// (fsn_api_improved.h); the glue between the blocks is improved_segment_kernels.hip, and the mask is written by the stream
// step's own kernel.
#include "fsn_api_improved.h"

using namespace fsn_improved;

namespace {

// what every pass checks before it launches anything; `workspace` NULL with need_ws false: a pass that takes none
int check_segment_call(const fsn_improved_cfg* cfg, int B, int k, const void* state, size_t state_bytes, long frames_done,
                       const int* total_frames, bool need_ws, const void* workspace, size_t workspace_bytes) {
    FSN_TRY(check_stream(cfg, B, k));
    FSN_REQUIRE(state && total_frames && (workspace || !need_ws), "NULL pointer argument");
    FSN_REQUIRE(frames_done >= 0 && frames_done <= (1L << 52), "improved segment: frames_done %ld outside 0 .. 2^52", frames_done);
    if (state_bytes < fsn_improved_stream_state_bytes(cfg, B) ||
        (need_ws && workspace_bytes < fsn_improved_stream_workspace_bytes(cfg, B, k))) {
        fsn_set_error("improved segment: state / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}

}  // namespace

// pass 1: the full-band norm's sum
extern "C" int fsn_improved_segment_stats(const fsn_improved_cfg* cfg, void* state, size_t state_bytes, long frames_done,
                                          const int* total_frames, const float* mag, int B, int k, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, k, state, state_bytes, frames_done, total_frames, false, nullptr, 0));
    FSN_REQUIRE(mag, "NULL pointer argument");
    Carver cs(state);
    const State st = state_carve(cs, cfg, B);
    const FsnImprovedStream g = stream_geometry(cfg, B, k, frames_done, Ws{});
    return fsn_launch_improved_segment_stat(mag, st.fb_sum, total_frames, g, static_cast<hipStream_t>(stream));
}

// pass 2: the full-band block on its normalised input, its output to the caller's plane, the sections' sums
extern "C" int fsn_improved_segment_fullband(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                             int fb_norm, long frames_done, const int* total_frames, const float* mag, int B, int k,
                                             float* fb_out, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, k, state, state_bytes, frames_done, total_frames, true, workspace, workspace_bytes));
    FSN_REQUIRE(packed && mag && fb_out, "NULL pointer argument");
    FSN_REQUIRE(fb_norm == 0 || fb_norm == 1, "improved segment: fb_norm %d, the pass takes 0 (offline) or 1 (cumulative)", fb_norm);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const State st = state_carve(cs, cfg, B);
    const Ws w = ws_carve(cw, cfg, B, k);
    const FsnImprovedStream g = stream_geometry(cfg, B, k, frames_done, w);
    // model.py:565-568 with the finished (or the running) mean
    FSN_TRY(fsn_launch_improved_segment_front(fb_norm, mag, w.comp, w.fb_in, st.fb_sum, st.steps, total_frames, g, s));
    FSN_TRY(run_block(p.fb, pk, w.fb_in, g.FmP, k, g.Bp, st.fb, w.gx, w.hs_a, w.hs_b, w.fb_out, cfg->fb_activation == 1, stream));
    return fsn_launch_improved_segment_sums(w.comp, w.fb_out, g.Fm, fb_out, st.sb_sum, total_frames, g, s);
}

// pass 3: fsn_improved_stream_step from its sections on, with the one divisor of every finished sum
extern "C" int fsn_improved_segment_sections(const fsn_improved_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                             long frames_done, const int* total_frames, const float* mag, const float* fb_out, int B,
                                             int k, float* mask, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, k, state, state_bytes, frames_done, total_frames, true, workspace, workspace_bytes));
    FSN_REQUIRE(packed && mag && fb_out && mask, "NULL pointer argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const State st = state_carve(cs, cfg, B);
    const Ws w = ws_carve(cw, cfg, B, k);
    const FsnImprovedStream g = stream_geometry(cfg, B, k, frames_done, w);
    // model.py:402-449, 575
    FSN_TRY(fsn_launch_improved_segment_front(2, mag, w.comp, nullptr, nullptr, nullptr, total_frames, g, s));
    FSN_TRY(fsn_launch_improved_segment_sections(w.comp, fb_out, st.sb_sum, total_frames, g, s));
    FSN_TRY(run_sections(cfg, p, pk, st, w, g, stream));
    return fsn_launch_improved_stream_mask(mask, g, s);
}

extern "C" int fsn_improved_segment_divisors(const fsn_improved_cfg* cfg, const void* state, size_t state_bytes,
                                             const int* total_frames, int B, float* den_fb, float* den_sb, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, 1, state, state_bytes, 0, total_frames, false, nullptr, 0));
    FSN_REQUIRE(den_fb && den_sb, "NULL pointer argument");
    Carver cs(const_cast<void*>(state));
    const State st = state_carve(cs, cfg, B);
    const FsnImprovedStream g = stream_geometry(cfg, B, 1, 0, Ws{});
    return fsn_launch_improved_segment_divisors(st.fb_sum, st.sb_sum, total_frames, den_fb, den_sb, g, static_cast<hipStream_t>(stream));
}
