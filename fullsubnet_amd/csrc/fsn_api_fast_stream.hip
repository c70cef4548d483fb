// C ABI of libfsn_hip.so, Fast FullSubNet as a stream: the packed weights, the state blob and the host sequence of
// fsn_fast_stream_step (k more model steps with carried state; include/fsn_hip.h states the contract, DESIGN why the model
// is causal).  The recurrences run on the stateful layer entry (fsn_lstm_layer_forward_state on weights packed once by
// fsn_lstm_layer_pack), the mel product and the output layers on the linear GEMM, the ends on fast_glue_kernels.hip's
// spec_rows / mask_out with look-ahead 0, and everything that touches the state between them on fast_stream_kernels.hip.
// The same stages under the offline norm, as three passes over the segments of a recording of any length
// (fsn_fast_segment_*), follow the step; their state-touching glue is fast_segment_kernels.hip.
#include "fsn_api_internal.h"

namespace {

constexpr int kEnc0H = 384, kEnc1H = 320, kDecH = 512;  // the reference's literals (model.py:36-96); 257 units run padded to 320

int unit_width(const fsn_fast_cfg* c) { return 2 * c->mel_neighbors + 1 + 2 * c->enc_neighbors + 1; }

// what every entry of this file asks of a configuration, whatever its norm
int check_shape(const fsn_fast_cfg* c) {
    FSN_REQUIRE(c->F == 257 && c->num_mels == 64, "fast stream: F %d / num_mels %d, the step takes 257 / 64 (the reference's block widths)",
                c->F, c->num_mels);
    FSN_REQUIRE(c->shrink >= 1, "fast stream: shrink %d must be >= 1", c->shrink);
    FSN_REQUIRE(c->mel_neighbors >= 0 && c->mel_neighbors <= 7 && c->enc_neighbors >= 0 && c->enc_neighbors <= 7,
                "fast stream: neighbours (%d, %d) outside 0 .. 7", c->mel_neighbors, c->enc_neighbors);
    FSN_REQUIRE(c->bn_hidden >= 128 && c->bn_hidden <= 512 && c->bn_hidden % 128 == 0 && (c->bn_layers == 1 || c->bn_layers == 2),
                "fast stream: bottleneck %d x %d, the step takes 128, 256, 384 or 512 units with 1 or 2 layers", c->bn_hidden,
                c->bn_layers);
    return FSN_OK;
}
int check_cfg(const fsn_fast_cfg* c) {
    FSN_REQUIRE(c, "NULL configuration");
    FSN_REQUIRE(c->norm == FSN_NORM_CUMULATIVE_LAPLACE, "streaming needs the causal norm (FSN_NORM_CUMULATIVE_LAPLACE)");
    return check_shape(c);
}
int check_stream(const fsn_fast_cfg* c, int B, int k) {
    FSN_TRY(check_cfg(c));
    FSN_REQUIRE(B >= 1 && B <= 4096 && k >= 1 && k <= 4096, "fast stream: batch %d / frames %d out of range", B, k);
    return FSN_OK;
}

// ---- packed weights: float offsets into the blob ------------------------------------------------------------------------
struct Layer {
    int I, H;
    size_t off;
};
struct Linear {
    int I, O;  // I: the (padded) input width
    size_t w, b;
};
struct Packed {
    Linear mel, enc_fc, bn_fc, dec_fc;
    Layer enc0, enc1, bn[2], dec0, dec1;
    size_t total;
};
Packed packed_layout(const fsn_fast_cfg* c) {
    Packed p{};
    size_t off = 0;
    auto layer = [&](int I, int H) {
        Layer l{I, H, off};
        off += fsn_round_up_sz(fsn_lstm_layer_packed_bytes(I, H) / sizeof(float), 64);
        return l;
    };
    auto linear = [&](int I, int O) {
        Linear l{I, O, 0, 0};
        const size_t Ip = fsn_round_up(I, 16), Op = fsn_round_up(O, 16);
        l.w = off;
        off += fsn_round_up_sz(Op * Ip, 64);
        l.b = off;
        off += fsn_round_up_sz(Op, 64);
        return l;
    };
    const int M = c->num_mels, H = c->bn_hidden;
    p.mel = linear(c->F, M);
    p.enc0 = layer(M, kEnc0H);
    p.enc1 = layer(kEnc0H, kEnc1H);
    p.enc_fc = linear(kEnc1H, M);
    p.bn[0] = layer(unit_width(c), H);
    p.bn[1] = c->bn_layers == 2 ? layer(H, H) : Layer{0, 0, 0};
    p.bn_fc = linear(H, 1);
    p.dec0 = layer(2 * M, kDecH);
    p.dec1 = layer(kDecH, kDecH);
    p.dec_fc = linear(kDecH, 2 * c->F);
    p.total = off;
    return p;
}

// ---- the state blob and the workspace -------------------------------------------------------------------------------------
struct State {
    float *enc0_h, *enc0_c, *enc1_h, *enc1_c, *dec0_h, *dec0_c, *dec1_h, *dec1_c, *bn_h[2], *bn_c[2];
    double *mel_sum, *unit_sum;
    float *partial, *held;
};
State state_carve(Carver& cv, const fsn_fast_cfg* c, int B) {
    State st{};
    const size_t Bp = fsn_round_up(B, 16), N = (size_t)B * c->num_mels;
    st.enc0_h = cv.take<float>(Bp * kEnc0H);
    st.enc0_c = cv.take<float>(Bp * kEnc0H);
    st.enc1_h = cv.take<float>(Bp * kEnc1H);
    st.enc1_c = cv.take<float>(Bp * kEnc1H);
    st.dec0_h = cv.take<float>(Bp * kDecH);
    st.dec0_c = cv.take<float>(Bp * kDecH);
    st.dec1_h = cv.take<float>(Bp * kDecH);
    st.dec1_c = cv.take<float>(Bp * kDecH);
    for (int l = 0; l < c->bn_layers; ++l) {
        st.bn_h[l] = cv.take<float>(N * c->bn_hidden);
        st.bn_c[l] = cv.take<float>(N * c->bn_hidden);
    }
    st.mel_sum = cv.take<double>((size_t)B);
    st.unit_sum = cv.take<double>(N);
    st.partial = cv.take<float>(N * unit_width(c));
    st.held = cv.take<float>(N);
    return st;
}
struct Ws {
    float *rows, *mel, *enc_in, *gx, *hseq_a, *hseq_b, *enc, *units, *bn_a, *bn_b, *slow, *dec_in, *out;
};
// the low-rate frames a call of k steps can complete, whatever its phase
int max_low_frames(int k, int shrink) { return (k + shrink - 1) / shrink; }
Ws ws_carve(Carver& cv, const fsn_fast_cfg* c, int B, int k) {
    Ws w{};
    const size_t Bp = fsn_round_up(B, 16), Fp = fsn_fpad(c->F), M = c->num_mels, N = (size_t)B * M, kk = k;
    const size_t low = max_low_frames(k, c->shrink), Wp = fsn_round_up(unit_width(c), 16), H = c->bn_hidden;
    w.rows = cv.take<float>(kk * Bp * Fp);
    w.mel = cv.take<float>(kk * Bp * M);
    w.enc_in = cv.take<float>(kk * Bp * M);
    const size_t gx_pairs = kk * Bp * 4 * kDecH, gx_bn = low * N * 4 * H;  // the widest input projection of a layer
    w.gx = cv.take<float>(gx_pairs > gx_bn ? gx_pairs : gx_bn);
    w.hseq_a = cv.take<float>(kk * Bp * kDecH);
    w.hseq_b = cv.take<float>(kk * Bp * kDecH);
    w.enc = cv.take<float>(kk * Bp * M);
    w.units = cv.take<float>(low * N * Wp);
    w.bn_a = cv.take<float>(low * N * H);
    w.bn_b = cv.take<float>(low * N * H);
    w.slow = cv.take<float>(low * N);
    w.dec_in = cv.take<float>(kk * Bp * 2 * M);
    w.out = cv.take<float>(kk * Bp * 2 * c->F);
    return w;
}

int pack_linear(const Linear& l, int I, const float* w, const float* b, float* pk, hipStream_t s) {
    const int Ip = fsn_round_up(l.I, 16), Op = fsn_round_up(l.O, 16);
    FSN_TRY(fsn_launch_pack(w, pk + l.w, l.O, I, Op, Ip, s));
    if (b) return fsn_launch_bias_sum(b, nullptr, pk + l.b, l.O, Op, s);
    if (hipMemsetAsync(pk + l.b, 0, (size_t)Op * sizeof(float), s) != hipSuccess) {
        fsn_set_error("fast stream pack: clearing a bias failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}
// y [rows][l.O] = x [rows][ldx] W^T + b (+ ReLU); rows a multiple of 16
int run_linear(const Linear& l, const float* pk, const float* x, long ldx, float* y, int rows, bool relu, hipStream_t s) {
    return fsn_launch_gemm(gemm_a_rows(x, ldx, rows), pk + l.w, gemm_c_rows(y, l.O, rows, l.O, pk + l.b, relu), rows / 16,
                           fsn_round_up(l.O, 16) / 16, fsn_round_up(l.I, 16) / 16, s);
}
// T more steps of one layer on N rows from (h, c), which are updated in place: x [T][N][ldx] -> hseq [T][N][H]
int run_layer(const Layer& l, const float* pk, const float* x, long ldx, int T, int N, float* hseq, float* h, float* c, float* gx,
              void* stream) {
    return fsn_lstm_layer_forward_state(x, ldx, pk + l.off, T, N, l.I, l.H, hseq, h, c, gx,
                                        fsn_lstm_layer_state_workspace_bytes(T, N, l.H), stream);
}

}  // namespace

extern "C" size_t fsn_fast_stream_packed_bytes(const fsn_fast_cfg* cfg) {
    if (check_cfg(cfg) != FSN_OK) return 0;
    return fsn_round_up_sz(packed_layout(cfg).total * sizeof(float), 256);
}

extern "C" int fsn_fast_stream_pack(const fsn_fast_cfg* cfg, const fsn_fast_params* w, void* packed, size_t packed_bytes,
                                    void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_cfg(cfg));
    FSN_REQUIRE(w && packed, "NULL pointer argument");
    const bool two = cfg->bn_layers == 2;
    FSN_REQUIRE(w->mel_w && w->enc0_w_ih && w->enc0_w_hh && w->enc0_b_ih && w->enc0_b_hh && w->enc1_w_ih && w->enc1_w_hh &&
                    w->enc1_b_ih && w->enc1_b_hh && w->enc1_fc_w && w->enc1_fc_b && w->bn_w_ih_l0 && w->bn_w_hh_l0 && w->bn_b_ih_l0 &&
                    w->bn_b_hh_l0 && (!two || (w->bn_w_ih_l1 && w->bn_w_hh_l1 && w->bn_b_ih_l1 && w->bn_b_hh_l1)) && w->bn_fc_w &&
                    w->bn_fc_b && w->dec0_w_ih && w->dec0_w_hh && w->dec0_b_ih && w->dec0_b_hh && w->dec1_w_ih && w->dec1_w_hh &&
                    w->dec1_b_ih && w->dec1_b_hh && w->dec1_fc_w && w->dec1_fc_b,
                "fast stream pack: NULL weight tensor");
    if (packed_bytes < fsn_fast_stream_packed_bytes(cfg)) {
        fsn_set_error("fast stream pack: buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const Packed p = packed_layout(cfg);
    float* pk = static_cast<float*>(packed);
    auto layer = [&](const Layer& l, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh) {
        return fsn_lstm_layer_pack(w_ih, w_hh, b_ih, b_hh, l.I, l.H, pk + l.off, fsn_lstm_layer_packed_bytes(l.I, l.H), stream);
    };
    FSN_TRY(pack_linear(p.mel, cfg->F, w->mel_w, nullptr, pk, s));
    FSN_TRY(layer(p.enc0, w->enc0_w_ih, w->enc0_w_hh, w->enc0_b_ih, w->enc0_b_hh));
    FSN_TRY(layer(p.enc1, w->enc1_w_ih, w->enc1_w_hh, w->enc1_b_ih, w->enc1_b_hh));
    FSN_TRY(pack_linear(p.enc_fc, kEnc1H, w->enc1_fc_w, w->enc1_fc_b, pk, s));
    FSN_TRY(layer(p.bn[0], w->bn_w_ih_l0, w->bn_w_hh_l0, w->bn_b_ih_l0, w->bn_b_hh_l0));
    if (two) FSN_TRY(layer(p.bn[1], w->bn_w_ih_l1, w->bn_w_hh_l1, w->bn_b_ih_l1, w->bn_b_hh_l1));
    FSN_TRY(pack_linear(p.bn_fc, cfg->bn_hidden, w->bn_fc_w, w->bn_fc_b, pk, s));
    FSN_TRY(layer(p.dec0, w->dec0_w_ih, w->dec0_w_hh, w->dec0_b_ih, w->dec0_b_hh));
    FSN_TRY(layer(p.dec1, w->dec1_w_ih, w->dec1_w_hh, w->dec1_b_ih, w->dec1_b_hh));
    return pack_linear(p.dec_fc, kDecH, w->dec1_fc_w, w->dec1_fc_b, pk, s);
}

extern "C" size_t fsn_fast_stream_state_bytes(const fsn_fast_cfg* cfg, int B) {
    if (check_stream(cfg, B, 1) != FSN_OK) return 0;
    Carver cv(nullptr);
    state_carve(cv, cfg, B);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" size_t fsn_fast_stream_workspace_bytes(const fsn_fast_cfg* cfg, int B, int k) {
    if (check_stream(cfg, B, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    ws_carve(cv, cfg, B, k);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_debug_fast_stream_state_layout(const fsn_fast_cfg* cfg, int B, long* out, int n) {
    if (!out || n < 21 || check_stream(cfg, B, 1) != FSN_OK) return -1;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);  // never dereferenced: only differences are taken
    Carver cv(base);
    const State st = state_carve(cv, cfg, B);
    const void* fields[16] = {st.enc0_h, st.enc0_c, st.enc1_h, st.enc1_c, st.dec0_h,  st.dec0_c,   st.dec1_h,  st.dec1_c,
                              st.bn_h[0], st.bn_c[0], st.bn_h[1], st.bn_c[1], st.mel_sum, st.unit_sum, st.partial, st.held};
    for (int i = 0; i < 16; ++i) out[i] = fields[i] ? (long)(static_cast<const char*>(fields[i]) - base) : -1;
    out[16] = fsn_round_up(B, 16);
    out[17] = (long)B * cfg->num_mels;
    out[18] = kEnc1H;
    out[19] = unit_width(cfg);
    out[20] = (long)fsn_round_up_sz(cv.off, 256);
    return 0;
}

// The order of a call (DESIGN "Fast FullSubNet as a stream"): the decoder of step t needs the bottleneck's output of a
// low-rate frame that may complete in this same call, so the bottleneck runs between the encoder and the decoder, on the
// n_low frames that complete in [steps_done, steps_done + k) - none of them: skipped, the held output serves.
extern "C" int fsn_fast_stream_step(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes, int steps_done,
                                    const float* mag, int B, int k, float* crm_out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_stream(cfg, B, k));
    FSN_REQUIRE(packed && state && mag && crm_out && workspace && steps_done >= 0, "NULL pointer argument / negative step count");
    FSN_REQUIRE((long)steps_done + k <= 2147483647L, "fast stream: step count beyond 2^31 - 1");
    if (state_bytes < fsn_fast_stream_state_bytes(cfg, B) || workspace_bytes < fsn_fast_stream_workspace_bytes(cfg, B, k)) {
        fsn_set_error("fast stream: state / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->F, Fp = fsn_fpad(F), M = cfg->num_mels, Bp = fsn_round_up(B, 16), N = B * M;
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const State st = state_carve(cs, cfg, B);
    const Ws w = ws_carve(cw, cfg, B, k);
    FsnFastStream g{};
    g.B = B;
    g.Bp = Bp;
    g.M = M;
    g.k = k;
    g.t0 = steps_done;
    g.shrink = cfg->shrink;
    g.n_mel = cfg->mel_neighbors;
    g.n_enc = cfg->enc_neighbors;
    g.W = unit_width(cfg);
    g.Wp = fsn_round_up(g.W, 16);
    g.Np = N;
    g.n_low = fsn_fast_stream_low_frames(steps_done, k, cfg->shrink);
    // 1. [B, 1, F, k] -> rows [k][Bp][Fp], the mel product, the mel norm (model.py:151-160; the caller appends the look-ahead)
    FSN_TRY(fsn_fast_spec_rows(mag, B, F, k, 0, w.rows, Bp, Fp, stream));
    FSN_TRY(run_linear(p.mel, pk, w.rows, Fp, w.mel, k * Bp, false, s));
    FSN_TRY(fsn_launch_fast_stream_mel_norm(w.mel, w.enc_in, st.mel_sum, g, s));
    // 2. the encoder pair on all k frames
    FSN_TRY(run_layer(p.enc0, pk, w.enc_in, M, k, Bp, w.hseq_a, st.enc0_h, st.enc0_c, w.gx, stream));
    FSN_TRY(run_layer(p.enc1, pk, w.hseq_a, kEnc0H, k, Bp, w.hseq_b, st.enc1_h, st.enc1_c, w.gx, stream));
    FSN_TRY(run_linear(p.enc_fc, pk, w.hseq_b, kEnc1H, w.enc, k * Bp, true, s));
    // 3. unit windows, block accumulation, the unit norm (model.py:163-178)
    FSN_TRY(fsn_launch_fast_stream_units(w.mel, w.enc, M, st.partial, st.unit_sum, w.units, g, s));
    // 4. the bottleneck on the low-rate frames that completed
    if (g.n_low > 0) {
        FSN_TRY(run_layer(p.bn[0], pk, w.units, g.Wp, g.n_low, N, w.bn_a, st.bn_h[0], st.bn_c[0], w.gx, stream));
        const float* top = w.bn_a;
        if (cfg->bn_layers == 2) {
            FSN_TRY(run_layer(p.bn[1], pk, w.bn_a, cfg->bn_hidden, g.n_low, N, w.bn_b, st.bn_h[1], st.bn_c[1], w.gx, stream));
            top = w.bn_b;
        }
        FSN_TRY(run_linear(p.bn_fc, pk, top, cfg->bn_hidden, w.slow, g.n_low * N, true, s));
    }
    // 5. - 6. the held output joined to the encoder's (model.py:180-190), the decoder pair on all k frames
    FSN_TRY(fsn_launch_fast_stream_decoder_input(w.enc, M, w.slow, st.held, w.dec_in, g, s));
    FSN_TRY(run_layer(p.dec0, pk, w.dec_in, 2 * M, k, Bp, w.hseq_a, st.dec0_h, st.dec0_c, w.gx, stream));
    FSN_TRY(run_layer(p.dec1, pk, w.hseq_a, kDecH, k, Bp, w.hseq_b, st.dec1_h, st.dec1_c, w.gx, stream));
    FSN_TRY(run_linear(p.dec_fc, pk, w.hseq_b, kDecH, w.out, k * Bp, false, s));
    // 7. the mask of all k steps (model.py:200-202 without the look-ahead slice)
    return fsn_fast_mask_out(w.out, 2L * F, k, B, Bp, F, 0, crm_out, stream);
}

// ---- recordings of any length under the offline norm: three passes over the segments -------------------------------------
// include/fsn_hip.h states the contract, DESIGN "Fast FullSubNet: recordings of any length" why three passes.  The state
// begins with fsn_fast_stream_step's layout: pass 2 carries the encoder pair's (h, c) there, pass 3 the bottleneck's and the
// decoder pair's, the open block's partial sum and the held output.  Behind it lie the two fp64 accumulators and the block
// sum of pass 2's statistic, a field of its own, so no field is cleared between the passes.
namespace {

struct SegState {
    State st;
    double *acc_mel, *acc_unit;
    float* stat_partial;
};
SegState seg_state_carve(Carver& cv, const fsn_fast_cfg* c, int B) {
    SegState g{};
    g.st = state_carve(cv, c, B);
    g.acc_mel = cv.take<double>((size_t)B);
    g.acc_unit = cv.take<double>((size_t)B);
    g.stat_partial = cv.take<float>((size_t)B * c->num_mels * unit_width(c));
    return g;
}
int check_segment(const fsn_fast_cfg* c, int B, int k) {
    FSN_REQUIRE(c, "NULL configuration");
    FSN_REQUIRE(c->norm == FSN_NORM_OFFLINE_LAPLACE,
                "fast segment: these entries are the offline norm's three passes (FSN_NORM_OFFLINE_LAPLACE); the causal norm "
                "needs one pass of fsn_fast_stream_step over the same segments");
    FSN_TRY(check_shape(c));
    FSN_REQUIRE(B >= 1 && B <= 4096 && k >= 1 && k <= 4096, "fast segment: batch %d / frames %d out of range", B, k);
    return FSN_OK;
}
size_t seg_state_bytes(const fsn_fast_cfg* c, int B) {
    Carver cv(nullptr);
    seg_state_carve(cv, c, B);
    return fsn_round_up_sz(cv.off, 256);
}
size_t seg_workspace_bytes(const fsn_fast_cfg* c, int B, int k) {
    Carver cv(nullptr);
    ws_carve(cv, c, B, k);  // the stream step's buffers: every pass uses a subset of them
    return fsn_round_up_sz(cv.off, 256);
}
int check_segment_call(const fsn_fast_cfg* c, int B, int k, const void* state, size_t state_bytes, int frames_done,
                       bool needs_workspace, const void* workspace, size_t workspace_bytes) {
    FSN_TRY(check_segment(c, B, k));
    FSN_REQUIRE(state && frames_done >= 0 && (!needs_workspace || workspace), "NULL pointer argument / negative step count");
    FSN_REQUIRE((long)frames_done + k <= 2147483647L, "fast segment: step count beyond 2^31 - 1");
    if (state_bytes < seg_state_bytes(c, B) || (needs_workspace && workspace_bytes < seg_workspace_bytes(c, B, k))) {
        fsn_set_error("fast segment: state / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}
FsnFastStream seg_geometry(const fsn_fast_cfg* c, int B, int k, int frames_done) {
    FsnFastStream g{};
    g.B = B;
    g.Bp = fsn_round_up(B, 16);
    g.M = c->num_mels;
    g.k = k;
    g.t0 = frames_done;
    g.shrink = c->shrink;
    g.n_mel = c->mel_neighbors;
    g.n_enc = c->enc_neighbors;
    g.W = unit_width(c);
    g.Wp = fsn_round_up(g.W, 16);
    g.Np = B * c->num_mels;
    g.n_low = fsn_fast_stream_low_frames(frames_done, k, c->shrink);
    return g;
}

}  // namespace

extern "C" size_t fsn_fast_segment_state_bytes(const fsn_fast_cfg* cfg, int B) {
    if (check_segment(cfg, B, 1) != FSN_OK) return 0;
    return seg_state_bytes(cfg, B);
}

extern "C" size_t fsn_fast_segment_workspace_bytes(const fsn_fast_cfg* cfg, int B, int k) {
    if (check_segment(cfg, B, k) != FSN_OK) return 0;
    return seg_workspace_bytes(cfg, B, k);
}

extern "C" int fsn_debug_fast_segment_state_layout(const fsn_fast_cfg* cfg, int B, long* out, int n) {
    if (!out || n < 25 || check_segment(cfg, B, 1) != FSN_OK) return -1;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);  // never dereferenced: only differences are taken
    Carver cv(base);
    const SegState g = seg_state_carve(cv, cfg, B);
    const State& st = g.st;
    const void* fields[19] = {st.enc0_h,  st.enc0_c,  st.enc1_h,  st.enc1_c,  st.dec0_h,  st.dec0_c,   st.dec1_h,
                              st.dec1_c,  st.bn_h[0], st.bn_c[0], st.bn_h[1], st.bn_c[1], st.mel_sum,  st.unit_sum,
                              st.partial, st.held,    g.acc_mel,  g.acc_unit, g.stat_partial};
    for (int i = 0; i < 19; ++i) out[i] = fields[i] ? (long)(static_cast<const char*>(fields[i]) - base) : -1;
    Carver stream_only(nullptr);
    state_carve(stream_only, cfg, B);
    out[19] = (long)stream_only.off;  // where fsn_fast_stream_step's fields end
    out[20] = fsn_round_up(B, 16);
    out[21] = (long)B * cfg->num_mels;
    out[22] = kEnc1H;
    out[23] = unit_width(cfg);
    out[24] = (long)fsn_round_up_sz(cv.off, 256);
    return 0;
}

// pass 1: the mel spectrum of the segment into the caller's plane, its frames' sums into the accumulator
extern "C" int fsn_fast_segment_stats(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes, const float* mag,
                                      int B, int k, float* mel_out, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, k, state, state_bytes, 0, true, workspace, workspace_bytes));
    FSN_REQUIRE(packed && mag && mel_out, "NULL pointer argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->F, Fp = fsn_fpad(F), Bp = fsn_round_up(B, 16);
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const SegState st = seg_state_carve(cs, cfg, B);
    const Ws w = ws_carve(cw, cfg, B, k);
    const FsnFastStream g = seg_geometry(cfg, B, k, 0);
    // rows beyond B and columns beyond F are zeros, so the padding rows of mel_out are
    FSN_TRY(fsn_fast_spec_rows(mag, B, F, k, 0, w.rows, Bp, Fp, stream));
    FSN_TRY(run_linear(p.mel, pk, w.rows, Fp, mel_out, k * Bp, false, s));
    return fsn_launch_fast_segment_mel_stat(mel_out, st.acc_mel, g, s);
}

// pass 2: the encoder pair on the normalised mel spectrum, and the statistic of the down-sampled unit tensor
extern "C" int fsn_fast_segment_encoder(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                        int frames_done, const int* total_frames, const float* mel, int B, int k, float* enc_out,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, k, state, state_bytes, frames_done, true, workspace, workspace_bytes));
    FSN_REQUIRE(packed && total_frames && mel && enc_out, "NULL pointer argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int M = cfg->num_mels, Bp = fsn_round_up(B, 16);
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const SegState g = seg_state_carve(cs, cfg, B);
    const State& st = g.st;
    const Ws w = ws_carve(cw, cfg, B, k);
    const FsnFastStream a = seg_geometry(cfg, B, k, frames_done);
    FSN_TRY(fsn_launch_fast_segment_mel_norm(mel, w.enc_in, g.acc_mel, total_frames, a, s));
    FSN_TRY(run_layer(p.enc0, pk, w.enc_in, M, k, Bp, w.hseq_a, st.enc0_h, st.enc0_c, w.gx, stream));
    FSN_TRY(run_layer(p.enc1, pk, w.hseq_a, kEnc0H, k, Bp, w.hseq_b, st.enc1_h, st.enc1_c, w.gx, stream));
    FSN_TRY(run_linear(p.enc_fc, pk, w.hseq_b, kEnc1H, enc_out, k * Bp, true, s));
    return fsn_launch_fast_segment_units(false, mel, enc_out, M, g.stat_partial, g.acc_unit, total_frames, nullptr, a, s);
}

// pass 3: fsn_fast_stream_step from its stage 3 on, with the one divisor of the finished statistic
extern "C" int fsn_fast_segment_decoder(const fsn_fast_cfg* cfg, const void* packed, void* state, size_t state_bytes,
                                        int frames_done, const int* total_frames, const float* mel, const float* enc, int B, int k,
                                        float* crm_out, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, k, state, state_bytes, frames_done, true, workspace, workspace_bytes));
    FSN_REQUIRE(packed && total_frames && mel && enc && crm_out, "NULL pointer argument");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->F, M = cfg->num_mels, Bp = fsn_round_up(B, 16), N = B * M;
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cs(state), cw(workspace);
    const SegState g = seg_state_carve(cs, cfg, B);
    const State& st = g.st;
    const Ws w = ws_carve(cw, cfg, B, k);
    const FsnFastStream a = seg_geometry(cfg, B, k, frames_done);
    FSN_TRY(fsn_launch_fast_segment_units(true, mel, enc, M, st.partial, g.acc_unit, total_frames, w.units, a, s));
    if (a.n_low > 0) {
        FSN_TRY(run_layer(p.bn[0], pk, w.units, a.Wp, a.n_low, N, w.bn_a, st.bn_h[0], st.bn_c[0], w.gx, stream));
        const float* top = w.bn_a;
        if (cfg->bn_layers == 2) {
            FSN_TRY(run_layer(p.bn[1], pk, w.bn_a, cfg->bn_hidden, a.n_low, N, w.bn_b, st.bn_h[1], st.bn_c[1], w.gx, stream));
            top = w.bn_b;
        }
        FSN_TRY(run_linear(p.bn_fc, pk, top, cfg->bn_hidden, w.slow, a.n_low * N, true, s));
    }
    FSN_TRY(fsn_launch_fast_stream_decoder_input(enc, M, w.slow, st.held, w.dec_in, a, s));
    FSN_TRY(run_layer(p.dec0, pk, w.dec_in, 2 * M, k, Bp, w.hseq_a, st.dec0_h, st.dec0_c, w.gx, stream));
    FSN_TRY(run_layer(p.dec1, pk, w.hseq_a, kDecH, k, Bp, w.hseq_b, st.dec1_h, st.dec1_c, w.gx, stream));
    FSN_TRY(run_linear(p.dec_fc, pk, w.hseq_b, kDecH, w.out, k * Bp, false, s));
    return fsn_fast_mask_out(w.out, 2L * F, k, B, Bp, F, 0, crm_out, stream);
}

extern "C" int fsn_fast_segment_divisors(const fsn_fast_cfg* cfg, const void* state, size_t state_bytes, const int* total_frames,
                                         int B, float* den_mel, float* den_unit, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, B, 1, state, state_bytes, 0, false, nullptr, 0));
    FSN_REQUIRE(total_frames && den_mel && den_unit, "NULL pointer argument");
    Carver cs(const_cast<void*>(state));
    const SegState g = seg_state_carve(cs, cfg, B);
    return fsn_launch_fast_segment_divisors(g.acc_mel, g.acc_unit, total_frames, den_mel, den_unit, B, cfg->shrink, unit_width(cfg),
                                            static_cast<hipStream_t>(stream));
}

// ---- streaming pool: the same step over a subset of the slots of a pool, each slot at its own block phase ---------------------
// State: one record per slot (FsnFastPoolLayout, fsn_common.h).  A window of k consecutive steps holds lo = k / shrink or hi =
// ceil(k / shrink) multiples of shrink, so every listed slot completes lo or hi low-rate frames; the caller lists the ones
// that complete hi first (n_long of them), which makes the bottleneck's rows of low-rate frame ordinal lo a prefix of its
// compact rows: the bottleneck is T = lo on all n 64 rows, then T = 1 on the first n_long 64 rows of the same (h, c) tiles.
// The launches are sized from n_long on the host; the record's own count decides every piece of arithmetic, and a kernel at
// the head of the call checks the one against the other (fast_stream_pool_kernels.hip).
namespace {

FsnFastPoolLayout pool_layout(const fsn_fast_cfg* c, int look_ahead) {
    return fsn_fast_pool_layout(c->F, c->bn_hidden, c->bn_layers, unit_width(c), look_ahead);
}
int check_pool(const fsn_fast_cfg* c, int look_ahead, int capacity) {
    FSN_TRY(check_cfg(c));
    FSN_REQUIRE(look_ahead >= 0 && look_ahead <= 64, "fast streaming pool: look_ahead %d out of range [0, 64]", look_ahead);
    FSN_REQUIRE(capacity >= 1 && capacity <= 4096, "fast streaming pool: capacity %d out of range [1, 4096]", capacity);
    return FSN_OK;
}
int check_pool_call(const fsn_fast_cfg* c, int look_ahead, const void* state, size_t state_bytes, int capacity, const int* slots,
                    int n) {
    FSN_TRY(check_pool(c, look_ahead, capacity));
    FSN_REQUIRE(state && slots, "NULL pointer argument");
    FSN_REQUIRE(n >= 1 && n <= capacity, "fast streaming pool: %d slots listed, need 1 .. capacity = %d", n, capacity);
    if (state_bytes < (size_t)capacity * pool_layout(c, look_ahead).slot_bytes) {
        fsn_set_error("fast streaming pool: state buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}
struct PoolWs {
    unsigned* status;
    FsnFastPoolTiles t;
};
PoolWs pool_ws_carve(Carver& cv, const fsn_fast_cfg* c, int n) {
    PoolWs p{};
    const size_t Bp = fsn_round_up(n, 16), N = (size_t)n * c->num_mels;
    p.status = cv.take<unsigned>(64);
    for (int a = 0; a < 8; ++a) p.t.pair[a] = cv.take<float>(Bp * fsn_fast_pair_h(a / 2));
    for (int l = 0; l < c->bn_layers; ++l)
        for (int a = 0; a < 2; ++a) p.t.bn[l][a] = cv.take<float>(N * c->bn_hidden);
    return p;
}
// the transform entries are built for the 512 / 256 transform, like fsn_stream_pool_analysis
int check_pool_fft(const fsn_fast_cfg* c, int n_fft, int hop) {
    FSN_REQUIRE(n_fft == 512 && hop == 256, "fast streaming pool: only n_fft = 512, hop = 256 is built (got %d/%d)", n_fft, hop);
    FSN_REQUIRE(c->F == n_fft / 2 + 1, "F %d != n_fft/2+1", c->F);
    return FSN_OK;
}

}  // namespace

extern "C" size_t fsn_fast_stream_pool_state_bytes(const fsn_fast_cfg* cfg, int look_ahead, int capacity) {
    if (check_pool(cfg, look_ahead, capacity) != FSN_OK) return 0;
    return (size_t)capacity * pool_layout(cfg, look_ahead).slot_bytes;
}

extern "C" size_t fsn_fast_stream_pool_workspace_bytes(const fsn_fast_cfg* cfg, int n, int k) {
    if (check_stream(cfg, n, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    ws_carve(cv, cfg, n, k);  // sized for hi = ceil(k / shrink) low-rate frames of all rows
    pool_ws_carve(cv, cfg, n);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_fast_stream_pool_reset(const fsn_fast_cfg* cfg, int look_ahead, void* state, size_t state_bytes, int capacity,
                                          const int* slots, int n, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, look_ahead, state, state_bytes, capacity, slots, n));
    // the FullSubNet pool's reset kernel: it reads slot_bytes alone
    return fsn_launch_pool_reset(state, fsn_fast_pool_transform_layout(pool_layout(cfg, look_ahead)), capacity, slots, n,
                                 static_cast<hipStream_t>(stream));
}

extern "C" int fsn_fast_stream_pool_step(const fsn_fast_cfg* cfg, int look_ahead, const void* packed, void* state,
                                         size_t state_bytes, int capacity, const int* slots, int n, int n_long, const float* mag,
                                         int k, float* crm_out, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, look_ahead, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_stream(cfg, n, k));
    FSN_REQUIRE(packed && mag && crm_out && workspace, "NULL pointer argument");
    FSN_REQUIRE(n_long >= 0 && n_long <= n, "fast streaming pool: n_long %d outside 0 .. n = %d", n_long, n);
    FSN_REQUIRE(k % cfg->shrink != 0 || n_long == n,
                "fast streaming pool: shrink %d divides k = %d, so every slot completes k / shrink frames: n_long must be n = %d (got %d)",
                cfg->shrink, k, n, n_long);
    if (workspace_bytes < fsn_fast_stream_pool_workspace_bytes(cfg, n, k)) {
        fsn_set_error("fast streaming pool: workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->F, Fp = fsn_fpad(F), M = cfg->num_mels, Bp = fsn_round_up(n, 16), N = n * M, H = cfg->bn_hidden;
    const Packed p = packed_layout(cfg);
    const float* pk = static_cast<const float*>(packed);
    Carver cw(workspace);
    const Ws w = ws_carve(cw, cfg, n, k);
    const PoolWs pw = pool_ws_carve(cw, cfg, n);
    const FsnFastPoolTiles& t = pw.t;
    FsnFastPool g{};
    g.state = static_cast<char*>(state);
    g.L = pool_layout(cfg, look_ahead);
    g.slots = slots;
    g.status = pw.status;
    g.capacity = capacity;
    g.n = n;
    g.n_long = n_long;
    g.k = k;
    g.Bp = Bp;
    g.Np = N;
    g.shrink = cfg->shrink;
    g.n_mel = cfg->mel_neighbors;
    g.n_enc = cfg->enc_neighbors;
    g.W = unit_width(cfg);
    g.Wp = fsn_round_up(g.W, 16);
    g.lo = k / cfg->shrink;
    g.hi = max_low_frames(k, cfg->shrink);
    const int lo = g.lo, extra = g.hi > g.lo ? n_long * M : 0;  // the rows of low-rate frame ordinal lo
    // 0. the caller's order against the records' own counts -> the status word every record-writing kernel reads
    FSN_TRY(fsn_launch_fast_pool_check(g, s));
    // 1. [n, 1, F, k] -> rows [k][Bp][Fp], the mel product, the mel norm with each row's own sum and count
    FSN_TRY(fsn_fast_spec_rows(mag, n, F, k, 0, w.rows, Bp, Fp, stream));
    FSN_TRY(run_linear(p.mel, pk, w.rows, Fp, w.mel, k * Bp, false, s));
    FSN_TRY(fsn_launch_fast_pool_gather_pairs(g, t, s));
    FSN_TRY(fsn_launch_fast_pool_mel_norm(w.mel, w.enc_in, g, s));
    // 2. the encoder pair on all k frames
    FSN_TRY(run_layer(p.enc0, pk, w.enc_in, M, k, Bp, w.hseq_a, t.pair[0], t.pair[1], w.gx, stream));
    FSN_TRY(run_layer(p.enc1, pk, w.hseq_a, kEnc0H, k, Bp, w.hseq_b, t.pair[2], t.pair[3], w.gx, stream));
    FSN_TRY(run_linear(p.enc_fc, pk, w.hseq_b, kEnc1H, w.enc, k * Bp, true, s));
    // 3. unit windows, block accumulation and the unit norm, each row from its own phase
    FSN_TRY(fsn_launch_fast_pool_units(w.mel, w.enc, M, w.units, g, s));
    // 4. the bottleneck: lo steps on all rows, one more on the long rows' prefix; none of it when no listed slot is due
    if (lo > 0 || extra > 0) {
        const int slots_run = lo > 0 ? n : n_long;
        FSN_TRY(fsn_launch_fast_pool_gather_bn(g, t, slots_run, s));
        auto bn_layer = [&](const Layer& l, const float* x, long ldx, float* hseq, float* h, float* c) {
            if (lo > 0) FSN_TRY(run_layer(l, pk, x, ldx, lo, N, hseq, h, c, w.gx, stream));
            if (extra > 0)
                FSN_TRY(run_layer(l, pk, x + (size_t)lo * N * ldx, ldx, 1, extra, hseq + (size_t)lo * N * H, h, c, w.gx, stream));
            return (int)FSN_OK;
        };
        FSN_TRY(bn_layer(p.bn[0], w.units, g.Wp, w.bn_a, t.bn[0][0], t.bn[0][1]));
        const float* top = w.bn_a;
        if (cfg->bn_layers == 2) {
            FSN_TRY(bn_layer(p.bn[1], w.bn_a, H, w.bn_b, t.bn[1][0], t.bn[1][1]));
            top = w.bn_b;
        }
        FSN_TRY(run_linear(p.bn_fc, pk, top, H, w.slow, lo * N + extra, true, s));
        FSN_TRY(fsn_launch_fast_pool_scatter_bn(g, t, slots_run, s));
    }
    // 5. - 6. the held output joined to the encoder's, the decoder pair on all k frames
    FSN_TRY(fsn_launch_fast_pool_decoder_input(w.enc, M, w.slow, w.dec_in, g, s));
    FSN_TRY(run_layer(p.dec0, pk, w.dec_in, 2 * M, k, Bp, w.hseq_a, t.pair[4], t.pair[5], w.gx, stream));
    FSN_TRY(run_layer(p.dec1, pk, w.hseq_a, kDecH, k, Bp, w.hseq_b, t.pair[6], t.pair[7], w.gx, stream));
    FSN_TRY(run_linear(p.dec_fc, pk, w.hseq_b, kDecH, w.out, k * Bp, false, s));
    // 7. the mask of all k steps; NaN instead when the order check failed
    FSN_TRY(fsn_fast_mask_out(w.out, 2L * F, k, n, Bp, F, 0, crm_out, stream));
    FSN_TRY(fsn_launch_poison_if(g.status, crm_out, (size_t)n * 2 * F * k, s));
    // last: it advances the listed slots' step counts
    return fsn_launch_fast_pool_scatter_pairs(g, t, s);
}

extern "C" int fsn_fast_stream_pool_analysis(const fsn_fast_cfg* cfg, int look_ahead, void* state, size_t state_bytes,
                                             int capacity, const int* slots, int n, const float* hops, const float* prime,
                                             const int* frame_no, int n_fft, int hop, const float* window, float* mag,
                                             void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, look_ahead, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_pool_fft(cfg, n_fft, hop));
    FSN_REQUIRE(hops && frame_no && window && mag, "NULL pointer argument");
    return fsn_launch_pool_analysis(state, fsn_fast_pool_transform_layout(pool_layout(cfg, look_ahead)), capacity, slots, n, hops,
                                    prime, frame_no, window, mag, static_cast<hipStream_t>(stream));
}

extern "C" int fsn_fast_stream_pool_synthesis(const fsn_fast_cfg* cfg, int look_ahead, void* state, size_t state_bytes,
                                              int capacity, const int* slots, int n, const float* crm, int k,
                                              const int* first_frame, const int* tail_samples, int n_fft, int hop,
                                              const float* window, float* out, void* workspace, size_t workspace_bytes,
                                              void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, look_ahead, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_pool_fft(cfg, n_fft, hop));
    FSN_REQUIRE(crm && first_frame && tail_samples && window && out && workspace, "NULL pointer argument");
    FSN_REQUIRE(k >= 1 && k <= 4096, "fast streaming pool: frames %d out of range", k);
    if (workspace_bytes < (size_t)n * k * n_fft * sizeof(float)) {
        fsn_set_error("fast streaming pool: synthesis workspace too small (n k n_fft floats)");
        return FSN_ERR_WORKSPACE;
    }
    return fsn_launch_pool_synthesis(state, fsn_fast_pool_transform_layout(pool_layout(cfg, look_ahead)), capacity, slots, n, crm,
                                     k, first_frame, tail_samples, window, static_cast<float*>(workspace), out,
                                     static_cast<hipStream_t>(stream));
}

// test hook (host only): where the fields of one record lie, from the function the entries lay it out with
extern "C" int fsn_debug_fast_stream_pool_layout(const fsn_fast_cfg* cfg, int look_ahead, long* out, int n) {
    if (!out || n < 28 || check_pool(cfg, look_ahead, 1) != FSN_OK) return -1;
    const FsnFastPoolLayout L = pool_layout(cfg, look_ahead);
    for (int a = 0; a < 8; ++a) out[a] = (long)L.pair[a];
    for (int l = 0; l < 2; ++l)
        for (int a = 0; a < 2; ++a) out[8 + 2 * l + a] = l < L.layers ? (long)L.bn[l][a] : -1;
    const size_t rest[10] = {L.mel_sum, L.unit_sum, L.partial, L.held, L.steps, L.in_tail, L.ola_tail, L.ring_re, L.ring_im, L.slot_bytes};
    for (int i = 0; i < 10; ++i) out[12 + i] = (long)rest[i];
    const int dims[6] = {L.F, L.FP, L.R, L.H, L.layers, L.W};
    for (int i = 0; i < 6; ++i) out[22 + i] = dims[i];
    return 0;
}
