// C ABI of libfsn_hip.so, nn.GRU: two stacked layers on the full-band chain kernel, and the single layer's forward
// (inference / training) and BPTT.
#include "fsn_api_internal.h"

// ---- two stacked GRU layers of equal width, few rows: ONE persistent launch of the chain kernel ---------------------------
// (audio_zen/model/module/sequence_model.py:59-66 with num_layers = 2: the full-band model of a GRU FullSubNet, B <= 64 rows.)
// nn.GRU's weights are expanded to the four-gate cell r | z | nx | nh (zero blocks where a gate has no input / no recurrent
// part) and take the LSTM chain's path unchanged: projection GEMM of layer 0, fb_chain_kernel<.., CELL = 1>.
extern "C" int fsn_gru2_forward_supported(int T, int N, int H) { return T >= 1 && lstm2_on_chain(T, N, H) ? 1 : 0; }
extern "C" size_t fsn_gru2_fwd_workspace_bytes(int T, int N, int I, int H) {
    if (T < 1 || N < 16 || N % 16 || I < 1 || H < 64) return 0;
    const size_t Ipad = fsn_round_up(I, 16), G = 4 * (size_t)H;
    Carver cv(nullptr);
    cv.take<float>(2 * (G * Ipad + 3 * G * H));  // the expanded matrices and their fragment-order copies
    cv.take<float>(2 * G);                       // b4 of both layers
    cv.take<float>((size_t)T * N * G);           // layer-0 projection
    cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
    cv.take<unsigned>(fsn_fb_chain_flag_words());
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" int fsn_gru2_forward(const float* x, long ldx, const float* w_ih0, const float* w_hh0, const float* b_ih0,
                                const float* b_hh0, const float* w_ih1, const float* w_hh1, const float* b_ih1,
                                const float* b_hh1, int T, int N, int I, int H, float* hseq1, void* workspace,
                                size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(x && w_ih0 && w_hh0 && b_ih0 && b_hh0 && w_ih1 && w_hh1 && b_ih1 && b_hh1 && hseq1 && workspace, "NULL pointer argument");
    FSN_REQUIRE(fsn_gru2_forward_supported(T, N, H), "gru2 forward: built for H = 384 / 512 twice, up to 64 rows and 4095 steps on a "
                                                     "device that holds the chain's grid (fsn_gru2_forward_supported)");
    if (workspace_bytes < fsn_gru2_fwd_workspace_bytes(T, N, I, H)) {
        fsn_set_error("gru2 forward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = 4 * H;
    Carver cv(workspace);
    float* e = cv.take<float>(2 * ((size_t)G * Ipad + (size_t)3 * G * H));
    float *wih0_4 = e, *whh0_4 = wih0_4 + (size_t)G * I, *wih1_4 = whh0_4 + (size_t)G * H, *whh1_4 = wih1_4 + (size_t)G * H;
    float* pk = e + (size_t)G * Ipad + (size_t)3 * G * H;
    float *wih0_p = pk, *whh0_p = wih0_p + (size_t)G * Ipad, *wih1_p = whh0_p + (size_t)G * H, *whh1_p = wih1_p + (size_t)G * H;
    float* b0 = cv.take<float>((size_t)2 * G);
    float* b1 = b0 + G;
    float* gx = cv.take<float>((size_t)T * N * G);
    float* exchange = cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
    unsigned* flags = cv.take<unsigned>(fsn_fb_chain_flag_words());
    FSN_TRY(fsn_launch_gru_expand4(w_ih0, w_hh0, b_ih0, b_hh0, wih0_4, whh0_4, b0, I, H, s));
    FSN_TRY(fsn_launch_gru_expand4(w_ih1, w_hh1, b_ih1, b_hh1, wih1_4, whh1_4, b1, H, H, s));
    FSN_TRY(fsn_launch_pack(wih0_4, wih0_p, G, I, G, Ipad, s));
    FSN_TRY(fsn_launch_pack(whh0_4, whh0_p, G, H, G, H, s));
    FSN_TRY(fsn_launch_pack(wih1_4, wih1_p, G, H, G, H, s));
    FSN_TRY(fsn_launch_pack(whh1_4, whh1_p, G, H, G, H, s));
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), wih0_p, gemm_c_frag(gx, b0), T * (N / 16), G / 16, Ipad / 16, s));
    FSN_PERSIST_BEGIN(s);
    FSN_TRY(fsn_launch_fb_chain(gx, whh0_p, wih1_p, whh1_p, b1, exchange, flags, hseq1, T, N, H, s, nullptr, nullptr, nullptr, 1));
    return fsn_launch_poison_if(flags + fsn_fb_chain_status_word(), hseq1, (size_t)T * N * H, s);
}

// ---- nn.GRU layer (sequence_model.py:59-66): forward (inference / training) + BPTT -----------------
extern "C" size_t fsn_gru_layer_save_bytes(int T, int N, int H) {
    return fsn_round_up_sz((size_t)T * N * 4 * H * sizeof(float), 256);  // r | z | n | hn
}
// Many rows in inference (the sub-band model of a GRU FullSubNet: B F rows, audio_zen/model/module/sequence_model.py:59-66
// under fullsubnet/model.py:121-128): the layer runs on the LSTM's persistent kernels with the GRU written as a four-gate
// cell (lstm_cell.h) - lstm_rec_in_kernel for a narrow row-major input (<= 32 columns: the projection is
// formed inside), lstm_rec_x_kernel for the layer above an equally wide one (input = its hidden sequence, no projection
// GEMM, no gx round trip).  Whole rounds of 2 - 4 row tiles per workgroup; the few left-over tiles advance step by step
// on the auxiliary stream beside the persistent launch, on compact copies of their rows.
struct GruPlan {
    int rt, main_wgs, left_tiles;
};
static GruPlan gru_layer_plan(int N, int I, long ldx, int H) {
    GruPlan p{0, 0, N / 16};
    const int Ipad = fsn_round_up(I, 16);
    if (H != 384 || !((Ipad <= 32 && (ldx <= 0 || ldx >= Ipad)) || (I == H && (ldx <= 0 || ldx == H)))) return p;
    const int cus = plan_cus();
    const int tiles = N / 16;
    // Few rows per CU: the step launches spread a step over more workgroups.  The persistent kernels take 2 - 4 row tiles per
    // workgroup, so up to 2 x CUs tiles they leave CUs idle and cost what 2 x CUs tiles cost (GRU FullSubNet, 190 frames:
    // 31.5 - 32.9 ms from 16 to 32 utterances; step by step 1.77 ms per utterance: 26.5 ms at 15, ~30 at 17): from 9/8 x CUs on
    if (tiles < cus + cus / 8) return p;
    long best = -1;
    for (int rt = 4; rt >= 2; --rt) {
        // whole rounds of rt tiles on every CU, or ONE round of fewer workgroups; a left-over tile costs about a
        // hundredth of a tile of a resident workgroup (layer_plan's measure)
        int wgs = 0;
        const int rounds = tiles / (cus * rt);
        if (rounds >= 1) wgs = rounds * cus;
        else if (tiles / rt <= cus) wgs = tiles / rt;
        if (wgs < 1) continue;
        const int left = tiles - wgs * rt;
        const long cost = (long)((wgs + cus - 1) / cus) * rt * 100 + left;
        if (best < 0 || cost < best) {
            best = cost;
            p = GruPlan{rt, wgs, left};
        }
    }
    return p;
}
static size_t gru_layer_step_workspace_bytes(int T, int N, int I, int H) {
    Carver cv(nullptr);
    cv.take<float>((size_t)3 * H * fsn_round_up(I, 16));
    cv.take<float>((size_t)3 * H * H);
    cv.take<float>((size_t)3 * H);
    cv.take<float>((size_t)T * N * 3 * H);
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" size_t fsn_gru_layer_fwd_workspace_bytes(int T, int N, int I, int H) {
    if (T < 1 || N < 16 || I < 1 || H < 64) return 0;
    const size_t Ipad = fsn_round_up(I, 16), G4 = 4 * (size_t)H;
    const GruPlan p = gru_layer_plan(N, I, 0, H);
    Carver cv(nullptr);
    if (p.main_wgs > 0) {  // the persistent form's own buffers first, the step form's region (left-over rows) behind them
        cv.take<float>(G4 * Ipad + G4 * H);  // the four-gate matrices as expanded ...
        cv.take<float>(G4 * Ipad + G4 * H);  // ... and in fragment order, W_hh right behind W_ih
        cv.take<float>(G4);
        cv.take<float>((size_t)T * p.left_tiles * 16 * Ipad);
        cv.take<float>((size_t)T * p.left_tiles * 16 * H);
    }
    cv.take<char>(gru_layer_step_workspace_bytes(T, N, I, H));
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" int fsn_gru_layer_is_persistent(int T, int N, int I, long ldx, int H) {
    return T >= 1 && N >= 16 && N % 16 == 0 && I >= 1 && gru_layer_plan(N, I, ldx, H).main_wgs > 0 ? 1 : 0;
}

// The step form in two halves: weights re-tiled + input projection of all steps (one GEMM), then the T dependent step launches
// (gru_step_kernel: 32 registers, 12 KB of LDS - it fits beside a resident workgroup of the persistent kernels).
struct GruStepBufs {
    float *whh_p, *gx;
};
static int gru_layer_steps_prepare(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                   const float* b_hh, int T, int N, int I, int H, void* workspace, hipStream_t s, GruStepBufs* out) {
    const int Ipad = fsn_round_up(I, 16), G = 3 * H;
    Carver cv(workspace);
    float* wih_p = cv.take<float>((size_t)G * Ipad);
    float* whh_p = cv.take<float>((size_t)G * H);
    float* bias = cv.take<float>((size_t)G);
    float* gx = cv.take<float>((size_t)T * N * G);
    FSN_TRY(fsn_launch_pack(w_ih, wih_p, G, I, G, Ipad, s));
    FSN_TRY(fsn_launch_pack(w_hh, whh_p, G, H, G, H, s));
    // bias of the projection: b_ih everywhere + b_hh for r and z (b_hn stays inside r * (W_hn h + b_hn))
    FSN_TRY(fsn_launch_bias_sum(b_ih, nullptr, bias, G, G, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih, b_hh, bias, 2 * H, 2 * H, s));
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), wih_p, gemm_c_frag(gx, bias), T * (N / 16), G / 16, Ipad / 16, s));
    out->whh_p = whh_p;
    out->gx = gx;
    return FSN_OK;
}
static int gru_layer_steps_run(const GruStepBufs& b, const float* b_hh, int T, int N, int H, float* hseq, float* sv, hipStream_t s,
                               int beside_persistent = 0) {
    const size_t step = (size_t)N * H;
    for (int t = 0; t < T; ++t)
        FSN_TRY(fsn_launch_gru_step(b.gx, b.whh_p, b_hh + 2 * H, t ? hseq + (t - 1) * step : hseq, hseq + t * step,
                                    sv ? sv + (size_t)t * N * 4 * H : nullptr, (long)t * (N / 16), N / 16, H, t == 0, s,
                                    beside_persistent));
    return FSN_OK;
}
static int gru_layer_forward_steps(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                   const float* b_hh, int T, int N, int I, int H, float* hseq, float* sv, void* workspace,
                                   hipStream_t s) {
    GruStepBufs b{};
    FSN_TRY(gru_layer_steps_prepare(x, ldx, w_ih, w_hh, b_ih, b_hh, T, N, I, H, workspace, s, &b));
    return gru_layer_steps_run(b, b_hh, T, N, H, hseq, sv, s);
}

static int gru_layer_forward_persistent(const GruPlan& p, const float* x, long ldx, const float* w_ih, const float* w_hh,
                                        const float* b_ih, const float* b_hh, int T, int N, int I, int H, float* hseq,
                                        void* workspace, hipStream_t s) {
    const int Ipad = fsn_round_up(I, 16), G4 = 4 * H;
    const int left = p.left_tiles * 16, main_rows = N - left;
    Carver cv(workspace);
    float* w4 = cv.take<float>((size_t)G4 * Ipad + (size_t)G4 * H);
    float* w4p = cv.take<float>((size_t)G4 * Ipad + (size_t)G4 * H);
    float* b4 = cv.take<float>((size_t)G4);
    float* x_left = cv.take<float>((size_t)T * left * Ipad);
    float* h_left = cv.take<float>((size_t)T * left * H);
    void* step_ws = cv.take<char>(0);
    float *wih4 = w4, *whh4 = w4 + (size_t)G4 * I, *wih4_p = w4p, *whh4_p = w4p + (size_t)G4 * Ipad;
    FSN_TRY(fsn_launch_gru_expand4(w_ih, w_hh, b_ih, b_hh, wih4, whh4, b4, I, H, s, 1));
    FSN_TRY(fsn_launch_pack(wih4, wih4_p, G4, I, G4, Ipad, s));
    FSN_TRY(fsn_launch_pack(whh4, whh4_p, G4, H, G4, H, s));
    hipStream_t ls = s;
    GruStepBufs sb{};
    if (left > 0) {
        // rows [main_rows, N) of every step as compact [T][left] matrices (columns [0, Ipad) of a row; one 2-D copy when the
        // rows are exactly that wide, one per step otherwise) and their input projection - on `s`, AHEAD of the persistent
        // launch: the projection GEMM's workgroups (160 registers, 96 KB of LDS) do not fit beside a resident workgroup of it
        // and would wait for the whole launch (measured: the step launches then ran after it, +2.7 ms per batch of 64)
        FSN_TRY(gather_step_rows(x_left, x, ldx, T, N, main_rows, left, Ipad, s));
        FSN_TRY(gru_layer_steps_prepare(x_left, Ipad, w_ih, w_hh, b_ih, b_hh, T, left, I, H, step_ws, s, &sb));
        FSN_TRY(aux_fork(s, &ls));
    }
    if (Ipad <= 32) {
        const FsnSbInput xin = sb_input_rows(x, ldx, N, main_rows, Ipad / 16, wih4_p, b4);
        FSN_TRY(fsn_launch_lstm_rec_in(&xin, whh4_p, hseq, T, N, H, p.rt, p.main_wgs, s, 1));
    } else {
        FSN_TRY(fsn_launch_lstm_rec_x(x, wih4_p, whh4_p, b4, T, N, H, p.rt, p.main_wgs, s, nullptr, hseq, 1));
    }
    if (left > 0) {
        // the left-over rows' T step launches beside the persistent launch, then back into rows [main_rows, N) of hseq
        FSN_TRY(gru_layer_steps_run(sb, b_hh, T, left, H, h_left, nullptr, ls, 1));
        FSN_TRY(scatter_step_rows(hseq, H, h_left, T, N, main_rows, left, H, ls));
        FSN_TRY(aux_join(s));
    }
    return FSN_OK;
}

extern "C" int fsn_gru_layer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                     const float* b_hh, int T, int N, int I, int H, float* hseq, void* save,
                                     size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && hseq && workspace, "NULL pointer argument");
    if ((save && save_bytes < fsn_gru_layer_save_bytes(T, N, H)) ||
        workspace_bytes < fsn_gru_layer_fwd_workspace_bytes(T, N, I, H)) {
        fsn_set_error("gru layer forward: save / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!save) {
        const GruPlan p = gru_layer_plan(N, I, ldx, H);
        if (p.main_wgs > 0) return gru_layer_forward_persistent(p, x, ldx, w_ih, w_hh, b_ih, b_hh, T, N, I, H, hseq, workspace, s);
    }
    return gru_layer_forward_steps(x, ldx, w_ih, w_hh, b_ih, b_hh, T, N, I, H, hseq, static_cast<float*>(save), workspace, s);
}

// Streaming form (chunked / frame-by-frame inference with carried state): T more steps from h_state [N][H], which is
// updated in place (nn.GRU(x, h_0) is the analogue).  Same kernels and workspace as the offline forward.
extern "C" int fsn_gru_layer_forward_state(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                           const float* b_hh, int T, int N, int I, int H, float* hseq, float* h_state,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && hseq && h_state && workspace, "NULL pointer argument");
    if (workspace_bytes < fsn_gru_layer_fwd_workspace_bytes(T, N, I, H)) {
        fsn_set_error("gru layer forward (state): workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = 3 * H;
    Carver cv(workspace);
    float* wih_p = cv.take<float>((size_t)G * Ipad);
    float* whh_p = cv.take<float>((size_t)G * H);
    float* bias = cv.take<float>((size_t)G);
    float* gx = cv.take<float>((size_t)T * N * G);
    FSN_TRY(fsn_launch_pack(w_ih, wih_p, G, I, G, Ipad, s));
    FSN_TRY(fsn_launch_pack(w_hh, whh_p, G, H, G, H, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih, nullptr, bias, G, G, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih, b_hh, bias, 2 * H, 2 * H, s));
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), wih_p, gemm_c_frag(gx, bias), T * (N / 16), G / 16, Ipad / 16, s));
    const size_t step = (size_t)N * H;
    for (int t = 0; t < T; ++t)
        FSN_TRY(fsn_launch_gru_step(gx, whh_p, b_hh + 2 * H, t ? hseq + (t - 1) * step : h_state, hseq + t * step, nullptr,
                                    (long)t * (N / 16), N / 16, H, 0, s));
    if (hipMemcpyAsync(h_state, hseq + (size_t)(T - 1) * step, step * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) {
        fsn_set_error("gru layer forward (state): state copy failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}

extern "C" size_t fsn_gru_layer_bwd_workspace_bytes(int T, int N, int I, int H) {
    const int Ipad = fsn_round_up(I, 16), G = 3 * H;
    Carver cv(nullptr);
    cv.take<float>((size_t)H * G);      // W_hh^T fragments
    cv.take<float>((size_t)Ipad * G);   // W_ih^T fragments
    cv.take<float>((size_t)T * N * G);  // dgx
    cv.take<float>((size_t)T * N * H);  // dghn
    cv.take<float>((size_t)N * H);      // carry
    // the scratch of the weight-gradient products: every (M, Nc) that fsn_gru_layer_backward forms (each shape has
    // its own plan - a narrower product may split K further than the 3H-row one)
    size_t tn = fsn_gemm_tn_workspace_bytes(G, I, (long)T * N);
    for (const int m : {G, 2 * H, H}) {
        const size_t b = fsn_gemm_tn_workspace_bytes(m, H, (long)T * N);
        tn = tn > b ? tn : b;
    }
    size_t cs = 0;  // the column sums fsn_gru_layer_backward forms: 3H, 2H and H columns (each with its own row blocking)
    for (const int c : {G, 2 * H, H}) {
        const size_t b = fsn_colsum_workspace_bytes(c, (long)T * N);
        cs = cs > b ? cs : b;
    }
    cv.take<char>(tn > cs ? tn : cs);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_gru_layer_backward(const float* dh, const float* x, long ldx, const float* w_ih, const float* w_hh,
                                      int T, int N, int I, int H, const float* hseq, const void* save, float* dx,
                                      long lddx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(dh && x && w_ih && w_hh && hseq && save && dw_ih && dw_hh && db_ih && db_hh && workspace,
                "NULL pointer argument");
    FSN_REQUIRE(!dx || lddx >= I, "dx row stride %ld < I", lddx);
    if (workspace_bytes < fsn_gru_layer_bwd_workspace_bytes(T, N, I, H)) {
        fsn_set_error("gru layer backward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = 3 * H;
    Carver cv(workspace);
    float* whhT_p = cv.take<float>((size_t)H * G);
    float* wihT_p = cv.take<float>((size_t)Ipad * G);
    float* dgx = cv.take<float>((size_t)T * N * G);
    float* dghn = cv.take<float>((size_t)T * N * H);
    float* carry = cv.take<float>((size_t)N * H);
    void* scratch = cv.take<char>(0);  // the rest of the workspace (sized by fsn_gru_layer_bwd_workspace_bytes)
    const float* sv = static_cast<const float*>(save);
    FSN_TRY(fsn_launch_pack(w_hh, whhT_p, H, G, H, G, s, 1, H));
    FSN_TRY(fsn_launch_pack(w_ih, wihT_p, I, G, Ipad, G, s, 1, I));
    const size_t step = (size_t)N * H;
    for (int t = T - 1; t >= 0; --t) {
        const size_t tn1 = t + 1 < T ? (size_t)(t + 1) : 0;
        FSN_TRY(fsn_launch_gru_bptt_step(dh + t * step, dgx + tn1 * N * G, dghn + tn1 * step, whhT_p, carry,
                                         sv + (size_t)t * N * 4 * H, t ? hseq + (t - 1) * step : hseq,
                                         dgx + (size_t)t * N * G, dghn + t * step, N / 16, H, t == T - 1, t == 0, s));
    }
    if (dx) {
        FSN_TRY(fsn_launch_gemm(gemm_a_rows(dgx, G), wihT_p, gemm_c_rows(dx, lddx, T * N, I), T * (N / 16), Ipad / 16, G / 16, s));
    }
    FSN_TRY(fsn_launch_gemm_tn(dgx, G, x, ldx, dw_ih, I, G, I, (long)T * N, scratch, s));
    if (T > 1) {
        // dW_hh: rows r, z from the x-side derivatives (identical on the h side), rows n from dghn
        FSN_TRY(fsn_launch_gemm_tn(dgx + (size_t)N * G, G, hseq, H, dw_hh, H, 2 * H, H, (long)(T - 1) * N, scratch, s));
        FSN_TRY(fsn_launch_gemm_tn(dghn + step, H, hseq, H, dw_hh + (size_t)2 * H * H, H, H, H, (long)(T - 1) * N,
                                   scratch, s));
    } else if (hipMemsetAsync(dw_hh, 0, (size_t)G * H * sizeof(float), s) != hipSuccess) {
        fsn_set_error("memset failed");
        return FSN_ERR_LAUNCH;
    }
    FSN_TRY(fsn_launch_colsum(dgx, G, db_ih, G, (long)T * N, scratch, s));
    FSN_TRY(fsn_launch_colsum(dgx, G, db_hh, 2 * H, (long)T * N, scratch, s));
    return fsn_launch_colsum(dghn, H, db_hh + 2 * H, H, (long)T * N, scratch, s);
}
