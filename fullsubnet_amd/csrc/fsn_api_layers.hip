// C ABI of libfsn_hip.so, stand-alone nn.LSTM layers and stacks in inference (and the single layer's training forward):
// their row plans, one layer (+ its output layer), two stacked layers, several stacks over the same frames, the streaming
// form with carried state, and the normalised input of Improved FullSubNet's band sections.
#include "fsn_api_internal.h"

// ---- training step: one nn.LSTM layer, forward with saved activations + BPTT ---------------------
// (recipes/dns_interspeech_2020/fullsubnet/trainer.py:56-63 through sequence_model.py:52-58)
int check_lstm_layer(int T, int N, int I, int H, long ldx) {
    FSN_REQUIRE(T >= 1 && N >= 16 && N % 16 == 0, "lstm layer: need T >= 1 and N a positive multiple of 16 (got %d, %d)", T, N);
    FSN_REQUIRE(I >= 1 && H >= 64 && H % 64 == 0, "lstm layer: need I >= 1 and H a multiple of 64 (got %d, %d)", I, H);
    FSN_REQUIRE(ldx >= fsn_round_up(I, 16) && ldx % 4 == 0, "lstm layer: x row stride %ld must be >= round_up(I,16) and 16-byte aligned", ldx);
    return FSN_OK;
}

// `rows` rows x K columns of each of T steps between two [T][step rows][ld] matrices: one 2-D copy when both sides' rows are
// exactly K wide, one per step otherwise
static int copy_step_rows(float* dst, size_t dst_step, size_t dst_ld, const float* src, size_t src_step, size_t src_ld, int T,
                          int rows, size_t K, hipStream_t s) {
    bool ok = true;
    if (dst_ld == K && src_ld == K)
        ok = hipMemcpy2DAsync(dst, dst_step * K * sizeof(float), src, src_step * K * sizeof(float), rows * K * sizeof(float),
                              (size_t)T, hipMemcpyDeviceToDevice, s) == hipSuccess;
    else
        for (int t = 0; t < T && ok; ++t)
            ok = hipMemcpy2DAsync(dst + t * dst_step * dst_ld, dst_ld * sizeof(float), src + t * src_step * src_ld,
                                  src_ld * sizeof(float), K * sizeof(float), (size_t)rows, hipMemcpyDeviceToDevice,
                                  s) == hipSuccess;
    if (!ok) {
        fsn_set_error("copy of the left-over rows failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}
int gather_step_rows(float* dst, const float* src, long ld, int T, int N, int row0, int left, int K, hipStream_t s) {
    return copy_step_rows(dst, left, K, src + (size_t)row0 * ld, N, ld, T, left, K, s);
}
int scatter_step_rows(float* dst, long ld, const float* src, int T, int N, int row0, int left, int K, hipStream_t s) {
    return copy_step_rows(dst + (size_t)row0 * ld, N, ld, src, left, K, T, left, K, s);
}

extern "C" size_t fsn_lstm_layer_save_bytes(int T, int N, int H) {
    return fsn_round_up_sz(((size_t)T * N * 4 * H + (size_t)T * N * H) * sizeof(float), 256);
}
extern "C" size_t fsn_lstm_layer_fwd_workspace_bytes(int T, int N, int I, int H) {
    Carver cv(nullptr);
    cv.take<float>((size_t)4 * H * fsn_round_up(I, 16));
    cv.take<float>((size_t)4 * H * H);
    cv.take<float>((size_t)4 * H);
    cv.take<float>((size_t)T * N * 4 * H);
    cv.take<float>((size_t)N * H);  // cell state of the step kernels (inference mode)
    return fsn_round_up_sz(cv.off, 256);
}

// Row split of a stand-alone layer in inference mode: the persistent kernel (built for H = 384) takes
// whole rounds of 16 RT-row tiles on all CUs, everything else goes step by step.
static FsnRecPlan layer_plan(int N, int H) {
    FsnRecPlan p{};
    p.tiles = N / 16;
    p.npad = N;
    const int cus = plan_cus();
    if (H != 384 || p.tiles < cus / 4) {
        p.left_tiles = p.tiles;
    } else if (p.tiles <= cus) {
        p.rt = 1;
        p.main_wgs = p.tiles;
    } else {
        // whole rounds on all CUs + left-over tiles step by step beside them ...
        p.rt = p.tiles / cus < 5 ? p.tiles / cus : 5;
        p.main_wgs = cus;
        p.left_tiles = p.tiles - cus * p.rt;
        // ... or FEWER workgroups with one more tile each and nothing left over (the workgroups are independent: a launch
        // takes its tiles-per-workgroup's time whatever its grid).  Measured on Fast FullSubNet's bottleneck (96 steps, round
        // 6): ~11 ms per tile of a workgroup, ~0.11 ms per left-over tile - 448 tiles as 256 x 1 + 192 left over 32.2 ms, as
        // 224 x 2 what 512 tiles take (25.4); 288 tiles stay 256 x 1 + 32 (21.0 against 24.6).
        const int rt2 = (p.tiles + cus - 1) / cus;
        if (p.left_tiles > 0 && rt2 <= 4 && p.tiles % rt2 == 0 && 100 * rt2 < 100 * p.rt + p.left_tiles) {
            p.rt = rt2;
            p.main_wgs = p.tiles / rt2;
            p.left_tiles = 0;
        }
    }
    return p;
}
// The same split with SEVERAL whole rounds (more than four row tiles per CU: layer_plan stops at one round of five and hands
// everything beyond to the step kernels - 96 / 128 utterances of a composed FullSubNet were 518 / 776 left-over tiles, 151 / 216 ms
// per model call): rounds of 2 - 4 tiles per workgroup on every CU, as many as fit, the rest (fewer than one round) left over.
static FsnRecPlan layer_plan_rounds(int N, int H) {
    const int cus = plan_cus();
    const int tiles = N / 16;
    if (H != 384 || tiles < 2 * cus) return layer_plan(N, H);
    FsnRecPlan p{};
    p.tiles = tiles;
    p.npad = N;
    long best = -1;
    for (int rt = 4; rt >= 2; --rt) {
        const int rounds = tiles / (cus * rt);
        if (rounds < 1) continue;
        const int left = tiles - rounds * cus * rt;
        const long cost = (long)rounds * rt * 100 + left;  // a left-over tile: about a hundredth of a tile of a resident workgroup
        if (best < 0 || cost < best) {
            best = cost;
            p.rt = rt;
            p.main_wgs = rounds * cus;
            p.left_tiles = left;
        }
    }
    return p;
}
// Rows (a multiple of 16, >= N) a caller that owns the row padding should give a stand-alone layer of N rows: the next count
// whose plan has no left-over tiles when that is the cheaper plan by the measure above, N itself otherwise.
extern "C" int fsn_lstm_layer_plan_rows(int N, int H) {
    if (N < 1) return N;
    const int n16 = fsn_round_up(N, 16);
    const FsnRecPlan p = layer_plan(n16, H);
    if (p.main_wgs <= 0 || p.left_tiles == 0) return n16;
    const int cus = plan_cus();
    const int rt2 = (p.tiles + cus - 1) / cus;
    if (rt2 > 4) return n16;
    const int padded = (p.tiles + rt2 - 1) / rt2 * rt2;
    return 100 * rt2 < 100 * p.rt + p.left_tiles ? padded * 16 : n16;
}

extern "C" int fsn_lstm_layer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh,
                                      const float* b_ih, const float* b_hh, int T, int N, int I, int H, float* hseq,
                                      void* save, size_t save_bytes, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && hseq && workspace, "NULL pointer argument");
    if ((save && save_bytes < fsn_lstm_layer_save_bytes(T, N, H)) ||
        workspace_bytes < fsn_lstm_layer_fwd_workspace_bytes(T, N, I, H)) {
        fsn_set_error("lstm layer forward: save / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16);
    Carver cv(workspace);
    float* wih_p = cv.take<float>((size_t)4 * H * Ipad);
    float* whh_p = cv.take<float>((size_t)4 * H * H);
    float* bias = cv.take<float>((size_t)4 * H);
    float* gx = cv.take<float>((size_t)T * N * 4 * H);
    float* c_state = cv.take<float>((size_t)N * H);
    float* gates = static_cast<float*>(save);
    float* cseq = gates + (size_t)T * N * 4 * H;
    FSN_TRY(fsn_launch_pack(w_ih, wih_p, 4 * H, I, 4 * H, Ipad, s));
    FSN_TRY(fsn_launch_pack(w_hh, whh_p, 4 * H, H, 4 * H, H, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih, b_hh, bias, 4 * H, 4 * H, s));
    if (!save) {
        // inference with a narrow input on the persistent kernel (e.g. Fast FullSubNet's bottleneck: 12 inputs,
        // 16 384 rows): the K <= 32 projection is formed inside the recurrent kernel from a staged LDS tile,
        // like the sub-band model's layer 0, instead of writing and re-reading a [T][N][4H] projection
        FsnRecPlan plan = layer_plan(N, H);
        if (plan.main_wgs > 0 && (plan.rt > 4 || plan.left_tiles > 16) && (Ipad <= 32 || (I == H && ldx == H)))
            plan = layer_plan_rounds(N, H);  // more than one round's worth of rows (the two forms below take any grid)
        RecArgs rec;  // what the forms below share
        rec.whh = whh_p;
        rec.hseq = hseq;
        rec.Tp = T;
        rec.Npad = N;
        rec.H = H;
        rec.plan = plan;
        if (plan.main_wgs > 0 && plan.left_tiles == 0 && Ipad <= 32) {
            const FsnSbInput xin = sb_input_rows(x, ldx, N, N, Ipad / 16, wih_p, bias);
            rec.xin = &xin;
            rec.c_left = c_state;
            return run_recurrence(rec, s);
        }
        // The same two forms with LEFT-OVER row tiles (whole rounds of 2 - 4 tiles per workgroup + a few tiles more: 64 x 257
        // rows are 256 x 4 tiles + 4): the persistent kernel takes the whole rounds, the left-over rows advance step by step
        // beside it (run_recurrence) from their own small projection - compact copies of their input rows, one GEMM, formed AHEAD
        // of the persistent launch (the GEMM's workgroups do not fit beside it) inside the region the full projection would
        // have taken.  Before: the full [T][N][4H] projection was written and read back for every row (a composed LSTM
        // FullSubNet at 64 x 3 s: 92 ms per model call against 80 at 62 utterances, whose tiles divide evenly).
        const bool narrow = Ipad <= 32 && ldx >= Ipad, stacked = I == H && ldx == H && fsn_lstm_rec_x_supported(H, plan.rt);
        if (plan.main_wgs > 0 && plan.left_tiles > 0 && plan.rt >= 2 && plan.rt <= 4 && (narrow || stacked) && whh_p > wih_p &&
            (size_t)plan.left_tiles * 16 * ((size_t)4 * H + Ipad) <= (size_t)N * 4 * H) {
            const int left = plan.left_tiles * 16, main_rows = N - left;
            float* gx_left = gx;                                  // [T][left / 16 tiles] fragment order
            float* x_left = gx + (size_t)T * left * 4 * H;        // [T][left][Ipad]
            FSN_TRY(gather_step_rows(x_left, x, ldx, T, N, main_rows, left, Ipad, s));
            FSN_TRY(fsn_launch_gemm(gemm_a_rows(x_left, Ipad), wih_p, gemm_c_frag(gx_left, bias), T * (left / 16), 4 * H / 16,
                                    Ipad / 16, s));
            rec.gx_left = gx_left;
            rec.left_stride = left / 16;
            rec.c_left = c_state + (size_t)main_rows * H;
            if (narrow) {
                const FsnSbInput xin = sb_input_rows(x, ldx, N, main_rows, Ipad / 16, wih_p, bias);
                rec.xin = &xin;
                return run_recurrence(rec, s);
            }
            rec.x_main = x;
            rec.wih_main = wih_p;
            rec.bias_main = bias;
            return run_recurrence(rec, s);
        }
        // a layer of a stack on the persistent kernel (input = the hidden sequence of an equally wide layer below, e.g.
        // the second bottleneck layer of Fast FullSubNet, fast_fullsubnet/model.py:66-74): the K = H projection is
        // formed inside the recurrent kernel from x streamed through its LDS ring (lstm_rec_x_kernel<.., HSEQ>) - no
        // projection GEMM, no [T][N][4H] gx round trip
        if (plan.main_wgs > 0 && plan.left_tiles == 0 && I == H && ldx == H && fsn_lstm_rec_x_supported(H, plan.rt) &&
            whh_p > wih_p)
            return fsn_launch_lstm_rec_x(x, wih_p, whh_p, bias, T, N, H, plan.rt, plan.main_wgs, s, nullptr, hseq);
    }
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), wih_p, gemm_c_frag(gx, bias), T * (N / 16), 4 * H / 16, Ipad / 16, s));
    if (!save) {  // inference: nothing kept but the hidden sequence
        const FsnRecPlan plan = layer_plan(N, H);
        const long main_tiles = (long)plan.main_wgs * plan.rt;
        RecArgs rec;
        rec.gx = gx;
        rec.gx_left = gx;
        rec.left_stride = plan.tiles;
        rec.left_off = main_tiles;
        rec.whh = whh_p;
        rec.hseq = hseq;
        rec.c_left = c_state + main_tiles * 16 * H;
        rec.Tp = T;
        rec.Npad = N;
        rec.H = H;
        rec.plan = plan;
        return run_recurrence(rec, s);
    }
    const size_t step = (size_t)N * H;
    for (int t = 0; t < T; ++t)
        FSN_TRY(fsn_launch_lstm_step_train(gx, whh_p, t ? hseq + (t - 1) * step : hseq, hseq + t * step,
                                           t ? cseq + (t - 1) * step : cseq, cseq + t * step,
                                           gates + (size_t)t * N * 4 * H, (long)t * (N / 16), N / 16, H, t == 0, s));
    return FSN_OK;
}

// ---- a stacked layer + the output layer that follows it, inference ---------------------------------------------------
// (sequence_model.py:106-125: `self.fc_output_layer(self.sequence_model(x))` for the LAST layer of a stack with one or two
// outputs - Fast FullSubNet's bottleneck, fast_fullsubnet/model.py:66-74: 16 384 rows x 384 units -> 1 value per step.)
// When the persistent kernel that forms the projection itself takes the layer (fsn_lstm_layer_fc_supported), its fused
// two-row output layer does the nn.Linear as well: the [T][N][H] hidden sequence is neither written nor read back.
// out0 / out1: [T][ldo] PRE-activation outputs 0 / 1 (time-major; out1 may be NULL when O == 1).
static bool lstm_layer_fc_plan(int T, int N, int I, long ldx, int H, int O, FsnRecPlan* plan) {
    if (T < 1 || N < 16 || N % 16 || H != 384 || I != H || ldx != H || O < 1 || O > 2) return false;
    const FsnRecPlan p = layer_plan(N, H);
    if (plan) *plan = p;
    return p.main_wgs > 0 && p.left_tiles == 0 && fsn_lstm_rec_x_supported(H, p.rt);
}
extern "C" int fsn_lstm_layer_fc_supported(int T, int N, int I, long ldx, int H, int O) {
    return lstm_layer_fc_plan(T, N, I, ldx, H, O, nullptr) ? 1 : 0;
}
extern "C" size_t fsn_lstm_layer_fc_workspace_bytes(int T, int N, int I, int H) {
    if (T < 1 || N < 16 || I < 1 || H < 64) return 0;
    Carver cv(nullptr);
    cv.take<float>((size_t)4 * H * fsn_round_up(I, 16));
    cv.take<float>((size_t)4 * H * H);
    cv.take<float>((size_t)4 * H);
    cv.take<float>((size_t)16 * H);      // the output layer's two rows as one packed column tile
    cv.take<float>(16);
    cv.take<float>((size_t)T * N);       // the unused second output when O == 1
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" int fsn_lstm_layer_forward_fc(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                         const float* b_hh, int T, int N, int I, int H, const float* fc_w, const float* fc_b,
                                         int O, float* out0, float* out1, long ldo, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && fc_w && fc_b && out0 && workspace, "NULL pointer argument");
    FsnRecPlan plan{};
    FSN_REQUIRE(lstm_layer_fc_plan(T, N, I, ldx, H, O, &plan),
                "lstm layer + output layer: not a shape of the fused form (H = I = ldx = 384, 1 or 2 outputs, whole rounds of "
                "2 - 4 row tiles per CU): ask fsn_lstm_layer_fc_supported");
    FSN_REQUIRE(ldo >= N && (O == 1 || out1), "lstm layer + output layer: ldo %ld < N or the second output is missing", ldo);
    if (workspace_bytes < fsn_lstm_layer_fc_workspace_bytes(T, N, I, H)) {
        fsn_set_error("lstm layer + output layer: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Carver cv(workspace);
    float* wih_p = cv.take<float>((size_t)4 * H * fsn_round_up(I, 16));
    float* whh_p = cv.take<float>((size_t)4 * H * H);
    float* bias = cv.take<float>((size_t)4 * H);
    float* fcw_p = cv.take<float>((size_t)16 * H);
    float* fcb_p = cv.take<float>(16);
    float* spare = cv.take<float>((size_t)T * N);
    FSN_TRY(fsn_launch_pack(w_ih, wih_p, 4 * H, I, 4 * H, fsn_round_up(I, 16), s));
    FSN_TRY(fsn_launch_pack(w_hh, whh_p, 4 * H, H, 4 * H, H, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih, b_hh, bias, 4 * H, 4 * H, s));
    FSN_TRY(fsn_launch_pack(fc_w, fcw_p, O, H, 16, H, s));
    FSN_TRY(fsn_launch_bias_sum(fc_b, nullptr, fcb_p, O, 16, s));
    // the kernel's destination of row n at step t is plane[((n / F) T + t) FP + n % F]: one group of F = N rows, FP = ldo
    // -> plane[t ldo + n], time-major
    const FsnRecFc fc = rec_fc(fcw_p, fcb_p, out0, O > 1 ? out1 : spare, N, 0, N, (int)ldo, T, 0);
    return fsn_launch_lstm_rec_x(x, wih_p, whh_p, bias, T, N, H, plan.rt, plan.main_wgs, s, &fc, nullptr);
}

bool lstm2_on_chain(int T, int N, int H) { return fsn_fb_chain_supported(H, N) && T <= fsn_fb_chain_max_steps(); }

// Two stacked LSTM layers of equal width in inference mode as one wavefront (layer 1 at step t next to layer 0
// at step t + 1: T + 1 dependent launches instead of 2 T).  For the latency-bound regime - few rows - where
// SequenceModel blocks of the sibling models live (Improved FullSubNet's band sections: B x {20, 25, 6, 4} rows).
// H = 384 twice, up to 32 input columns, whole 64-row clusters in the group kernel's ranges (96 - 159 and 224 - 256 row
// tiles: e.g. Fast FullSubNet's bottleneck at 24 - 39 utterances per rank): clusters, 0 = not this shape
static int lstm2_infer_group_clusters(int T, int N, int I, int H0, int H1, long ldx) {
    if (H0 != 384 || H1 != 384 || I > 32 || N % 64 != 0 || N / 16 < kWavefrontBelowTiles) return 0;
    if (ldx != 16 && ldx != 32) return 0;  // the kernel reads x rows of exactly one or two K chunks; anything else: generic path
    if ((size_t)T * N * H0 * sizeof(float) > 0x7fffffffull) return 0;  // the reach of a buffer resource's offsets
    const int tiles = N / 16, c = fsn_lstm2_group_clusters(tiles);
    return 4 * c == tiles ? c : 0;
}
static size_t lstm2_fwd_workspace(int T, int N, int I, int H0, int H1, int group_clusters);
// sized for either row stride of x (the group kernel's buffers are included whenever the shape COULD take it)
extern "C" size_t fsn_lstm2_fwd_workspace_bytes(int T, int N, int I, int H0, int H1) {
    return lstm2_fwd_workspace(T, N, I, H0, H1, lstm2_infer_group_clusters(T, N, I, H0, H1, fsn_round_up(I, 16)));
}
static size_t lstm2_fwd_workspace(int T, int N, int I, int H0, int H1, int group_clusters) {
    Carver cv(nullptr);
    cv.take<float>((size_t)4 * H0 * fsn_round_up(I, 16));  // W_ih0 fragments
    cv.take<float>((size_t)4 * H0 * H0);                   // W_hh0
    cv.take<float>((size_t)4 * H1 * H0);                   // W_ih1
    cv.take<float>((size_t)4 * H1 * H1);                   // W_hh1
    cv.take<float>((size_t)4 * H0);                        // b0
    cv.take<float>((size_t)4 * H1);                        // b1
    cv.take<float>((size_t)4 * H1 * 16);                   // b1 as fragment tiles
    cv.take<float>((size_t)T * N * 4 * H0);                // layer-0 projection
    cv.take<float>((size_t)T * N * H0);                    // layer-0 hidden sequence
    cv.take<float>((size_t)N * (H0 + H1));                 // cell states
    if (H0 == H1 && lstm2_on_chain(T, N, H0)) {            // the persistent chain kernel instead of the wavefront
        cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
        cv.take<unsigned>(fsn_fb_chain_flag_words());
    }
    if (const int clusters = group_clusters) {  // the group kernel (general two-layer form)
        cv.take<float>((size_t)4 * H0 * 32 + (size_t)3 * 4 * H0 * H0);
        cv.take<unsigned>(fsn_lstm2_group_flag_words(clusters));
    }
    return fsn_round_up_sz(cv.off, 256);
}
// 1 when fsn_lstm2_forward has a persistent kernel for this shape (callers that would otherwise run layer by layer on
// the per-layer persistent kernels - 1536+ rows - should then prefer it)
extern "C" int fsn_lstm2_forward_is_persistent(int T, int N, int I, long ldx, int H0, int H1) {
    return (H0 == H1 && lstm2_on_chain(T, N, H0)) || lstm2_infer_group_clusters(T, N, I, H0, H1, ldx) > 0;
}
extern "C" int fsn_lstm2_forward(const float* x, long ldx, const float* w_ih0, const float* w_hh0, const float* b_ih0,
                                 const float* b_hh0, const float* w_ih1, const float* w_hh1, const float* b_ih1,
                                 const float* b_hh1, int T, int N, int I, int H0, int H1, float* hseq1, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H0, ldx));
    FSN_REQUIRE(H1 >= 64 && H1 % 64 == 0, "lstm2: second hidden size %d must be a multiple of 64", H1);
    FSN_REQUIRE(x && w_ih0 && w_hh0 && b_ih0 && b_hh0 && w_ih1 && w_hh1 && b_ih1 && b_hh1 && hseq1 && workspace,
                "NULL pointer argument");
    if (workspace_bytes < fsn_lstm2_fwd_workspace_bytes(T, N, I, H0, H1)) {
        fsn_set_error("lstm2 forward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G0 = 4 * H0, G1 = 4 * H1;
    Carver cv(workspace);
    float* wih0_p = cv.take<float>((size_t)G0 * Ipad);
    float* whh0_p = cv.take<float>((size_t)G0 * H0);
    float* wih1_p = cv.take<float>((size_t)G1 * H0);
    float* whh1_p = cv.take<float>((size_t)G1 * H1);
    float* b0 = cv.take<float>((size_t)G0);
    float* b1 = cv.take<float>((size_t)G1);
    float* b1_frag = cv.take<float>((size_t)G1 * 16);
    float* gx = cv.take<float>((size_t)T * N * G0);
    float* hseq0 = cv.take<float>((size_t)T * N * H0);
    float* cst = cv.take<float>((size_t)N * (H0 + H1));
    if (const int clusters = lstm2_infer_group_clusters(T, N, I, H0, H1, ldx)) {
        // both layers, all steps, as one persistent launch of the group kernel (no projection GEMM, no gx): the four
        // packed matrices in one buffer, W_ih0 32 columns wide
        if (H0 == H1 && lstm2_on_chain(T, N, H0)) {
            cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
            cv.take<unsigned>(fsn_fb_chain_flag_words());
        }
        float* gw = cv.take<float>((size_t)G0 * 32 + (size_t)3 * G0 * H0);
        unsigned* flags = cv.take<unsigned>(fsn_lstm2_group_flag_words(clusters));
        float* g_wih0 = gw;
        float* g_whh0 = g_wih0 + (size_t)G0 * 32;
        float* g_wih1 = g_whh0 + (size_t)G0 * H0;
        float* g_whh1 = g_wih1 + (size_t)G0 * H0;
        FSN_TRY(fsn_launch_pack(w_ih0, g_wih0, G0, I, G0, 32, s));
        FSN_TRY(fsn_launch_pack(w_hh0, g_whh0, G0, H0, G0, H0, s));
        FSN_TRY(fsn_launch_pack(w_ih1, g_wih1, G1, H0, G1, H0, s));
        FSN_TRY(fsn_launch_pack(w_hh1, g_whh1, G1, H1, G1, H1, s));
        FSN_TRY(fsn_launch_bias_sum(b_ih0, b_hh0, b0, G0, G0, s));
        FSN_TRY(fsn_launch_bias_sum(b_ih1, b_hh1, b1, G1, G1, s));
        FSN_PERSIST_BEGIN(s);
        FSN_TRY(fsn_launch_lstm2_group_train(x, ldx, (int)ldx, N, g_wih0, g_whh0, g_wih1, g_whh1, b0, b1, hseq0, hseq1, nullptr,
                                             nullptr, flags, T, clusters, H0, s));
        return fsn_launch_poison_if(flags + fsn_lstm2_group_status_word(clusters), hseq1, (size_t)T * N * H1, s);
    }
    FSN_TRY(fsn_launch_pack(w_ih0, wih0_p, G0, I, G0, Ipad, s));
    FSN_TRY(fsn_launch_pack(w_hh0, whh0_p, G0, H0, G0, H0, s));
    FSN_TRY(fsn_launch_pack(w_ih1, wih1_p, G1, H0, G1, H0, s));
    FSN_TRY(fsn_launch_pack(w_hh1, whh1_p, G1, H1, G1, H1, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih0, b_hh0, b0, G0, G0, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih1, b_hh1, b1, G1, G1, s));
    FSN_TRY(fsn_launch_bias_frag(b1, b1_frag, G1, s));
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), wih0_p, gemm_c_frag(gx, b0), T * (N / 16), G0 / 16, Ipad / 16, s));
    if (H0 == H1 && lstm2_on_chain(T, N, H0)) {  // H = 384 / 512, up to 64 rows: one persistent launch (fb_chain_kernels.hip)
        float* exchange = cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
        unsigned* flags = cv.take<unsigned>(fsn_fb_chain_flag_words());
        FSN_PERSIST_BEGIN(s);
        FSN_TRY(fsn_launch_fb_chain(gx, whh0_p, wih1_p, whh1_p, b1, exchange, flags, hseq1, T, N, H0, s));
        return fsn_launch_poison_if(flags + fsn_fb_chain_status_word(), hseq1, (size_t)T * N * H0, s);
    }
    return fsn_launch_lstm_wavefront2w(gx, N / 16, 0, whh0_p, wih1_p, b1_frag, whh1_p, hseq0, hseq1, N, 0, cst,
                                       cst + (size_t)N * H0, T, N / 16, H0, H1, s);
}

// Streaming form (frame-by-frame / chunked inference with carried state): T more steps from the state
// (h, c) [N][H], which is updated in place.  Always on the per-step kernels.  The weights are re-tiled
// once (fsn_lstm_layer_pack; layer_packed_layout in fsn_api_internal.h) - a per-frame caller must not pay three pack
// launches per layer per call.
// ---- Improved FullSubNet: the normalised input of one band section, in the LSTM entries' layout ------------------------
extern "C" size_t fsn_improved_section_input_workspace_bytes(int B, int F) {
    if (B < 1 || F < 2) return 0;
    return fsn_round_up_sz(fsn_section_input_workspace_floats(B, F) * sizeof(float), 256);
}
// fsn_improved_section_input and its ragged form share one body; frames == NULL is the rectangular batch
static int section_input(const float* noisy, const float* fb_out, const int* frames, int B, int F, int T, int lower, int upper,
                         int sb_center, int sb_neighbor, int fb_center, int fb_neighbor, int unit_lo, int unit_hi, float eps,
                         float* out, int Np, int ldo, void* workspace, size_t workspace_bytes, void* stream) {
    FSN_REQUIRE(noisy && fb_out && out && workspace, "NULL pointer argument");
    FSN_REQUIRE(B >= 1 && F >= 2 && T >= 1 && 0 <= lower && lower < upper && upper <= F, "section input: bad band [%d, %d) of %d bins",
                lower, upper, F);
    FSN_REQUIRE(sb_center >= 1 && fb_center >= 1 && sb_neighbor >= 0 && fb_neighbor >= 0 && (upper - lower) % sb_center == 0 &&
                    (upper - lower) % fb_center == 0 && (upper - lower) / sb_center == (upper - lower) / fb_center,
                "section input: the band must hold the same whole number of units for both windows");
    const int units = (upper - lower) / sb_center, W = sb_center + 2 * sb_neighbor + fb_center + 2 * fb_neighbor;
    // the reflections of model.py:376-383 are single ones: a window may not reach beyond a mirror image of the spectrum
    FSN_REQUIRE(sb_neighbor < F && fb_neighbor < F && sb_center + sb_neighbor <= F && fb_center + fb_neighbor <= F,
                "section input: windows wider than the spectrum");
    FSN_REQUIRE(0 <= unit_lo && unit_lo < unit_hi && unit_hi <= units, "section input: unit range [%d, %d) of %d", unit_lo, unit_hi,
                units);
    FSN_REQUIRE(Np >= B * (unit_hi - unit_lo) && Np <= 65535 && ldo >= W && ldo <= 240,
                "section input: out [T][%d][%d]: rows up to 65535, the window's %d columns up to 240 (a 64-frame tile in LDS)", Np,
                ldo, W);
    FSN_REQUIRE(eps > 0.f, "section input: eps must be positive");
    if (workspace_bytes < fsn_improved_section_input_workspace_bytes(B, F)) {
        fsn_set_error("section input: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    return fsn_launch_section_input(noisy, fb_out, B, F, T, lower, units, sb_center, sb_neighbor, fb_center, fb_neighbor, unit_lo,
                                    unit_hi, eps, out, Np, ldo, workspace, static_cast<hipStream_t>(stream), frames);
}
extern "C" int fsn_improved_section_input(const float* noisy, const float* fb_out, int B, int F, int T, int lower, int upper,
                                          int sb_center, int sb_neighbor, int fb_center, int fb_neighbor, int unit_lo,
                                          int unit_hi, float eps, float* out, int Np, int ldo, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    return section_input(noisy, fb_out, nullptr, B, F, T, lower, upper, sb_center, sb_neighbor, fb_center, fb_neighbor, unit_lo,
                         unit_hi, eps, out, Np, ldo, workspace, workspace_bytes, stream);
}
extern "C" int fsn_improved_section_input_ragged(const float* noisy, const float* fb_out, const int* frames, int B, int F, int T,
                                                 int lower, int upper, int sb_center, int sb_neighbor, int fb_center,
                                                 int fb_neighbor, int unit_lo, int unit_hi, float eps, float* out, int Np, int ldo,
                                                 void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(frames, "NULL pointer argument");
    return section_input(noisy, fb_out, frames, B, F, T, lower, upper, sb_center, sb_neighbor, fb_center, fb_neighbor, unit_lo,
                         unit_hi, eps, out, Np, ldo, workspace, workspace_bytes, stream);
}

// ---- several independent two-layer stacks over the same frames ------------------------------------------------------
// (improved_fullsubnet/model.py:402-449: the band sections' SequenceModels - B x {20, 25, 6, 4} rows at 48 kHz, input
// widths 62 .. 180 - all see the same T frames.)  When every stack is H = 384 twice and together they fill most of the
// chip's workgroup sets, all of them run as ONE persistent launch of the group kernel (GX form: projection GEMM per
// stack, then lstm2_group_multi_kernel); otherwise stack by stack through fsn_lstm2_forward's forms.
static int lstm2_multi_clusters(int n, const fsn_lstm2_stack* st, int T) {
    const int cap = fsn_lstm2_group_multi_cap();
    if (cap == 0 || n < 1 || n > 8 || T < 4) return 0;
    int clusters = 0;
    for (int k = 0; k < n; ++k) {
        if (st[k].H0 != 384 || st[k].H1 != 384 || st[k].N % 16 || (size_t)T * st[k].N * 384 * 4 > 0x7fffffffull) return 0;
        clusters += (st[k].N + 63) / 64;
    }
    // below ~3/4 of the sets the stacks are faster as wavefronts on their own streams (a persistent step costs the same
    // ~58 us whatever the cluster count)
    return clusters <= cap && 4 * clusters >= 3 * cap ? clusters : 0;
}
struct Lstm2MultiPlan {
    float *whh0, *wih1, *whh1, *wih0, *b0, *b1, *gx, *hseq0;
};
static void lstm2_multi_carve(int n, const fsn_lstm2_stack* st, int T, int clusters, Carver& cv, Lstm2MultiPlan* out,
                              unsigned** flags) {
    // the recurrent matrices of all stacks first (one buffer: 32-bit offsets inside the kernel)
    for (int k = 0; k < n; ++k) {
        const size_t G = 4 * (size_t)st[k].H0, H = st[k].H0;
        Lstm2MultiPlan p{};
        p.whh0 = cv.take<float>(G * H);
        p.wih1 = cv.take<float>(G * H);
        p.whh1 = cv.take<float>(G * H);
        if (out) out[k] = p;
    }
    for (int k = 0; k < n; ++k) {
        const size_t G = 4 * (size_t)st[k].H0, H = st[k].H0, Ipad = fsn_round_up(st[k].I, 16);
        Lstm2MultiPlan p = out ? out[k] : Lstm2MultiPlan{};
        p.wih0 = cv.take<float>(G * Ipad);
        p.b0 = cv.take<float>(G);
        p.b1 = cv.take<float>(G);
        p.gx = cv.take<float>((size_t)T * st[k].N * G);
        p.hseq0 = cv.take<float>((size_t)T * st[k].N * H);
        if (out) out[k] = p;
    }
    unsigned* f = cv.take<unsigned>(fsn_lstm2_group_flag_words(clusters));
    if (flags) *flags = f;
}
static int check_lstm2_stacks(int n, const fsn_lstm2_stack* st, int T) {
    FSN_REQUIRE(st && n >= 1 && n <= 8, "lstm2 multi: 1 .. 8 stacks (got %d)", n);
    for (int k = 0; k < n; ++k) {
        FSN_TRY(check_lstm_layer(T, st[k].N, st[k].I, st[k].H0, st[k].ldx));
        FSN_REQUIRE(st[k].H1 >= 64 && st[k].H1 % 64 == 0, "lstm2 multi: stack %d: second hidden size %d must be a multiple of 64", k,
                    st[k].H1);
    }
    return FSN_OK;
}
extern "C" int fsn_lstm2_multi_is_persistent(int n, const fsn_lstm2_stack* stacks, int T) {
    if (!stacks || n < 1 || n > 8) return 0;
    for (int k = 0; k < n; ++k)
        if (stacks[k].N < 16 || stacks[k].I < 1) return 0;
    return lstm2_multi_clusters(n, stacks, T) > 0 ? 1 : 0;
}
extern "C" size_t fsn_lstm2_multi_workspace_bytes(int n, const fsn_lstm2_stack* stacks, int T) {
    if (check_lstm2_stacks(n, stacks, T) != FSN_OK) return 0;
    if (const int clusters = lstm2_multi_clusters(n, stacks, T)) {
        Carver cv(nullptr);
        lstm2_multi_carve(n, stacks, T, clusters, cv, nullptr, nullptr);
        return fsn_round_up_sz(cv.off, 256);
    }
    size_t most = 0;  // stack by stack: one stack's workspace at a time
    for (int k = 0; k < n; ++k) {
        const size_t b = fsn_lstm2_fwd_workspace_bytes(T, stacks[k].N, stacks[k].I, stacks[k].H0, stacks[k].H1);
        most = b > most ? b : most;
    }
    return most;
}
extern "C" int fsn_lstm2_forward_multi(int n, const fsn_lstm2_stack* stacks, int T, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm2_stacks(n, stacks, T));
    FSN_REQUIRE(workspace, "NULL pointer argument");
    for (int k = 0; k < n; ++k) {
        const fsn_lstm2_stack& q = stacks[k];
        FSN_REQUIRE(q.x && q.w_ih0 && q.w_hh0 && q.b_ih0 && q.b_hh0 && q.w_ih1 && q.w_hh1 && q.b_ih1 && q.b_hh1 && q.hseq1,
                    "lstm2 multi: stack %d: NULL pointer argument", k);
    }
    if (workspace_bytes < fsn_lstm2_multi_workspace_bytes(n, stacks, T)) {
        fsn_set_error("lstm2 multi: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    const int clusters = lstm2_multi_clusters(n, stacks, T);
    if (!clusters) {
        for (int k = 0; k < n; ++k) {
            const fsn_lstm2_stack& q = stacks[k];
            FSN_TRY(fsn_lstm2_forward(q.x, q.ldx, q.w_ih0, q.w_hh0, q.b_ih0, q.b_hh0, q.w_ih1, q.w_hh1, q.b_ih1, q.b_hh1, T, q.N,
                                      q.I, q.H0, q.H1, q.hseq1, workspace, workspace_bytes, stream));
        }
        return FSN_OK;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    Carver cv(workspace);
    Lstm2MultiPlan plan[8];
    unsigned* flags = nullptr;
    lstm2_multi_carve(n, stacks, T, clusters, cv, plan, &flags);
    FsnGroupStack gs[8];
    for (int k = 0; k < n; ++k) {
        const fsn_lstm2_stack& q = stacks[k];
        const Lstm2MultiPlan& p = plan[k];
        const int H = q.H0, G = 4 * H, Ipad = fsn_round_up(q.I, 16);
        FSN_TRY(fsn_launch_pack(q.w_ih0, p.wih0, G, q.I, G, Ipad, s));
        FSN_TRY(fsn_launch_pack(q.w_hh0, p.whh0, G, H, G, H, s));
        FSN_TRY(fsn_launch_pack(q.w_ih1, p.wih1, G, H, G, H, s));
        FSN_TRY(fsn_launch_pack(q.w_hh1, p.whh1, G, H, G, H, s));
        FSN_TRY(fsn_launch_bias_sum(q.b_ih0, q.b_hh0, p.b0, G, G, s));
        FSN_TRY(fsn_launch_bias_sum(q.b_ih1, q.b_hh1, p.b1, G, G, s));
        FSN_TRY(fsn_launch_gemm(gemm_a_rows(q.x, q.ldx), p.wih0, gemm_c_frag(p.gx, p.b0), T * (q.N / 16), G / 16, Ipad / 16, s));
        FsnGroupStack& g = gs[k];
        g.gx = p.gx;
        g.whh0_p = p.whh0;
        g.wih1_p = p.wih1;
        g.whh1_p = p.whh1;
        g.bias1 = p.b1;
        g.hseq0 = p.hseq0;
        g.hseq1 = q.hseq1;
        g.N = q.N;
    }
    FSN_PERSIST_BEGIN(s);
    FSN_TRY(fsn_launch_lstm2_group_multi(n, gs, flags, T, 384, s));
    for (int k = 0; k < n; ++k)
        FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_group_status_word(clusters), stacks[k].hseq1,
                                     (size_t)T * stacks[k].N * stacks[k].H1, s));
    return FSN_OK;
}

extern "C" size_t fsn_lstm_layer_packed_bytes(int I, int H) {
    if (I < 1 || H < 64 || H % 64) return 0;
    return layer_packed_layout(I, H).total * sizeof(float);
}
extern "C" int fsn_lstm_layer_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int I,
                                   int H, void* packed, size_t packed_bytes, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(w_ih && w_hh && b_ih && b_hh && packed, "NULL pointer argument");
    FSN_REQUIRE(I >= 1 && H >= 64 && H % 64 == 0, "lstm layer: need I >= 1 and H a multiple of 64 (got %d, %d)", I, H);
    if (packed_bytes < fsn_lstm_layer_packed_bytes(I, H)) {
        fsn_set_error("lstm layer pack: buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LayerPacked p = layer_packed_layout(I, H);
    float* o = static_cast<float*>(packed);
    FSN_TRY(fsn_launch_pack(w_ih, o + p.wih, 4 * H, I, 4 * H, fsn_round_up(I, 16), s));
    FSN_TRY(fsn_launch_pack(w_hh, o + p.whh, 4 * H, H, 4 * H, H, s));
    return fsn_launch_bias_sum(b_ih, b_hh, o + p.bias, 4 * H, 4 * H, s);
}
extern "C" size_t fsn_lstm_layer_state_workspace_bytes(int T, int N, int H) {
    return fsn_round_up_sz((size_t)T * N * 4 * H * sizeof(float), 256);  // the input projection of the T steps
}
extern "C" int fsn_lstm_layer_forward_state(const float* x, long ldx, const void* packed, int T, int N, int I, int H,
                                            float* hseq, float* h_state, float* c_state, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(x && packed && hseq && h_state && c_state && workspace, "NULL pointer argument");
    if (workspace_bytes < fsn_lstm_layer_state_workspace_bytes(T, N, H)) {
        fsn_set_error("lstm layer forward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const LayerPacked p = layer_packed_layout(I, H);
    const float* pk = static_cast<const float*>(packed);
    float* gx = static_cast<float*>(workspace);
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), pk + p.wih, gemm_c_frag(gx, pk + p.bias), T * (N / 16), 4 * H / 16,
                            fsn_round_up(I, 16) / 16, s));
    const size_t step = (size_t)N * H;
    for (int t = 0; t < T; ++t)
        FSN_TRY(fsn_launch_lstm_step(gx, pk + p.whh, t ? hseq + (t - 1) * step : h_state, hseq + t * step, c_state,
                                     (long)t * (N / 16), N / 16, H, 0, s));
    if (hipMemcpyAsync(h_state, hseq + (size_t)(T - 1) * step, step * sizeof(float), hipMemcpyDeviceToDevice, s) !=
        hipSuccess) {
        fsn_set_error("state copy failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}
