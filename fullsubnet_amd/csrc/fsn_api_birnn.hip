// C ABI of libfsn_hip.so, bidirectional nn.LSTM / nn.GRU layers (audio_zen/model/module/sequence_model.py:52-66 with
// bidirectional = True): forward (inference / training) and BPTT of ONE layer, both directions per step launch
// (birnn_step_kernels.hip).  Everything that is not a recurrence runs on the launchers the unidirectional entries use: the
// input projection of both directions is ONE GEMM with 2 g H output columns (the stacked W_ih [2][gH][I] is a taller weight
// matrix), dX one product per direction and their sum, the weight gradients gemm_tn / colsum per direction.
#include "fsn_api_internal.h"
#include "fsn_birnn.h"

static thread_local unsigned g_bi_step_launches = 0;
extern "C" unsigned fsn_debug_bilayer_last_step_launches(void) { return g_bi_step_launches; }

static bool bi_shape_ok(int T, int N, int I, int H) { return T >= 1 && N >= 16 && N % 16 == 0 && I >= 1 && H >= 64 && H % 64 == 0; }
static int check_bilayer(int T, int N, int I, int H, long ldx, long ldh, const char* what) {
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(ldh >= 2 * (long)H && ldh % 4 == 0, "bilayer: %s row stride %ld must be >= 2 H = %d and 16-byte aligned", what, ldh, 2 * H);
    return FSN_OK;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
static size_t bilayer_save_bytes(int T, int N, int H, int g) {  // per direction: gates [T][N][4H] (+ LSTM: cells [T][N][H])
    return fsn_round_up_sz((size_t)2 * T * N * (g == 4 ? 5 : 4) * H * sizeof(float), 256);
}
struct BiFwdBufs {
    float *wih_p, *whh_p, *bias, *gx, *c;
};
static size_t bilayer_fwd_carve(void* ws, int T, int N, int I, int H, int g, BiFwdBufs* b) {
    const size_t G = (size_t)g * H;
    Carver cv(ws);
    b->wih_p = cv.take<float>(2 * G * fsn_round_up(I, 16));
    b->whh_p = cv.take<float>(2 * G * H);
    b->bias = cv.take<float>(2 * G);
    b->gx = cv.take<float>((size_t)T * N * 2 * G);
    b->c = cv.take<float>((size_t)2 * N * H);  // LSTM cell state of each direction (inference)
    return fsn_round_up_sz(cv.off, 256);
}
static int bilayer_forward(int g, const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                           const float* b_hh, int T, int N, int I, int H, float* hseq, long ldh, void* save, size_t save_bytes,
                           void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    g_bi_step_launches = 0;
    FSN_TRY(check_bilayer(T, N, I, H, ldx, ldh, "hseq"));
    FSN_REQUIRE(x && w_ih && w_hh && b_ih && b_hh && hseq && workspace, "NULL pointer argument");
    BiFwdBufs b{};
    if ((save && save_bytes < bilayer_save_bytes(T, N, H, g)) || workspace_bytes < bilayer_fwd_carve(nullptr, T, N, I, H, g, &b)) {
        fsn_set_error("bilayer forward: save / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = g * H;
    bilayer_fwd_carve(workspace, T, N, I, H, g, &b);
    FSN_TRY(fsn_launch_pack(w_ih, b.wih_p, 2 * G, I, 2 * G, Ipad, s));
    for (int d = 0; d < 2; ++d) FSN_TRY(fsn_launch_pack(w_hh + (size_t)d * G * H, b.whh_p + (size_t)d * G * H, G, H, G, H, s));
    if (g == 4) {
        FSN_TRY(fsn_launch_bias_sum(b_ih, b_hh, b.bias, 2 * G, 2 * G, s));
    } else {  // b_ih everywhere + b_hh for r and z (b_hn stays inside r * (W_hn h + b_hn))
        FSN_TRY(fsn_launch_bias_sum(b_ih, nullptr, b.bias, 2 * G, 2 * G, s));
        for (int d = 0; d < 2; ++d) FSN_TRY(fsn_launch_bias_sum(b_ih + d * G, b_hh + d * G, b.bias + d * G, 2 * H, 2 * H, s));
    }
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), b.wih_p, gemm_c_frag(b.gx, b.bias), T * (N / 16), 2 * G / 16, Ipad / 16, s));
    FsnBiLayer L{};
    L.gx = b.gx;
    L.hseq = hseq;
    L.ldh = ldh;
    L.T = T;
    L.N = N;
    L.H = H;
    const size_t dir_save = (size_t)T * N * (g == 4 ? 5 : 4) * H;
    for (int d = 0; d < 2; ++d) {
        L.whh_p[d] = b.whh_p + (size_t)d * G * H;
        L.b_hn[d] = b_hh + (size_t)d * G + 2 * H;
        L.c[d] = b.c + (size_t)d * N * H;
        L.save[d] = save ? static_cast<float*>(save) + d * dir_save : nullptr;
    }
    for (int st = 0; st < T; ++st) {
        FSN_TRY(g == 4 ? fsn_launch_bilstm_step(L, st, s) : fsn_launch_bigru_step(L, st, s));
        ++g_bi_step_launches;
    }
    return FSN_OK;
}

extern "C" size_t fsn_lstm_bilayer_save_bytes(int T, int N, int H) { return bi_shape_ok(T, N, 1, H) ? bilayer_save_bytes(T, N, H, 4) : 0; }
extern "C" size_t fsn_gru_bilayer_save_bytes(int T, int N, int H) { return bi_shape_ok(T, N, 1, H) ? bilayer_save_bytes(T, N, H, 3) : 0; }
extern "C" size_t fsn_lstm_bilayer_fwd_workspace_bytes(int T, int N, int I, int H) {
    BiFwdBufs b{};
    return bi_shape_ok(T, N, I, H) ? bilayer_fwd_carve(nullptr, T, N, I, H, 4, &b) : 0;
}
extern "C" size_t fsn_gru_bilayer_fwd_workspace_bytes(int T, int N, int I, int H) {
    BiFwdBufs b{};
    return bi_shape_ok(T, N, I, H) ? bilayer_fwd_carve(nullptr, T, N, I, H, 3, &b) : 0;
}
extern "C" int fsn_lstm_bilayer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                        const float* b_hh, int T, int N, int I, int H, float* hseq, long ldh, void* save,
                                        size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return bilayer_forward(4, x, ldx, w_ih, w_hh, b_ih, b_hh, T, N, I, H, hseq, ldh, save, save_bytes, workspace, workspace_bytes, stream);
}
extern "C" int fsn_gru_bilayer_forward(const float* x, long ldx, const float* w_ih, const float* w_hh, const float* b_ih,
                                       const float* b_hh, int T, int N, int I, int H, float* hseq, long ldh, void* save,
                                       size_t save_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return bilayer_forward(3, x, ldx, w_ih, w_hh, b_ih, b_hh, T, N, I, H, hseq, ldh, save, save_bytes, workspace, workspace_bytes, stream);
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// The weight-gradient sums of a direction run over its rows in the order ITS recurrence visited them: for the reverse
// direction the gate gradients, the input and its hidden states are first copied frame-reversed (fsn_launch_time_flip),
// so that a direction's gradients are the same bits in either slot.  Three copies per call that a product with a reversed
// row order would save; see DESIGN 9.
struct BiBwdBufs {
    float *whhT_p, *wihT_p, *dg, *dghn, *carry, *dx_part, *dg_flip, *dghn_flip, *x_flip, *h_flip;
    void* scratch;
};
static size_t bilayer_bwd_carve(void* ws, int T, int N, int I, int H, int g, BiBwdBufs* b) {
    const size_t G = (size_t)g * H, Ipad = fsn_round_up(I, 16), rows = (size_t)T * N;
    Carver cv(ws);
    b->whhT_p = cv.take<float>(2 * H * G);
    b->wihT_p = cv.take<float>(Ipad * 2 * G);
    b->dg = cv.take<float>(rows * 2 * G);
    b->dghn = cv.take<float>(g == 3 ? 2 * rows * H : 0);
    b->carry = cv.take<float>((size_t)2 * N * H);
    b->dx_part = cv.take<float>(2 * rows * Ipad);  // each direction's share of dX
    b->dg_flip = cv.take<float>(rows * G);
    b->dghn_flip = cv.take<float>(g == 3 ? rows * H : 0);
    b->x_flip = cv.take<float>(rows * Ipad);
    b->h_flip = cv.take<float>(rows * H);
    size_t sc = fsn_gemm_tn_workspace_bytes((int)G, I, (long)rows);
    for (const int m : {(int)G, 2 * H, H}) {
        const size_t t = fsn_gemm_tn_workspace_bytes(m, H, (long)rows), c = fsn_colsum_workspace_bytes(m, (long)rows);
        sc = sc > t ? sc : t;
        sc = sc > c ? sc : c;
    }
    b->scratch = cv.take<char>(sc);
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" size_t fsn_lstm_bilayer_bwd_workspace_bytes(int T, int N, int I, int H) {
    BiBwdBufs b{};
    return bi_shape_ok(T, N, I, H) ? bilayer_bwd_carve(nullptr, T, N, I, H, 4, &b) : 0;
}
extern "C" size_t fsn_gru_bilayer_bwd_workspace_bytes(int T, int N, int I, int H) {
    BiBwdBufs b{};
    return bi_shape_ok(T, N, I, H) ? bilayer_bwd_carve(nullptr, T, N, I, H, 3, &b) : 0;
}

static int bilayer_backward(int g, const float* dh, long lddh, const float* x, long ldx, const float* w_ih, const float* w_hh,
                            int T, int N, int I, int H, const float* hseq, long ldh, const void* save, float* dx, long lddx,
                            float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace, size_t workspace_bytes,
                            void* stream) {
    CallScope scope(stream);
    g_bi_step_launches = 0;
    FSN_TRY(check_bilayer(T, N, I, H, ldx, ldh, "hseq"));
    FSN_REQUIRE(lddh >= 2 * (long)H && lddh % 4 == 0, "bilayer: dh row stride %ld must be >= 2 H = %d and 16-byte aligned", lddh, 2 * H);
    FSN_REQUIRE(dh && x && w_ih && w_hh && hseq && save && dw_ih && dw_hh && db_ih && (g == 4 || db_hh) && workspace,
                "NULL pointer argument");
    FSN_REQUIRE(!dx || lddx >= I, "dx row stride %ld < I", lddx);
    BiBwdBufs b{};
    if (workspace_bytes < bilayer_bwd_carve(nullptr, T, N, I, H, g, &b)) {
        fsn_set_error("bilayer backward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = g * H;
    const size_t rows = (size_t)T * N, nh = (size_t)N * H;
    bilayer_bwd_carve(workspace, T, N, I, H, g, &b);
    // W_hh^T and W_ih^T of each direction
    for (int d = 0; d < 2; ++d) {
        FSN_TRY(fsn_launch_pack(w_hh + (size_t)d * G * H, b.whhT_p + (size_t)d * H * G, H, G, H, G, s, 1, H));
        FSN_TRY(fsn_launch_pack(w_ih + (size_t)d * G * I, b.wihT_p + (size_t)d * Ipad * G, I, G, Ipad, G, s, 1, I));
    }
    FsnBiBptt B{};
    B.dh = dh;
    B.lddh = lddh;
    B.hseq = hseq;
    B.ldh = ldh;
    B.dg = b.dg;
    B.T = T;
    B.N = N;
    B.H = H;
    const size_t dir_save = rows * (g == 4 ? 5 : 4) * H;
    for (int d = 0; d < 2; ++d) {
        B.whhT_p[d] = b.whhT_p + (size_t)d * H * G;
        B.save[d] = static_cast<const float*>(save) + d * dir_save;
        B.dghn[d] = b.dghn + d * rows * H;
        B.carry[d] = b.carry + d * nh;
    }
    for (int st = 0; st < T; ++st) {
        FSN_TRY(g == 4 ? fsn_launch_bilstm_bptt_step(B, st, s) : fsn_launch_bigru_bptt_step(B, st, s));
        ++g_bi_step_launches;
    }
    if (dx) {
        // dX = dg_f W_ih_f + dg_r W_ih_r as two products of K = g H and one add.  As ONE product over the concatenated gate
        // gradients (K = 2 g H = 3072 at the production widths) the single fp32 chain missed the sweep's rule: max error
        // 4.6 x torch's fp32 on the GRU at H = 512, 3.1 x on the LSTM at H = 384 (tests/test_gpu_birnn.py, allowed 4 x)
        for (int d = 0; d < 2; ++d)
            FSN_TRY(fsn_launch_gemm(gemm_a_rows(b.dg + (size_t)d * G, 2 * G), b.wihT_p + (size_t)d * Ipad * G,
                                    gemm_c_rows(b.dx_part + d * rows * Ipad, Ipad, T * N, I), T * (N / 16), Ipad / 16, G / 16, s));
        FSN_TRY(fsn_launch_add_rows(b.dx_part, b.dx_part + rows * Ipad, Ipad, dx, lddx, (long)rows, I, s));
    }
    // the reverse direction's operands in step order
    FSN_TRY(fsn_launch_time_flip(b.dg + G, 2 * G, b.dg_flip, G, T, N, G, s));
    FSN_TRY(fsn_launch_time_flip(x, ldx, b.x_flip, Ipad, T, N, Ipad, s));
    FSN_TRY(fsn_launch_time_flip(hseq + H, ldh, b.h_flip, H, T, N, H, s));
    if (g == 3) FSN_TRY(fsn_launch_time_flip(b.dghn + rows * H, H, b.dghn_flip, H, T, N, H, s));
    for (int d = 0; d < 2; ++d) {
        // direction d's gate gradients, input and hidden states as [T][N][.] matrices in its step order
        const float* dg = d ? b.dg_flip : b.dg;
        const long ldg = d ? G : 2 * G;
        const float* dghn = d ? b.dghn_flip : b.dghn;
        const float* xs = d ? b.x_flip : x;
        const long ldxs = d ? Ipad : ldx;
        const float* hs = d ? b.h_flip : hseq;
        const long ldhs = d ? H : ldh;
        float* dwi = dw_ih + (size_t)d * G * I;
        float* dwh = dw_hh + (size_t)d * G * H;
        if (g == 4) {
            FSN_TRY(fsn_launch_gemm_tn(dg, ldg, xs, ldxs, dwi, I, G, I, (long)rows, b.scratch, s, db_ih + (size_t)d * G));
            if (T > 1) FSN_TRY(fsn_launch_gemm_tn(dg + (size_t)N * ldg, ldg, hs, ldhs, dwh, H, G, H, (long)(T - 1) * N, b.scratch, s));
        } else {
            FSN_TRY(fsn_launch_gemm_tn(dg, ldg, xs, ldxs, dwi, I, G, I, (long)rows, b.scratch, s));
            if (T > 1) {  // rows r, z from the x-side derivatives (identical on the h side), rows n from dghn
                FSN_TRY(fsn_launch_gemm_tn(dg + (size_t)N * ldg, ldg, hs, ldhs, dwh, H, 2 * H, H, (long)(T - 1) * N, b.scratch, s));
                FSN_TRY(fsn_launch_gemm_tn(dghn + nh, H, hs, ldhs, dwh + (size_t)2 * H * H, H, H, H, (long)(T - 1) * N, b.scratch, s));
            }
            FSN_TRY(fsn_launch_colsum(dg, ldg, db_ih + (size_t)d * G, G, (long)rows, b.scratch, s));
            FSN_TRY(fsn_launch_colsum(dg, ldg, db_hh + (size_t)d * G, 2 * H, (long)rows, b.scratch, s));
            FSN_TRY(fsn_launch_colsum(dghn, H, db_hh + (size_t)d * G + 2 * H, H, (long)rows, b.scratch, s));
        }
    }
    if (T == 1 && hipMemsetAsync(dw_hh, 0, (size_t)2 * G * H * sizeof(float), s) != hipSuccess) {
        fsn_set_error("memset failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}

extern "C" int fsn_lstm_bilayer_backward(const float* dh, long lddh, const float* x, long ldx, const float* w_ih, const float* w_hh,
                                         int T, int N, int I, int H, const float* hseq, long ldh, const void* save, float* dx,
                                         long lddx, float* dw_ih, float* dw_hh, float* db, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return bilayer_backward(4, dh, lddh, x, ldx, w_ih, w_hh, T, N, I, H, hseq, ldh, save, dx, lddx, dw_ih, dw_hh, db, nullptr,
                            workspace, workspace_bytes, stream);
}
extern "C" int fsn_gru_bilayer_backward(const float* dh, long lddh, const float* x, long ldx, const float* w_ih, const float* w_hh,
                                        int T, int N, int I, int H, const float* hseq, long ldh, const void* save, float* dx,
                                        long lddx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    return bilayer_backward(3, dh, lddh, x, ldx, w_ih, w_hh, T, N, I, H, hseq, ldh, save, dx, lddx, dw_ih, dw_hh, db_ih, db_hh,
                            workspace, workspace_bytes, stream);
}
