// C ABI of libfsn_hip.so, training: two stacked nn.LSTM layers forward with saved activations and their BPTT, one
// layer's BPTT, and nn.Linear forward / backward.
#include <atomic>

#include "fsn_api_internal.h"

static std::atomic<int> g_g16_off{0};               // fsn_debug_g16_kernels(0): the fp32-era group kernels also under 16-bit arithmetic
static std::atomic<int> g_in16_off{0};              // fsn_debug_g16_kernels(3): dx / dW_ih0 from the fp32 gate gradients (round 5's form)
static std::atomic<int> g_tn16h_off{0};             // fsn_debug_g16_kernels(2): ... only the weight-gradient products of round 3
// Test / measurement hook: 0 = the fp32-era group kernels also under the 16-bit training arithmetic (A/B against
// lstm_group16_kernels.hip), 1 (default) = the 16-bit arithmetic's own kernels where they apply.
extern "C" int fsn_debug_g16_kernels(int on) {
    g_g16_off.store(on == 0 ? 1 : 0, std::memory_order_relaxed);
    g_tn16h_off.store(on == 2 ? 1 : 0, std::memory_order_relaxed);
    g_in16_off.store(on == 3 ? 1 : 0, std::memory_order_relaxed);
    return FSN_OK;
}

// ---- training: two stacked nn.LSTM layers of equal width, forward with saved activations ----------------------
// (sequence_model.py:52-58 with num_layers = 2, under autograd: fullsubnet/trainer.py:56-63).  The result is that of two
// fsn_lstm_layer_forward calls; what it adds is the persistent kernels: the full-band shape (H = 512, up to 64 rows)
// runs on fb_chain_kernel, one launch for both layers and all steps instead of 2 T.
// ONE plan for both directions of the two-layer training entries (fsn_lstm2_forward_train, fsn_lstm2_backward and their
// workspace queries).  Forward and backward may land on different kernels - every path reads and writes the one save
// layout of fsn_lstm_layer_forward (gates [T][N][4H] | cell sequence [T][N][H]) and the one hseq layout - so each
// direction only has to honour its own kernel's bounds, all of which live here:
//   fwd_group  : clusters of lstm2_group_kernel<.., TRAIN, SAVE> - H = 384, 17 - 32 input columns, 96+ row tiles that
//                fill whole 64-row clusters up to 8 left-over tiles, hidden sequence within a buffer resource's 2 GB;
//   fwd_chain  : fb_chain_kernel<.., SAVE> - H = 384 / 512, up to 64 rows, up to 4095 steps (its hand-off offsets);
//   bptt_group : clusters of lstm2_group_bptt_kernel - H = 384, the same row shape, any input width (dX is a GEMM
//                afterwards) and any T (one buffer resource per (step, cluster) tile);
//   bptt_chain : fb_chain_bptt_kernel - H = 512, 16 .. 80 rows (one chain per row tile), T below fsn_fb_chain_bptt_max_steps
//                (32-bit dx offsets).
struct Lstm2TrainPlan {
    int fwd_group, bptt_group;
    bool fwd_chain, bptt_chain;
};
static Lstm2TrainPlan lstm2_train_plan(int T, int N, int I, int H) {
    Lstm2TrainPlan p{0, 0, false, false};
    const int tiles = N / 16;
    if (H == 384 && tiles >= kWavefrontBelowTiles) {
        const int cf = fsn_lstm2_group_clusters(tiles), cb = fsn_lstm2_group_bptt_clusters(tiles);
        if (fsn_round_up(I, 16) == 32 && (size_t)T * N * H * sizeof(float) <= 0x7fffffffull && cf > 0 && tiles - 4 * cf <= 8)
            p.fwd_group = cf;
        if (cb > 0 && tiles - 4 * cb <= 8) p.bptt_group = cb;
    }
    p.fwd_chain = !p.fwd_group && lstm2_on_chain(T, N, H);
    p.bptt_chain = !p.bptt_group && fsn_fb_chain_bptt_supported(H, N) && T <= fsn_fb_chain_bptt_max_steps();
    return p;
}
static int lstm2_train_group_clusters(int T, int N, int I, int H) { return lstm2_train_plan(T, N, I, H).fwd_group; }
extern "C" int fsn_lstm2_train_is_persistent(int T, int N, int I, int H) {
    if (T < 1 || N < 16 || N % 16 || I < 1 || H < 1) return 0;
    const Lstm2TrainPlan p = lstm2_train_plan(T, N, I, H);
    return ((p.fwd_group > 0 || p.fwd_chain) && (p.bptt_group > 0 || p.bptt_chain)) ? 1 : 0;
}
// the 16-bit arithmetic has kernels of its own for the group shapes (lstm_group16_kernels.hip) when they take the same
// clusters; the flag array is sized for either family
static bool lstm2_use_g16(int arith, int clusters, int N) {
    return arith != FSN_ARITH_F32 && clusters > 0 && fsn_lstm2_g16_clusters(N / 16) >= clusters && !g_g16_off.load(std::memory_order_relaxed);
}
// ONE plan of the 16-bit training arithmetic for both directions, computed here and nowhere else: which kernels a call of
// fsn_lstm2_forward_train / fsn_lstm2_backward under `arith` (with or without FSN_ARITH_SAVES16) lands on.  Each direction
// has its own clusters (Lstm2TrainPlan); a direction without clusters runs layer by layer or on the chain, in fp32.
struct Lstm2Plan16 {
    int fwd_clusters, bwd_clusters;  // 64-row clusters of the group launch of each direction (0: none)
    int fwd_left, bwd_left;          // rows beside that launch, step by step in fp32
    bool fwd16, bwd16;               // the direction runs in the 16-bit arithmetic at all
    bool g16_fwd, g16_bptt;          // ... on lstm_group16_kernels.hip (else: the `arith` forms of the fp32-era group kernels)
    bool tn16h;                      // the three large weight-gradient products from 16-bit operands in memory
    int tn16h_form;                  // of the K = (T - 1) N products: 0 none, 1 the 192 x 192 form, 2 the 192 x 384 form
    bool in16;                       // ... and layer 0's input-side products (dx, dW_ih0) too
    bool h16_saved;                  // the products read the 16-bit h_t the forward launch left in the save slots
    // FSN_ARITH_SAVES16 in force: only where BOTH directions run on lstm_group16_kernels.hip, the one pair that writes and reads
    // the 16-bit gate slots.  (The flag used to reach the 16-bit BPTT launch whatever the forward had done: with 1 - 16 or 33+
    // input columns the forward runs layer by layer and saves fp32 gates, which that launch then decoded as 16-bit ones.)
    bool saves16;
};
static Lstm2Plan16 lstm2_plan16(int T, int N, int I, long ldx, int H, int arith) {
    const bool saves16_asked = (arith & FSN_ARITH_SAVES16) != 0;
    arith &= ~FSN_ARITH_SAVES16;
    const Lstm2TrainPlan tp = lstm2_train_plan(T, N, I, H);
    const int G = 4 * H;
    Lstm2Plan16 p{};
    p.fwd_clusters = tp.fwd_group;
    p.bwd_clusters = tp.bptt_group;
    p.fwd_left = tp.fwd_group ? N - 64 * tp.fwd_group : 0;
    p.bwd_left = tp.bptt_group ? N - 64 * tp.bptt_group : 0;
    p.fwd16 = arith != FSN_ARITH_F32 && tp.fwd_group > 0;
    p.bwd16 = arith != FSN_ARITH_F32 && tp.bptt_group > 0;
    p.g16_fwd = lstm2_use_g16(arith, tp.fwd_group, N);
    p.g16_bptt = lstm2_use_g16(arith, tp.bptt_group, N);
    // the weight-gradient products from 16-bit operands in memory (needs the shapes' one-workgroup-per-CU plan - for BOTH K:
    // dW_hh sums (T - 1) N rows, dW_ih1 T N, and a plan exists only for some K (every split non-empty); asking for the first
    // alone made fsn_lstm2_backward fail with "gemm_tn16h: no plan" at e.g. T = 2, N = 2064 or T = 3, N = 1728 on 256 CUs)
    p.tn16h = p.g16_bptt && T > 1 && fsn_gemm_tn16h_supported(G, H, (long)(T - 1) * N) && fsn_gemm_tn16h_supported(G, H, (long)T * N) &&
              !g_tn16h_off.load(std::memory_order_relaxed);
    p.tn16h_form = p.tn16h ? fsn_gemm_tn16h_form(G, H, (long)(T - 1) * N, nullptr) : 0;
    // ... and layer 0's input-side products too (dx, dW_ih0): then the BPTT launch stores no fp32 gate gradients at all
    p.in16 = p.tn16h && fsn_gemm_tn16n_supported(G, I, (long)T * N) && fsn_gemm_dx16_supported((long)T * N, G, I) && ldx == 32 &&
             !g_in16_off.load(std::memory_order_relaxed);
    p.saves16 = saves16_asked && p.g16_fwd && p.g16_bptt;
    // under FSN_ARITH_SAVES16 the forward launch left h_t in 16 bits inside the save buffers (second half of a row's gate slot)
    // for every cluster row - with no step-by-step rows beside the launch the hidden sequences need no conversion pass at all
    p.h16_saved = p.tn16h && p.saves16 && p.bwd_left == 0;
    return p;
}
// Test hook: that plan as integers (include/fsn_hip.h lists the fields)
extern "C" int fsn_debug_lstm2_plan16(int T, int N, int I, long ldx, int H, int arith, int* out, int n) {
    const int base = arith & ~FSN_ARITH_SAVES16;
    if (T < 1 || N < 16 || N % 16 || I < 1 || H < 1 || ldx < I || !out || n < 1 ||
        (base != FSN_ARITH_F32 && base != FSN_ARITH_F16 && base != FSN_ARITH_BF16))
        return -1;
    const Lstm2Plan16 p = lstm2_plan16(T, N, I, ldx, H, arith);
    const int v[13] = {p.fwd16, p.bwd16, p.g16_fwd, p.g16_bptt, p.tn16h, p.tn16h_form, p.in16, p.h16_saved,
                       p.bwd_left, p.bwd_clusters, p.fwd_left, p.fwd_clusters, p.saves16};
    const int m = n < 13 ? n : 13;
    for (int i = 0; i < m; ++i) out[i] = v[i];
    return m;
}
static size_t lstm2_group_flag_words_any(int clusters) {
    size_t a = fsn_lstm2_group_flag_words(clusters), b = fsn_lstm2_g16_flag_words(clusters), c = fsn_lstm2_group_bptt_flag_words(clusters);
    a = a > b ? a : b;
    return a > c ? a : c;
}
extern "C" size_t fsn_lstm2_train_workspace_bytes(int T, int N, int I, int H, int arith) {
    arith &= ~FSN_ARITH_SAVES16;
    const int Ipad = fsn_round_up(I, 16);
    Carver cv(nullptr);
    if (const int clusters = lstm2_train_group_clusters(T, N, I, H)) {
        const size_t left = (size_t)(N / 16 - 4 * clusters) * 16;
        cv.take<float>((size_t)4 * H * Ipad + (size_t)3 * 4 * H * H);
        cv.take<float>((size_t)2 * 4 * H);
        cv.take<unsigned>(lstm2_group_flag_words_any(clusters));
        cv.take<float>((size_t)T * left * Ipad);
        cv.take<float>((size_t)T * left * H);
        cv.take<float>((size_t)T * left * 4 * H);
        if (arith != FSN_ARITH_F32) cv.take<unsigned short>((size_t)4 * H * Ipad + (size_t)3 * 4 * H * H);  // 16-bit weights
        return fsn_round_up_sz(cv.off, 256);
    }
    if (lstm2_train_plan(T, N, I, H).fwd_chain) {
        cv.take<float>((size_t)4 * H * Ipad);
        cv.take<float>((size_t)3 * 4 * H * H);
        cv.take<float>((size_t)2 * 4 * H);
        cv.take<float>((size_t)T * N * 4 * H);
        cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
        cv.take<unsigned>(fsn_fb_chain_flag_words());
        return fsn_round_up_sz(cv.off, 256);
    }
    const size_t l0 = fsn_lstm_layer_fwd_workspace_bytes(T, N, I, H), l1 = fsn_lstm_layer_fwd_workspace_bytes(T, N, H, H);
    return l0 > l1 ? l0 : l1;
}
extern "C" int fsn_lstm2_forward_train(const float* x, long ldx, const float* w_ih0, const float* w_hh0,
                                       const float* b_ih0, const float* b_hh0, const float* w_ih1, const float* w_hh1,
                                       const float* b_ih1, const float* b_hh1, int T, int N, int I, int H, float* hseq0,
                                       float* hseq1, void* save0, void* save1, size_t save_bytes, void* workspace,
                                       size_t workspace_bytes, int arith, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    const int saves16 = arith & FSN_ARITH_SAVES16;  // only meaningful with a 16-bit arithmetic; passed on to the g16 launch
    arith &= ~FSN_ARITH_SAVES16;
    FSN_REQUIRE((arith == FSN_ARITH_F32 && !saves16) || arith == FSN_ARITH_F16 || arith == FSN_ARITH_BF16,
                "lstm2 forward (training): arithmetic %d unknown (FSN_ARITH_F32 / _F16 / _BF16 [| FSN_ARITH_SAVES16])", arith | saves16);
    FSN_REQUIRE(x && w_ih0 && w_hh0 && b_ih0 && b_hh0 && w_ih1 && w_hh1 && b_ih1 && b_hh1 && hseq0 && hseq1 && save0 &&
                    save1 && workspace,
                "NULL pointer argument");
    if (save_bytes < fsn_lstm_layer_save_bytes(T, N, H) || workspace_bytes < fsn_lstm2_train_workspace_bytes(T, N, I, H, arith)) {
        fsn_set_error("lstm2 forward (training): save / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16);
    if (const int clusters = lstm2_train_group_clusters(T, N, I, H)) {
        // whole 64-row clusters on the group kernel (both layers, one launch); the few rows that do not fill a cluster
        // step by step on the auxiliary stream beside it, straight into the same output buffers
        const int left_tiles = N / 16 - 4 * clusters, left = left_tiles * 16, row0 = 64 * clusters;
        FSN_REQUIRE(ldx == Ipad, "lstm2 forward (training): this shape needs x rows of exactly %d columns (got %ld)", Ipad, ldx);
        Carver cv(workspace);
        float* wih0_p = cv.take<float>((size_t)4 * H * Ipad + (size_t)3 * 4 * H * H);
        float* whh0_p = wih0_p + (size_t)4 * H * Ipad;
        float* wih1_p = whh0_p + (size_t)4 * H * H;
        float* whh1_p = wih1_p + (size_t)4 * H * H;
        float* b0 = cv.take<float>((size_t)2 * 4 * H);
        float* b1 = b0 + 4 * H;
        unsigned* flags = cv.take<unsigned>(lstm2_group_flag_words_any(clusters));
        float* x_left = cv.take<float>((size_t)T * left * Ipad);
        float* h0_left = cv.take<float>((size_t)T * left * H);
        float* gx_left = cv.take<float>((size_t)T * left * 4 * H);
        const size_t wfloats = (size_t)4 * H * Ipad + (size_t)3 * 4 * H * H;
        unsigned short* w16 = arith != FSN_ARITH_F32 ? cv.take<unsigned short>(wfloats) : nullptr;
        const Lstm2Plan16 p16 = lstm2_plan16(T, N, I, ldx, H, arith | saves16);
        const bool g16 = p16.g16_fwd;
        if (!g16 || left > 0) {  // the fp32-fragment weights: the group kernel's and the step-by-step rows' (the 16-bit kernels pack their own)
            FSN_TRY(fsn_launch_pack(w_ih0, wih0_p, 4 * H, I, 4 * H, Ipad, s));
            FSN_TRY(fsn_launch_pack(w_hh0, whh0_p, 4 * H, H, 4 * H, H, s));
            FSN_TRY(fsn_launch_pack(w_ih1, wih1_p, 4 * H, H, 4 * H, H, s));
            FSN_TRY(fsn_launch_pack(w_hh1, whh1_p, 4 * H, H, 4 * H, H, s));
        }
        FSN_TRY(fsn_launch_bias_sum(b_ih0, b_hh0, b0, 4 * H, 4 * H, s));
        FSN_TRY(fsn_launch_bias_sum(b_ih1, b_hh1, b1, 4 * H, 4 * H, s));
        if (w16 && !g16) FSN_TRY(fsn_launch_to16(wih0_p, w16, wfloats, arith, s));  // the group kernel's weight fragments in 16 bits
        float* sv0 = static_cast<float*>(save0);
        float* sv1 = static_cast<float*>(save1);
        hipStream_t as = s;
        if (left > 0) FSN_TRY(aux_fork(s, &as));
        {
            FSN_PERSIST_BEGIN(s);
            if (g16) {  // the 16-bit arithmetic's own kernels: they pack the raw weights their way into w16
                FSN_TRY(fsn_launch_lstm2_g16_train(x, I, N, w_ih0, w_hh0, w_ih1, w_hh1, b0, b1, hseq0, hseq1, sv0, sv1, flags, w16,
                                                   T, clusters, H, s, arith | (p16.saves16 ? FSN_ARITH_SAVES16 : 0)));
                FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_g16_status_word(clusters), hseq1, (size_t)T * N * H, s));
            } else {
                FSN_TRY(fsn_launch_lstm2_group_train(x, ldx, 32, N, wih0_p, whh0_p, wih1_p, whh1_p, b0, b1, hseq0, hseq1, sv0,
                                                     sv1, flags, T, clusters, H, s, arith, w16));
                FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_group_status_word(clusters), hseq1, (size_t)T * N * H, s));
            }
        }
        if (left > 0) {
            const size_t stepH = (size_t)N * H, stepG = (size_t)N * 4 * H;
            for (int layer = 0; layer < 2; ++layer) {
                // the left-over rows of this layer's input as a compact [T][left][K] matrix -> projection tiles
                const int K = layer ? H : Ipad;
                float* dst = layer ? h0_left : x_left;
                FSN_TRY(gather_step_rows(dst, layer ? hseq0 : x, layer ? H : ldx, T, N, row0, left, K, as));
                FSN_TRY(fsn_launch_gemm(gemm_a_rows(dst, K), layer ? wih1_p : wih0_p, gemm_c_frag(gx_left, layer ? b1 : b0),
                                        T * left_tiles, 4 * H / 16, K / 16, as));
                float* hs = (layer ? hseq1 : hseq0) + (size_t)row0 * H;
                float* sv = layer ? sv1 : sv0;
                float* gates = sv + (size_t)row0 * 4 * H;
                float* cseq = sv + (size_t)T * N * 4 * H + (size_t)row0 * H;
                for (int t = 0; t < T; ++t)
                    FSN_TRY(fsn_launch_lstm_step_train(gx_left, layer ? whh1_p : whh0_p, t ? hs + (t - 1) * stepH : hs,
                                                       hs + t * stepH, t ? cseq + (t - 1) * stepH : cseq, cseq + t * stepH,
                                                       gates + t * stepG, (long)t * left_tiles, left_tiles, H, t == 0, as));
            }
            FSN_TRY(aux_join(s));
        }
        return FSN_OK;
    }
    if (!lstm2_train_plan(T, N, I, H).fwd_chain) {  // layer by layer
        FSN_TRY(fsn_lstm_layer_forward(x, ldx, w_ih0, w_hh0, b_ih0, b_hh0, T, N, I, H, hseq0, save0, save_bytes, workspace,
                                       workspace_bytes, stream));
        return fsn_lstm_layer_forward(hseq0, H, w_ih1, w_hh1, b_ih1, b_hh1, T, N, H, H, hseq1, save1, save_bytes, workspace,
                                      workspace_bytes, stream);
    }
    Carver cv(workspace);
    float* wih0_p = cv.take<float>((size_t)4 * H * Ipad);
    float* whh0_p = cv.take<float>((size_t)4 * H * H);
    float* wih1_p = whh0_p + (size_t)4 * H * H;
    float* whh1_p = wih1_p + (size_t)4 * H * H;
    cv.take<float>((size_t)2 * 4 * H * H);
    float* b0 = cv.take<float>((size_t)2 * 4 * H);
    float* b1 = b0 + 4 * H;
    float* gx0 = cv.take<float>((size_t)T * N * 4 * H);
    float* exchange = cv.take<float>(fsn_fb_chain_exchange_floats(T, N));
    unsigned* flags = cv.take<unsigned>(fsn_fb_chain_flag_words());
    FSN_TRY(fsn_launch_pack(w_ih0, wih0_p, 4 * H, I, 4 * H, Ipad, s));
    FSN_TRY(fsn_launch_pack(w_hh0, whh0_p, 4 * H, H, 4 * H, H, s));
    FSN_TRY(fsn_launch_pack(w_ih1, wih1_p, 4 * H, H, 4 * H, H, s));
    FSN_TRY(fsn_launch_pack(w_hh1, whh1_p, 4 * H, H, 4 * H, H, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih0, b_hh0, b0, 4 * H, 4 * H, s));
    FSN_TRY(fsn_launch_bias_sum(b_ih1, b_hh1, b1, 4 * H, 4 * H, s));
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(x, ldx), wih0_p, gemm_c_frag(gx0, b0), T * (N / 16), 4 * H / 16, Ipad / 16, s));
    FSN_PERSIST_BEGIN(s);
    FSN_TRY(fsn_launch_fb_chain(gx0, whh0_p, wih1_p, whh1_p, b1, exchange, flags, hseq1, T, N, H, s, hseq0,
                                static_cast<float*>(save0), static_cast<float*>(save1)));
    return fsn_launch_poison_if(flags + fsn_fb_chain_status_word(), hseq1, (size_t)T * N * H, s);
}

extern "C" size_t fsn_lstm_layer_bwd_workspace_bytes(int T, int N, int I, int H) {
    const int Ipad = fsn_round_up(I, 16);
    Carver cv(nullptr);
    cv.take<float>((size_t)H * 4 * H);          // W_hh^T fragments
    cv.take<float>((size_t)Ipad * 4 * H);       // W_ih^T fragments
    cv.take<float>((size_t)T * N * 4 * H);      // dgates
    cv.take<float>((size_t)N * H);              // dh_rec
    cv.take<float>((size_t)N * H);              // dc
    size_t tn = fsn_gemm_tn_workspace_bytes(4 * H, I, (long)T * N);
    const size_t tn2 = fsn_gemm_tn_workspace_bytes(4 * H, H, (long)T * N);
    tn = tn > tn2 ? tn : tn2;
    const size_t cs = fsn_colsum_workspace_bytes(4 * H, (long)T * N);
    cv.take<char>(tn > cs ? tn : cs);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_lstm_layer_backward(const float* dh, const float* x, long ldx, const float* w_ih,
                                       const float* w_hh, int T, int N, int I, int H, const float* hseq,
                                       const void* save, float* dx, long lddx, float* dw_ih, float* dw_hh, float* db,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    FSN_REQUIRE(dh && x && w_ih && w_hh && hseq && save && dw_ih && dw_hh && db && workspace, "NULL pointer argument");
    FSN_REQUIRE(!dx || lddx >= I, "dx row stride %ld < I", lddx);
    if (workspace_bytes < fsn_lstm_layer_bwd_workspace_bytes(T, N, I, H)) {
        fsn_set_error("lstm layer backward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = 4 * H;
    Carver cv(workspace);
    float* whhT_p = cv.take<float>((size_t)H * G);
    float* wihT_p = cv.take<float>((size_t)Ipad * G);
    float* dgates = cv.take<float>((size_t)T * N * G);
    float* dh_rec = cv.take<float>((size_t)N * H);
    float* dc = cv.take<float>((size_t)N * H);
    size_t tn = fsn_gemm_tn_workspace_bytes(G, I, (long)T * N);
    const size_t tn2 = fsn_gemm_tn_workspace_bytes(G, H, (long)T * N);
    tn = tn > tn2 ? tn : tn2;
    const size_t cs = fsn_colsum_workspace_bytes(G, (long)T * N);
    void* scratch = cv.take<char>(tn > cs ? tn : cs);
    const float* gates = static_cast<const float*>(save);
    const float* cseq = gates + (size_t)T * N * G;
    // "weights" of dh_rec = dgates W_hh are W_hh^T: out = H columns, k = 4H; nn.LSTM stores exactly
    // that transposed ([4H][H] = [k][out]).  Likewise W_ih^T for dX.
    FSN_TRY(fsn_launch_pack(w_hh, whhT_p, H, G, H, G, s, 1, H));
    FSN_TRY(fsn_launch_pack(w_ih, wihT_p, I, G, Ipad, G, s, 1, I));
    const size_t step = (size_t)N * H;
    // one fused launch per step: dh_rec = dgates_{t+1} W_hh, then the cell derivative -> dgates_t
    for (int t = T - 1; t >= 0; --t)
        FSN_TRY(fsn_launch_bptt_step(dh + t * step, t + 1 < T ? dgates + (size_t)(t + 1) * N * G : dgates, whhT_p, dc,
                                     gates + (size_t)t * N * G, cseq + t * step, t ? cseq + (t - 1) * step : cseq,
                                     dgates + (size_t)t * N * G, N / 16, H, t == T - 1, t == 0, s));
    (void)dh_rec;
    if (dx)
        FSN_TRY(fsn_launch_gemm(gemm_a_rows(dgates, G), wihT_p, gemm_c_rows(dx, lddx, T * N, I), T * (N / 16), Ipad / 16, G / 16, s));
    // dW_ih = dgates^T X and, from the same pass over dgates, db = its column sums
    FSN_TRY(fsn_launch_gemm_tn(dgates, G, x, ldx, dw_ih, I, G, I, (long)T * N, scratch, s, db));
    if (T > 1) {
        FSN_TRY(fsn_launch_gemm_tn(dgates + (size_t)N * G, G, hseq, H, dw_hh, H, G, H, (long)(T - 1) * N, scratch, s));
    } else if (hipMemsetAsync(dw_hh, 0, (size_t)G * H * sizeof(float), s) != hipSuccess) {
        fsn_set_error("memset failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}

// ---- training: backward of two stacked layers (the counterpart of fsn_lstm2_forward_train) ------------------------
// Two fsn_lstm_layer_backward calls in one; the sub-band shape runs its BPTT - both layers, all steps, the
// layer-to-layer dX included - as ONE persistent launch (lstm_group_bptt_kernels.hip).
static int lstm2_bptt_group_clusters(int T, int N, int I, int H) { return lstm2_train_plan(T, N, I, H).bptt_group; }
extern "C" size_t fsn_lstm2_bwd_workspace_bytes(int T, int N, int I, int H, int arith) {
    arith &= ~FSN_ARITH_SAVES16;
    const int Ipad = fsn_round_up(I, 16), G = 4 * H;
    const size_t l1 = fsn_lstm_layer_bwd_workspace_bytes(T, N, H, H), l0 = fsn_lstm_layer_bwd_workspace_bytes(T, N, I, H);
    Carver cv(nullptr);
    if (const int clusters = lstm2_bptt_group_clusters(T, N, I, H)) {
        const size_t left = (size_t)(N / 16 - 4 * clusters) * 16;
        cv.take<float>((size_t)3 * H * G + (size_t)Ipad * G);  // W_hh1^T, W_ih1^T, W_hh0^T, W_ih0^T fragments
        cv.take<float>((size_t)2 * T * N * G);                 // dgates of both layers
        cv.take<float>((size_t)T * N * H);                     // layer 0's dH (dgates1 W_ih1), produced by the kernel
        cv.take<unsigned>(lstm2_group_flag_words_any(clusters));
        cv.take<float>((size_t)T * left * G);                  // left-over rows: compact dgates1
        cv.take<float>((size_t)T * left * H);                  // ... their dh0
        cv.take<float>((size_t)left * H);                      // ... dc
        size_t tn = fsn_gemm_tn_workspace_bytes(G, I, (long)T * N);
        const size_t tn2 = fsn_gemm_tn_workspace_bytes(G, H, (long)T * N);
        cv.take<char>(tn > tn2 ? tn : tn2);
        if (arith != FSN_ARITH_F32) cv.take<unsigned short>((size_t)3 * H * G);  // 16-bit W^T fragments
        if (arith != FSN_ARITH_F32) {  // lstm_group16_kernels.hip: its packed weights and the rings of exchanged gate-gradient tiles
            cv.take<char>(fsn_lstm2_g16_bwd_weight_bytes());
            cv.take<float>(fsn_lstm2_g16_partial_floats(clusters));
            cv.take<unsigned short>((size_t)2 * T * N * G);  // 16-bit gate gradients: operands of the weight-gradient products
            cv.take<unsigned short>((size_t)2 * T * N * H);  // 16-bit hidden sequences
            cv.take<float>((size_t)2 * clusters * G);        // bias-gradient sums per (layer, cluster)
            cv.take<unsigned short>((size_t)T * N * 32 + (size_t)G * 32);  // x in 16 bits | W_ih0 fragments (gemm_tn16n / gemm_dx16)
        }
        return fsn_round_up_sz(cv.off, 256);
    }
    if (lstm2_train_plan(T, N, I, H).bptt_chain) {
        cv.take<float>((size_t)3 * H * G + (size_t)Ipad * G);  // W_hh1^T, W_ih1^T, W_hh0^T, W_ih0^T fragments
        cv.take<float>((size_t)2 * T * N * G);                 // dgates of both layers
        cv.take<float>(fsn_fb_chain_bptt_dx_floats(T, N));
        cv.take<unsigned>(fsn_fb_chain_bptt_flag_words());
        size_t tn = fsn_gemm_tn_workspace_bytes(G, I, (long)T * N);
        const size_t tn2 = fsn_gemm_tn_workspace_bytes(G, H, (long)T * N);
        cv.take<char>(tn > tn2 ? tn : tn2);
        return fsn_round_up_sz(cv.off, 256);
    }
    cv.take<float>((size_t)T * N * H);  // dh0
    cv.take<char>(l1 > l0 ? l1 : l0);
    return fsn_round_up_sz(cv.off, 256);
}
// `phase`: which parts run (a sum; 7 = everything) - 1: back-propagation through time, the gate gradients stay in the
// workspace; 4: dx from them; 2: the weight- and bias-gradient products from them; 8: only what the products need BESIDES
// the gate gradients (the 16-bit copies of the hidden sequences: independent of part 1, so a caller can have them made on
// another stream while part 1 runs); 16 (with 2): a part-8 call has done that.  Parts 2 and 4 take the same arguments
// and the same workspace, untouched since part 1; either may be issued on another stream, ordered behind part 1 by the
// caller.  The persistent shapes only (sub-band group kernels, full-band chain): the layer-by-layer form runs whole in
// part 1.
static int lstm2_backward_phases(const float* dh1, const float* x, long ldx, const float* w_ih0, const float* w_hh0,
                                 const float* w_ih1, const float* w_hh1, int T, int N, int I, int H, const float* hseq0,
                                 const float* hseq1, const void* save0, const void* save1, float* dx, long lddx,
                                 float* dw_ih0, float* dw_hh0, float* db0, float* dw_ih1, float* dw_hh1, float* db1,
                                 void* workspace, size_t workspace_bytes, int arith, void* stream, int phase) {
    CallScope scope(stream);
    const bool chain_part = (phase & 1) != 0, products_part = (phase & 2) != 0, dx_part = (phase & 4) != 0;
    const bool prepare_part = (phase & 8) != 0, prepared = (phase & 16) != 0;
    FSN_TRY(check_lstm_layer(T, N, I, H, ldx));
    const int saves16 = arith & FSN_ARITH_SAVES16;  // must be what the forward call of this step was given
    arith &= ~FSN_ARITH_SAVES16;
    FSN_REQUIRE((arith == FSN_ARITH_F32 && !saves16) || arith == FSN_ARITH_F16 || arith == FSN_ARITH_BF16,
                "lstm2 backward: arithmetic %d unknown (FSN_ARITH_F32 / _F16 / _BF16 [| FSN_ARITH_SAVES16])", arith | saves16);
    FSN_REQUIRE(dh1 && x && w_ih0 && w_hh0 && w_ih1 && w_hh1 && hseq0 && hseq1 && save0 && save1 && dw_ih0 && dw_hh0 && db0 &&
                    dw_ih1 && dw_hh1 && db1 && workspace,
                "NULL pointer argument");
    FSN_REQUIRE(!dx || lddx >= I, "dx row stride %ld < I", lddx);
    if (workspace_bytes < fsn_lstm2_bwd_workspace_bytes(T, N, I, H, arith)) {
        fsn_set_error("lstm2 backward: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    const int clusters = lstm2_bptt_group_clusters(T, N, I, H);
    if (!clusters && lstm2_train_plan(T, N, I, H).bptt_chain) {
        // the full-band shape (H = 512, up to 80 rows): both layers' BPTT as one persistent launch (fb_chain_bptt_kernels.hip),
        // then the weight-gradient GEMMs
        hipStream_t s = static_cast<hipStream_t>(stream);
        const int Ipad = fsn_round_up(I, 16), G = 4 * H;
        Carver cv(workspace);
        float* whh1T_p = cv.take<float>((size_t)3 * H * G + (size_t)Ipad * G);
        float* wih1T_p = whh1T_p + (size_t)H * G;
        float* whh0T_p = wih1T_p + (size_t)H * G;
        float* wih0T_p = whh0T_p + (size_t)H * G;
        float* dg1 = cv.take<float>((size_t)2 * T * N * G);
        float* dg0 = dg1 + (size_t)T * N * G;
        float* dxp = cv.take<float>(fsn_fb_chain_bptt_dx_floats(T, N));
        unsigned* flags = cv.take<unsigned>(fsn_fb_chain_bptt_flag_words());
        size_t tn = fsn_gemm_tn_workspace_bytes(G, I, (long)T * N);
        const size_t tn2 = fsn_gemm_tn_workspace_bytes(G, H, (long)T * N);
        void* scratch = cv.take<char>(tn > tn2 ? tn : tn2);
        if (chain_part) {
            FSN_TRY(fsn_launch_pack(w_hh1, whh1T_p, H, G, H, G, s, 1, H));
            FSN_TRY(fsn_launch_pack(w_ih1, wih1T_p, H, G, H, G, s, 1, H));
            FSN_TRY(fsn_launch_pack(w_hh0, whh0T_p, H, G, H, G, s, 1, H));
            if (dx) FSN_TRY(fsn_launch_pack(w_ih0, wih0T_p, I, G, Ipad, G, s, 1, I));
            FSN_PERSIST_BEGIN(s);
            FSN_TRY(fsn_launch_fb_chain_bptt(dh1, whh1T_p, wih1T_p, whh0T_p, static_cast<const float*>(save0),
                                             static_cast<const float*>(save1), dg0, dg1, dxp, flags, T, N, H, s));
            // both gate-gradient buffers (dg1 | dg0 are adjacent): every weight gradient and dx derive from them
            FSN_TRY(fsn_launch_poison_if(flags + fsn_fb_chain_bptt_status_word(), dg1, (size_t)2 * T * N * G, s));
        }
        if (dx && dx_part) {
            FSN_TRY(fsn_launch_gemm(gemm_a_rows(dg0, G), wih0T_p, gemm_c_rows(dx, lddx, T * N, I), T * (N / 16), Ipad / 16, G / 16, s));
        }
        if (!products_part) return FSN_OK;
        FSN_TRY(fsn_launch_gemm_tn(dg1, G, hseq0, H, dw_ih1, H, G, H, (long)T * N, scratch, s, db1));
        FSN_TRY(fsn_launch_gemm_tn(dg0, G, x, ldx, dw_ih0, I, G, I, (long)T * N, scratch, s, db0));
        if (T > 1) {
            FSN_TRY(fsn_launch_gemm_tn(dg1 + (size_t)N * G, G, hseq1, H, dw_hh1, H, G, H, (long)(T - 1) * N, scratch, s));
            FSN_TRY(fsn_launch_gemm_tn(dg0 + (size_t)N * G, G, hseq0, H, dw_hh0, H, G, H, (long)(T - 1) * N, scratch, s));
        } else if (hipMemsetAsync(dw_hh1, 0, (size_t)G * H * sizeof(float), s) != hipSuccess ||
                   hipMemsetAsync(dw_hh0, 0, (size_t)G * H * sizeof(float), s) != hipSuccess) {
            fsn_set_error("memset failed");
            return FSN_ERR_LAUNCH;
        }
        return FSN_OK;
    }
    if (!clusters) {  // layer by layer; layer 1's dx is d loss / d hseq0
        if (!chain_part) return FSN_OK;  // (this form ran whole in phase 1)
        Carver cv(workspace);
        float* dh0 = cv.take<float>((size_t)T * N * H);
        const size_t l1 = fsn_lstm_layer_bwd_workspace_bytes(T, N, H, H), l0 = fsn_lstm_layer_bwd_workspace_bytes(T, N, I, H);
        void* ws = cv.take<char>(l1 > l0 ? l1 : l0);
        FSN_TRY(fsn_lstm_layer_backward(dh1, hseq0, H, w_ih1, w_hh1, T, N, H, H, hseq1, save1, dh0, H, dw_ih1, dw_hh1, db1, ws,
                                        l1 > l0 ? l1 : l0, stream));
        return fsn_lstm_layer_backward(dh0, x, ldx, w_ih0, w_hh0, T, N, I, H, hseq0, save0, dx, lddx, dw_ih0, dw_hh0, db0, ws,
                                       l1 > l0 ? l1 : l0, stream);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ipad = fsn_round_up(I, 16), G = 4 * H;
    const int left_tiles = N / 16 - 4 * clusters, left = left_tiles * 16, row0 = 64 * clusters;
    Carver cv(workspace);
    float* whh1T_p = cv.take<float>((size_t)3 * H * G + (size_t)Ipad * G);
    float* wih1T_p = whh1T_p + (size_t)H * G;
    float* whh0T_p = wih1T_p + (size_t)H * G;
    float* wih0T_p = whh0T_p + (size_t)H * G;
    float* dg1 = cv.take<float>((size_t)2 * T * N * G);
    float* dg0 = dg1 + (size_t)T * N * G;
    float* dxbuf = cv.take<float>((size_t)T * N * H);
    unsigned* flags = cv.take<unsigned>(lstm2_group_flag_words_any(clusters));
    float* dg1_left = cv.take<float>((size_t)T * left * G);
    float* dh0_left = cv.take<float>((size_t)T * left * H);
    float* dc_left = cv.take<float>((size_t)left * H);
    size_t tn = fsn_gemm_tn_workspace_bytes(G, I, (long)T * N);
    const size_t tn2 = fsn_gemm_tn_workspace_bytes(G, H, (long)T * N);
    void* scratch = cv.take<char>(tn > tn2 ? tn : tn2);
    unsigned short* w16 = arith != FSN_ARITH_F32 ? cv.take<unsigned short>((size_t)3 * H * G) : nullptr;
    void* g16_w = arith != FSN_ARITH_F32 ? cv.take<char>(fsn_lstm2_g16_bwd_weight_bytes()) : nullptr;
    float* partials = arith != FSN_ARITH_F32 ? cv.take<float>(fsn_lstm2_g16_partial_floats(clusters)) : nullptr;
    unsigned short* dg16 = arith != FSN_ARITH_F32 ? cv.take<unsigned short>((size_t)2 * T * N * G) : nullptr;  // layer 0 | layer 1
    unsigned short* h16 = arith != FSN_ARITH_F32 ? cv.take<unsigned short>((size_t)2 * T * N * H) : nullptr;    // hseq0 | hseq1
    float* dbp = arith != FSN_ARITH_F32 ? cv.take<float>((size_t)2 * clusters * G) : nullptr;
    const Lstm2Plan16 p16 = lstm2_plan16(T, N, I, ldx, H, arith | saves16);
    const bool g16 = p16.g16_bptt, tn16h = p16.tn16h, in16 = p16.in16;
    unsigned short* x16 = arith != FSN_ARITH_F32 ? cv.take<unsigned short>((size_t)T * N * 32 + (size_t)G * 32) : nullptr;  // x in 16 bits | W_ih0 fragments
    unsigned short* wdx16 = in16 ? x16 + (size_t)T * N * 32 : nullptr;
    const float* sv0 = static_cast<const float*>(save0);
    const float* sv1 = static_cast<const float*>(save1);
    const bool h16_saved = p16.h16_saved;  // the 16-bit h_t inside the save buffers: second half of a row's gate slot
    const unsigned short* h16_0 = h16_saved ? reinterpret_cast<const unsigned short*>(sv0) + G : h16;
    const unsigned short* h16_1 = h16_saved ? reinterpret_cast<const unsigned short*>(sv1) + G : (h16 ? h16 + (size_t)T * N * H : nullptr);
    const long ldh16 = h16_saved ? 2L * G : H;  // 16-bit elements between rows
    if (prepare_part) {
        if (tn16h && !h16_saved) {
            FSN_TRY(fsn_launch_to16(hseq0, h16, (size_t)T * N * H, arith, s));
            FSN_TRY(fsn_launch_to16(hseq1, h16 + (size_t)T * N * H, (size_t)T * N * H, arith, s));
        }
        if (!chain_part && !products_part && !dx_part) return FSN_OK;
    }
    if (chain_part) {
    // "weights" of dh = dgates W are W^T: out = H columns, k = 4H; nn.LSTM stores exactly that transposed.  (Not needed when the
    // 16-bit kernels take every row and every product: they pack the raw weights their own way.)
    if (!(g16 && left == 0 && in16)) {
        FSN_TRY(fsn_launch_pack(w_hh1, whh1T_p, H, G, H, G, s, 1, H));
        FSN_TRY(fsn_launch_pack(w_ih1, wih1T_p, H, G, H, G, s, 1, H));
        FSN_TRY(fsn_launch_pack(w_hh0, whh0T_p, H, G, H, G, s, 1, H));
        FSN_TRY(fsn_launch_pack(w_ih0, wih0T_p, I, G, Ipad, G, s, 1, I));
    }
    if (w16 && !g16) FSN_TRY(fsn_launch_to16(whh1T_p, w16, (size_t)3 * H * G, arith, s));  // the BPTT kernel's W^T fragments in 16 bits
    hipStream_t as = s;
    if (left > 0) FSN_TRY(aux_fork(s, &as));
    {
        FSN_PERSIST_BEGIN(s);
        if (g16) {  // the 16-bit arithmetic's own kernel (K-split; packs the raw weights its way into w16)
            // (layer 1's fp32 gate gradients of the cluster rows are not stored: the products below take the 16-bit copies)
            FSN_TRY(fsn_launch_lstm2_g16_bptt(dh1, w_hh1, w_ih1, w_hh0, sv0, sv1, dg0, dg1, partials, flags, g16_w, T, N, clusters,
                                              H, s, arith | (p16.saves16 ? FSN_ARITH_SAVES16 : 0), dg16, dg16 + (size_t)T * N * G, dbp,
                                              tn16h ? 0 : 1,
                                              in16 ? 0 : 1));  // dg16 = layer 0 | layer 1
            FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_g16_status_word(clusters), dg1, (size_t)2 * T * N * G, s));
            // the 16-bit copies and the bias-gradient sums as well (viewed as floats: every second value of a poisoned copy
            // is NaN - enough for every product to carry NaN into the gradient norm, on which the optimizer skips)
            FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_g16_status_word(clusters), reinterpret_cast<float*>(dg16),
                                         (size_t)T * N * G, s));
            FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_g16_status_word(clusters), dbp, (size_t)2 * clusters * G, s));
        } else {
            FSN_TRY(fsn_launch_lstm2_group_bptt(dh1, whh1T_p, wih1T_p, whh0T_p, sv0, sv1, dg0, dg1, dxbuf, flags, T, N, clusters,
                                                H, s, arith, w16));
            // both gate-gradient buffers (dg1 | dg0 are adjacent): every weight gradient and dx derive from them
            FSN_TRY(fsn_launch_poison_if(flags + fsn_lstm2_group_bptt_status_word(clusters), dg1, (size_t)2 * T * N * G, s));
        }
    }
    if (left > 0) {
        // the rows that do not fill a cluster: step by step on the auxiliary stream, straight into the same buffers
        const size_t stepH = (size_t)N * H, stepG = (size_t)N * G;
        for (int layer = 1; layer >= 0; --layer) {
            const float* sv = layer ? sv1 : sv0;
            const float* gates = sv + (size_t)row0 * G;
            const float* cseq = sv + (size_t)T * N * G + (size_t)row0 * H;
            float* dg = (layer ? dg1 : dg0) + (size_t)row0 * G;
            const float* whhT = layer ? whh1T_p : whh0T_p;
            for (int t = T - 1; t >= 0; --t) {
                const float* dh_t = layer ? dh1 + t * stepH + (size_t)row0 * H : dh0_left + (size_t)t * left * H;
                FSN_TRY(fsn_launch_bptt_step(dh_t, t + 1 < T ? dg + (t + 1) * stepG : dg, whhT, dc_left, gates + t * stepG,
                                             cseq + t * stepH, t ? cseq + (t - 1) * stepH : cseq, dg + t * stepG, left_tiles, H,
                                             t == T - 1, t == 0, as));
            }
            if (layer) {  // dh0 of these rows = dgates1 W_ih1: compact copy of their dgates1, one small GEMM
                FSN_TRY(gather_step_rows(dg1_left, dg1, G, T, N, row0, left, G, as));
                FSN_TRY(fsn_launch_gemm(gemm_a_rows(dg1_left, G), wih1T_p, gemm_c_rows(dh0_left, H, T * left, H), T * left_tiles,
                                        H / 16, G / 16, as));
            }
        }
        FSN_TRY(aux_join(s));
    }
    }  // chain_part
    if (dx && dx_part && in16) {
        // (the step-by-step rows' 16-bit copies first: the finish step of the products part may not have run yet)
        FSN_TRY(fsn_launch_g16_left_to16(dg0, dg16, T, N, row0, left, s, arith));
        FSN_TRY(fsn_launch_gemm_dx16(dg16, G, w_ih0, wdx16, dx, lddx, (long)T * N, G, I, s, arith));
    } else if (dx && dx_part) {
        FSN_TRY(fsn_launch_gemm(gemm_a_rows(dg0, G), wih0T_p, gemm_c_rows(dx, lddx, T * N, I), T * (N / 16), Ipad / 16, G / 16, s));
    }
    if (!products_part) return FSN_OK;
    // dW_ih = dgates^T X (+ db = its column sums: fp32 adds in every arithmetic), dW_hh = dgates_{1..}^T H_{0..T-2}
    // bias gradients = the BPTT launch's cluster sums + the step-by-step rows; those rows' 16-bit gate gradients (operands of
    // the products below: first when there are such rows; otherwise LAST - six tiny workgroups at the head of this part
    // queued behind whatever the caller's other stream was running and held the products back by its length)
    const bool finish_first = left > 0;
    if (g16 && finish_first)
        FSN_TRY(fsn_launch_lstm2_g16_finish(dg1, dg0, dg16 + (size_t)T * N * G, dg16, dbp, clusters, T, N, left, db1, db0, s, arith));
    if (tn16h) {
        // the three large products with both operands 16-bit in memory: dg16 = dg0 | dg1 written by the BPTT kernel, the
        // hidden sequences converted once (half the HBM bytes of the fp32 operands, LDS-DMA staging, no conversion pass)
        const size_t TNG = (size_t)T * N * G, TNH = (size_t)T * N * H;
        const unsigned short *dg16_0 = dg16, *dg16_1 = dg16 + TNG;
        if (!prepared && !prepare_part && !h16_saved) {
            FSN_TRY(fsn_launch_to16(hseq0, h16, TNH, arith, s));
            FSN_TRY(fsn_launch_to16(hseq1, h16 + TNH, TNH, arith, s));
        }
        (void)TNH;
        FSN_TRY(fsn_launch_gemm_tn16h(dg16_1, G, h16_0, ldh16, dw_ih1, H, G, H, (long)T * N, scratch, s, arith));
        FSN_TRY(fsn_launch_gemm_tn16h(dg16_1 + (size_t)N * G, G, h16_1, ldh16, dw_hh1, H, G, H, (long)(T - 1) * N, scratch, s, arith));
        FSN_TRY(fsn_launch_gemm_tn16h(dg16_0 + (size_t)N * G, G, h16_0, ldh16, dw_hh0, H, G, H, (long)(T - 1) * N, scratch, s, arith));
        if (in16) {  // x rounded once ([T N][32], its padding columns are zero), then the narrow product from 16-bit operands
            FSN_TRY(fsn_launch_to16(x, x16, (size_t)T * N * 32, arith, s));
            FSN_TRY(fsn_launch_gemm_tn16n(dg16_0, G, x16, 32, dw_ih0, I, G, I, (long)T * N, scratch, s, arith));
        } else {
            FSN_TRY(fsn_launch_gemm_tn(dg0, G, x, ldx, dw_ih0, I, G, I, (long)T * N, scratch, s, nullptr, arith));
        }
        if (!finish_first)
            FSN_TRY(fsn_launch_lstm2_g16_finish(dg1, dg0, dg16 + (size_t)T * N * G, dg16, dbp, clusters, T, N, left, db1, db0, s, arith));
        return FSN_OK;
    }
    if (g16) {  // (no plan for the 16-bit-operand products at this shape: the fp32 buffers; layer 1's were stored in that case)
        FSN_TRY(fsn_launch_gemm_tn(dg1, G, hseq0, H, dw_ih1, H, G, H, (long)T * N, scratch, s, nullptr, arith));
        FSN_TRY(fsn_launch_gemm_tn(dg0, G, x, ldx, dw_ih0, I, G, I, (long)T * N, scratch, s, nullptr, arith));
    } else {
        FSN_TRY(fsn_launch_gemm_tn(dg1, G, hseq0, H, dw_ih1, H, G, H, (long)T * N, scratch, s, db1, arith));
        FSN_TRY(fsn_launch_gemm_tn(dg0, G, x, ldx, dw_ih0, I, G, I, (long)T * N, scratch, s, db0, arith));
    }
    if (T > 1) {
        FSN_TRY(fsn_launch_gemm_tn(dg1 + (size_t)N * G, G, hseq1, H, dw_hh1, H, G, H, (long)(T - 1) * N, scratch, s, nullptr,
                                   arith));
        FSN_TRY(fsn_launch_gemm_tn(dg0 + (size_t)N * G, G, hseq0, H, dw_hh0, H, G, H, (long)(T - 1) * N, scratch, s, nullptr,
                                   arith));
    } else if (hipMemsetAsync(dw_hh1, 0, (size_t)G * H * sizeof(float), s) != hipSuccess ||
               hipMemsetAsync(dw_hh0, 0, (size_t)G * H * sizeof(float), s) != hipSuccess) {
        fsn_set_error("memset failed");
        return FSN_ERR_LAUNCH;
    }
    if (g16 && !finish_first)
        FSN_TRY(fsn_launch_lstm2_g16_finish(dg1, dg0, dg16 + (size_t)T * N * G, dg16, dbp, clusters, T, N, left, db1, db0, s, arith));
    return FSN_OK;
}

extern "C" int fsn_lstm2_backward(const float* dh1, const float* x, long ldx, const float* w_ih0, const float* w_hh0,
                                  const float* w_ih1, const float* w_hh1, int T, int N, int I, int H, const float* hseq0,
                                  const float* hseq1, const void* save0, const void* save1, float* dx, long lddx,
                                  float* dw_ih0, float* dw_hh0, float* db0, float* dw_ih1, float* dw_hh1, float* db1,
                                  void* workspace, size_t workspace_bytes, int arith, void* stream) {
    return lstm2_backward_phases(dh1, x, ldx, w_ih0, w_hh0, w_ih1, w_hh1, T, N, I, H, hseq0, hseq1, save0, save1, dx, lddx, dw_ih0,
                                 dw_hh0, db0, dw_ih1, dw_hh1, db1, workspace, workspace_bytes, arith, stream, 7);
}
extern "C" int fsn_lstm2_backward_phase(const float* dh1, const float* x, long ldx, const float* w_ih0, const float* w_hh0,
                                        const float* w_ih1, const float* w_hh1, int T, int N, int I, int H, const float* hseq0,
                                        const float* hseq1, const void* save0, const void* save1, float* dx, long lddx,
                                        float* dw_ih0, float* dw_hh0, float* db0, float* dw_ih1, float* dw_hh1, float* db1,
                                        void* workspace, size_t workspace_bytes, int arith, int phase, void* stream) {
    FSN_REQUIRE(phase >= 1 && phase <= 31 && (!(phase & 16) || (phase & 2)),
                "lstm2 backward parts %d: a sum of 1 (through time), 2 (weight-gradient products), 4 (dx), 8 (operand preparation), "
                "16 (with 2: prepared by an earlier part-8 call)", phase);
    return lstm2_backward_phases(dh1, x, ldx, w_ih0, w_hh0, w_ih1, w_hh1, T, N, I, H, hseq0, hseq1, save0, save1, dx, lddx, dw_ih0,
                                 dw_hh0, db0, dw_ih1, dw_hh1, db1, workspace, workspace_bytes, arith, stream, phase);
}

// ---- training step: nn.Linear (sequence_model.py:82-84) forward / backward ------------------------
// x [R][ldx] (columns I..ldx-1 zero, ldx = round_up(I,16)), w [O][I], b [O] -> y [R][O] (+ ReLU).
extern "C" size_t fsn_linear_workspace_bytes(int R, int I, int O) {
    const int Ip = fsn_round_up(I, 16), Op = fsn_round_up(O, 16);
    Carver cv(nullptr);
    cv.take<float>((size_t)Op * Ip);  // W (forward) or W^T (backward) fragments
    cv.take<float>((size_t)Op);       // padded bias
    size_t tn = fsn_gemm_tn_workspace_bytes(O, I, R);
    const size_t cs = fsn_colsum_workspace_bytes(O, R);
    cv.take<char>(tn > cs ? tn : cs);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_linear_forward(const float* x, long ldx, const float* w, const float* b, int R, int I, int O,
                                  int relu, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(x && w && b && y && workspace, "NULL pointer argument");
    FSN_REQUIRE(R >= 1 && I >= 1 && O >= 1 && ldx >= fsn_round_up(I, 16) && ldx % 4 == 0, "linear: bad shape");
    if (workspace_bytes < fsn_linear_workspace_bytes(R, I, O)) {
        fsn_set_error("linear: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (fsn_linear_small_out_ok(I, O, ldx))  // a handful of outputs: bandwidth-bound row dot products, no padded GEMM
        return fsn_launch_linear_small_out(x, ldx, w, b, y, R, I, O, relu, s);
    const int Ip = fsn_round_up(I, 16), Op = fsn_round_up(O, 16);
    Carver cv(workspace);
    float* wp = cv.take<float>((size_t)Op * Ip);
    float* bp = cv.take<float>((size_t)Op);
    FSN_TRY(fsn_launch_pack(w, wp, O, I, Op, Ip, s));
    FSN_TRY(fsn_launch_bias_sum(b, nullptr, bp, O, Op, s));
    return fsn_launch_gemm(gemm_a_rows(x, ldx, R), wp, gemm_c_rows(y, O, R, O, bp, relu != 0), (R + 15) / 16, Op / 16, Ip / 16, s);
}

// dy [R][lddy] (columns O..lddy-1 zero, lddy = round_up(O,16)) -> dx [R][lddx] (may be NULL), dw [O][I], db [O]
extern "C" int fsn_linear_backward(const float* dy, long lddy, const float* x, long ldx, const float* w, int R, int I,
                                   int O, float* dx, long lddx, float* dw, float* db, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(dy && x && w && workspace && (dx || dw) && (dw == nullptr) == (db == nullptr),
                "linear backward: NULL pointer argument (dx alone, dw + db alone, or all three)");
    FSN_REQUIRE(R >= 1 && I >= 1 && O >= 1 && lddy >= fsn_round_up(O, 16) && lddy % 4 == 0 && ldx >= I,
                "linear backward: bad shape");
    if (workspace_bytes < fsn_linear_workspace_bytes(R, I, O)) {
        fsn_set_error("linear: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int Ip = fsn_round_up(I, 16), Op = fsn_round_up(O, 16);
    Carver cv(workspace);
    float* wtp = cv.take<float>((size_t)Op * Ip);
    cv.take<float>((size_t)Op);
    size_t tn = fsn_gemm_tn_workspace_bytes(O, I, R);
    const size_t cs = fsn_colsum_workspace_bytes(O, R);
    void* scratch = cv.take<char>(tn > cs ? tn : cs);
    if (dx && fsn_linear_small_out_ok(I, O, lddx)) {
        FSN_TRY(fsn_launch_linear_small_dx(dy, lddy, w, dx, lddx, R, I, O, s));
    } else if (dx) {
        // dX = dY W: "weights" W^T (out = I, k = O) = the stored [O][I] read transposed
        FSN_TRY(fsn_launch_pack(w, wtp, I, O, Ip, Op, s, 1, I));
        FSN_TRY(fsn_launch_gemm(gemm_a_rows(dy, lddy, R), wtp, gemm_c_rows(dx, lddx, R, I), (R + 15) / 16, Ip / 16, Op / 16, s));
    }
    if (!dw) return FSN_OK;  // the input gradient alone (the parameter gradients by a second call, possibly on another stream)
    FSN_TRY(fsn_launch_gemm_tn(dy, lddy, x, ldx, dw, I, O, I, R, scratch, s));
    return fsn_launch_colsum(dy, lddy, db, O, R, scratch, s);
}

// ---- test hooks: the 16-bit arithmetic's conversion and product launchers on caller data ---------------------------
// Thin entries: shape, pointer and workspace-size checks here, then the launcher unchanged (its own checks stay in force).
// The workspace of the three weight-gradient forms is that of the fp32 product, fsn_debug_gemm_tn_workspace_bytes.
extern "C" size_t fsn_debug_gemm_tn_workspace_bytes(int M, int Nc, long K) {
    if (M < 1 || Nc < 1 || K < 1) return 0;
    return fsn_gemm_tn_workspace_bytes(M, Nc, K);
}
extern "C" int fsn_debug_tn16_plan(int narrow, int M, int Nc, long K, int* splits, int* form) {
    if (M < 1 || Nc < 1 || K < 1) return -1;
    int s = 0;
    const int f = narrow ? ((s = fsn_gemm_tn16n_splits(M, Nc, K)) > 0 ? 1 : 0) : fsn_gemm_tn16h_form(M, Nc, K, &s);
    if (splits) *splits = s;
    if (form) *form = f;
    return 0;
}
extern "C" int fsn_debug_to16(const float* src, void* dst, size_t n, int arith, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(src && dst && n > 0, "to16: NULL pointer argument or no elements");
    FSN_REQUIRE(((size_t)src & 15) == 0 && ((size_t)dst & 7) == 0, "to16: source rows of 16 bytes, destination of 8");
    return fsn_launch_to16(src, dst, n, arith, static_cast<hipStream_t>(stream));
}
static int debug_tn_args(const void* A, long lda, const void* B, long ldb, const float* C, long ldc, int M, int Nc, long K,
                         const void* workspace, size_t workspace_bytes) {
    FSN_REQUIRE(A && B && C && workspace, "NULL pointer argument");
    FSN_REQUIRE(M >= 1 && Nc >= 1 && K >= 1 && lda >= M && ldb >= Nc && ldc >= Nc, "gemm_tn: bad shape");
    if (workspace_bytes < fsn_gemm_tn_workspace_bytes(M, Nc, K)) {
        fsn_set_error("gemm_tn: workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}
extern "C" int fsn_debug_gemm_tn16h(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                                    void* workspace, size_t workspace_bytes, int arith, void* stream) {
    CallScope scope(stream);
    FSN_TRY(debug_tn_args(A16, lda, B16, ldb, C, ldc, M, Nc, K, workspace, workspace_bytes));
    return fsn_launch_gemm_tn16h(A16, lda, B16, ldb, C, ldc, M, Nc, K, workspace, static_cast<hipStream_t>(stream), arith);
}
extern "C" int fsn_debug_gemm_tn16n(const void* A16, long lda, const void* B16, long ldb, float* C, long ldc, int M, int Nc, long K,
                                    void* workspace, size_t workspace_bytes, int arith, void* stream) {
    CallScope scope(stream);
    FSN_TRY(debug_tn_args(A16, lda, B16, ldb, C, ldc, M, Nc, K, workspace, workspace_bytes));
    return fsn_launch_gemm_tn16n(A16, lda, B16, ldb, C, ldc, M, Nc, K, workspace, static_cast<hipStream_t>(stream), arith);
}
extern "C" int fsn_debug_gemm_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int Nc, long K,
                                 void* workspace, size_t workspace_bytes, int arith, void* stream) {
    CallScope scope(stream);
    FSN_TRY(debug_tn_args(A, lda, B, ldb, C, ldc, M, Nc, K, workspace, workspace_bytes));
    return fsn_launch_gemm_tn(A, lda, B, ldb, C, ldc, M, Nc, K, workspace, static_cast<hipStream_t>(stream), nullptr, arith);
}
// wfrag: G x 32 16-bit words (written here: the packed weight)
extern "C" int fsn_debug_gemm_dx16(const void* dg16, long ld16, const float* w, void* wfrag, size_t wfrag_bytes, float* dx, long lddx,
                                   long rows, int G, int I, int arith, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(dg16 && w && wfrag && dx, "NULL pointer argument");
    FSN_REQUIRE(rows >= 1 && G >= 1 && I >= 1 && ld16 >= G && lddx >= I, "gemm_dx16: bad shape");
    if (wfrag_bytes < (size_t)G * 32 * sizeof(unsigned short)) {
        fsn_set_error("gemm_dx16: weight-fragment scratch too small");
        return FSN_ERR_WORKSPACE;
    }
    return fsn_launch_gemm_dx16(dg16, ld16, w, wfrag, dx, lddx, rows, G, I, static_cast<hipStream_t>(stream), arith);
}
