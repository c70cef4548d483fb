// C ABI of libfsn_hip.so, the FullSubNet model (fullsubnet/model.py): weight packing, the model core and its batch
// chunking, the full-band / row-range / streaming forms, the STFT / iSTFT and elementwise boundary and the whole
// enhancement path (fsn_enhance, fsn_enhance_ragged).
#include <algorithm>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "fsn_api_internal.h"

static int check_cfg(const fsn_fullsubnet_cfg* cfg) {
    FSN_REQUIRE(cfg != nullptr, "cfg is NULL");
    FSN_REQUIRE(cfg->num_freqs >= 17 && cfg->num_freqs <= 4096, "num_freqs %d out of range", cfg->num_freqs);
    FSN_REQUIRE(cfg->look_ahead >= 0, "look_ahead %d < 0", cfg->look_ahead);
    FSN_REQUIRE(cfg->sb_num_neighbors >= 0 && cfg->sb_num_neighbors < cfg->num_freqs,
                "sb_num_neighbors %d must be in [0, num_freqs) (reflect padding)", cfg->sb_num_neighbors);
    FSN_REQUIRE(cfg->fb_hidden > 0 && cfg->fb_hidden % 64 == 0, "fb_hidden %d must be a multiple of 64",
                cfg->fb_hidden);
    FSN_REQUIRE(cfg->sb_hidden == 384, "sb_hidden %d unsupported (the sub-band recurrent kernel is built for 384)",
                cfg->sb_hidden);
    FSN_REQUIRE(cfg->norm_type == FSN_NORM_OFFLINE_LAPLACE || cfg->norm_type == FSN_NORM_CUMULATIVE_LAPLACE,
                "norm_type %d unsupported", cfg->norm_type);
    FSN_REQUIRE(cfg->arith == FSN_ARITH_F32 || cfg->arith == FSN_ARITH_F16X3, "arith %d unsupported", cfg->arith);
    return FSN_OK;
}

// ---- packed weights --------------------------------------------------------------------------
struct Packed {  // float offsets into the packed blob
    size_t fb_wih0, fb_whh0, fb_b0, fb_wih1, fb_whh1, fb_b1, fb_fc, fb_fcb;
    size_t sb_wih0, sb_whh0, sb_b0, sb_wih1, sb_whh1, sb_b1, sb_fc, sb_fcb;
    size_t fb_b1_frag, sb_b1_frag;  // layer-1 biases as accumulator-fragment tiles (wavefront step kernel)
    size_t sb_wih1_f16x3;           // experimental: sub-band W_ih of layer 1 split into fp16 halves (FSN_F16X3=1)
    size_t sb_whh1_f16x3;           // experimental: likewise W_hh of layer 1
    size_t sb_wih0_f16x3;           // experimental: W_ih of layer 0 (only when its padded width is 32), scale 4096
    size_t sb_whh0_f16x3;           // experimental: W_hh of layer 0
    size_t total;
    int FP, sb_kin_pad;
};
static Packed packed_layout(const fsn_fullsubnet_cfg* c) {
    Packed p;
    size_t o = 0;
    auto take = [&](size_t n) {
        o = fsn_round_up_sz(o, 64);
        const size_t r = o;
        o += n;
        return r;
    };
    const size_t Hf = c->fb_hidden, Hs = c->sb_hidden;
    p.FP = fsn_fpad(c->num_freqs);
    p.sb_kin_pad = fsn_round_up(2 * c->sb_num_neighbors + 2, 16);
    p.fb_wih0 = take(4 * Hf * p.FP);
    p.fb_whh0 = take(4 * Hf * Hf);
    p.fb_b0 = take(4 * Hf);
    p.fb_wih1 = take(4 * Hf * Hf);
    p.fb_whh1 = take(4 * Hf * Hf);
    p.fb_b1 = take(4 * Hf);
    p.fb_fc = take((size_t)p.FP * Hf);
    p.fb_fcb = take(p.FP);
    p.sb_wih0 = take(4 * Hs * p.sb_kin_pad);
    p.sb_whh0 = take(4 * Hs * Hs);
    p.sb_b0 = take(4 * Hs);
    p.sb_wih1 = take(4 * Hs * Hs);
    p.sb_whh1 = take(4 * Hs * Hs);
    p.sb_b1 = take(4 * Hs);
    p.sb_fc = take(16 * Hs);
    p.sb_fcb = take(16);
    p.fb_b1_frag = take(4 * Hf * 16);  // [4H/16 column tiles][64 lanes][4]
    p.sb_b1_frag = take(4 * Hs * 16);
    p.sb_wih1_f16x3 = take((fsn_f16x3_packed_halves(4 * (int)Hs, (int)Hs) + 1) / 2);  // halves -> floats
    p.sb_whh1_f16x3 = take((fsn_f16x3_packed_halves(4 * (int)Hs, (int)Hs) + 1) / 2);
    p.sb_wih0_f16x3 = take((fsn_f16x3_packed_halves(4 * (int)Hs, 32) + 1) / 2);
    p.sb_whh0_f16x3 = take((fsn_f16x3_packed_halves(4 * (int)Hs, (int)Hs) + 1) / 2);
    p.total = fsn_round_up_sz(o, 64);
    return p;
}

extern "C" size_t fsn_fullsubnet_packed_bytes(const fsn_fullsubnet_cfg* cfg) {
    if (check_cfg(cfg) != FSN_OK) return 0;
    return packed_layout(cfg).total * sizeof(float);
}

extern "C" int fsn_fullsubnet_pack(const fsn_fullsubnet_cfg* cfg, const fsn_fullsubnet_params* w, void* packed,
                                   size_t packed_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_cfg(cfg));
    FSN_REQUIRE(w && packed, "params / packed is NULL");
    const float* const* all = reinterpret_cast<const float* const*>(w);
    for (size_t i = 0; i < sizeof(*w) / sizeof(float*); ++i) FSN_REQUIRE(all[i], "params tensor %zu is NULL", i);
    const Packed p = packed_layout(cfg);
    FSN_REQUIRE(packed_bytes >= p.total * sizeof(float), "packed buffer too small: %zu < %zu", packed_bytes,
                p.total * sizeof(float));
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* o = static_cast<float*>(packed);
    const int F = cfg->num_freqs, Hf = cfg->fb_hidden, Hs = cfg->sb_hidden;
    const int kin = 2 * cfg->sb_num_neighbors + 2;
    FSN_TRY(fsn_launch_pack(w->fb_w_ih_l0, o + p.fb_wih0, 4 * Hf, F, 4 * Hf, p.FP, s));
    FSN_TRY(fsn_launch_pack(w->fb_w_hh_l0, o + p.fb_whh0, 4 * Hf, Hf, 4 * Hf, Hf, s));
    FSN_TRY(fsn_launch_bias_sum(w->fb_b_ih_l0, w->fb_b_hh_l0, o + p.fb_b0, 4 * Hf, 4 * Hf, s));
    FSN_TRY(fsn_launch_pack(w->fb_w_ih_l1, o + p.fb_wih1, 4 * Hf, Hf, 4 * Hf, Hf, s));
    FSN_TRY(fsn_launch_pack(w->fb_w_hh_l1, o + p.fb_whh1, 4 * Hf, Hf, 4 * Hf, Hf, s));
    FSN_TRY(fsn_launch_bias_sum(w->fb_b_ih_l1, w->fb_b_hh_l1, o + p.fb_b1, 4 * Hf, 4 * Hf, s));
    FSN_TRY(fsn_launch_pack(w->fb_fc_w, o + p.fb_fc, F, Hf, p.FP, Hf, s));
    FSN_TRY(fsn_launch_bias_sum(w->fb_fc_b, nullptr, o + p.fb_fcb, F, p.FP, s));
    FSN_TRY(fsn_launch_pack(w->sb_w_ih_l0, o + p.sb_wih0, 4 * Hs, kin, 4 * Hs, p.sb_kin_pad, s));
    FSN_TRY(fsn_launch_pack(w->sb_w_hh_l0, o + p.sb_whh0, 4 * Hs, Hs, 4 * Hs, Hs, s));
    FSN_TRY(fsn_launch_bias_sum(w->sb_b_ih_l0, w->sb_b_hh_l0, o + p.sb_b0, 4 * Hs, 4 * Hs, s));
    FSN_TRY(fsn_launch_pack(w->sb_w_ih_l1, o + p.sb_wih1, 4 * Hs, Hs, 4 * Hs, Hs, s));
    FSN_TRY(fsn_launch_pack(w->sb_w_hh_l1, o + p.sb_whh1, 4 * Hs, Hs, 4 * Hs, Hs, s));
    FSN_TRY(fsn_launch_bias_sum(w->sb_b_ih_l1, w->sb_b_hh_l1, o + p.sb_b1, 4 * Hs, 4 * Hs, s));
    FSN_TRY(fsn_launch_pack(w->sb_fc_w, o + p.sb_fc, 2, Hs, 16, Hs, s));
    FSN_TRY(fsn_launch_bias_sum(w->sb_fc_b, nullptr, o + p.sb_fcb, 2, 16, s));
    FSN_TRY(fsn_launch_bias_frag(o + p.fb_b1, o + p.fb_b1_frag, 4 * Hf, s));
    FSN_TRY(fsn_launch_bias_frag(o + p.sb_b1, o + p.sb_b1_frag, 4 * Hs, s));
    if (Hs % 32 == 0) {
        FSN_TRY(fsn_launch_pack_f16x3(w->sb_w_ih_l1, o + p.sb_wih1_f16x3, 4 * Hs, Hs, s));
        FSN_TRY(fsn_launch_pack_f16x3(w->sb_w_hh_l1, o + p.sb_whh1_f16x3, 4 * Hs, Hs, s));
        FSN_TRY(fsn_launch_pack_f16x3(w->sb_w_hh_l0, o + p.sb_whh0_f16x3, 4 * Hs, Hs, s));
        if (kin == 32)
            FSN_TRY(fsn_launch_pack_f16x3(w->sb_w_ih_l0, o + p.sb_wih0_f16x3, 4 * Hs, 32, s, fsn_f16x3_wih0_scale()));
    }
    return FSN_OK;
}

constexpr int kGroupTwoFromTiles = 224;  // 56+ clusters: two per workgroup set
constexpr int kGroupMaxTiles = 264;      // 64 clusters + up to 8 left-over tiles

// ---- model core: magT [B][Tp][FP] -> crm_r, crm_i [B][T][FP] ------------------------------------
struct CoreDims {
    int B, T, Tp, F, FP, Hf, Hs, nb, la;
    int Npad_fb;       // full-band rows per step (batch, padded to 16)
    bool fb_chain;     // the full-band LSTM layers run as one persistent launch (fb_chain_kernels.hip)
    int N, Npad;       // sub-band rows per step, padded rows (row stride of the [t][n] buffers)
    FsnRecPlan rec;    // how those rows are spread over the CUs
    bool fc_fused;     // output layer fused into the layer-1 persistent kernel (its hseq is never stored)
    bool l1x;          // layer 1 forms its input projection itself (lstm_rec_x_kernel): no projection GEMM, no gx
    int grp_clusters;  // > 0: the step regime runs on the group kernel (lstm_group_kernels.hip), that many clusters of 64 rows
    long row0;         // row-range calls: the N sub-band rows are rows row0 .. row0 + N - 1 of the B F rows
    int den_stride;    // row stride of the per-row (cumulative) sub-band divisors: they are indexed by GLOBAL row
};
// n_rows < 0: all B F sub-band rows; otherwise the rows [row0, row0 + n_rows) of the flattened (b, f) index space
// (the full-band model and the norm statistics always cover the B whole utterances).
static CoreDims core_dims(const fsn_fullsubnet_cfg* c, int B, int T, long row0 = 0, long n_rows = -1) {
    CoreDims d;
    d.B = B;
    d.T = T;
    d.la = c->look_ahead;
    d.Tp = T + c->look_ahead;
    d.F = c->num_freqs;
    d.FP = fsn_fpad(d.F);
    d.Hf = c->fb_hidden;
    d.Hs = c->sb_hidden;
    d.nb = c->sb_num_neighbors;
    d.Npad_fb = fsn_round_up(B, 16);
    d.fb_chain = fsn_fb_chain_supported(d.Hf, d.Npad_fb) && d.Tp <= fsn_fb_chain_max_steps();
    d.N = n_rows < 0 ? B * d.F : (int)n_rows;
    d.row0 = n_rows < 0 ? 0 : row0;
    d.rec = fsn_lstm_rec_plan(d.N, d.Hs);
    // 224 - 264 row tiles (14 - 16 utterances: one rank's share of config 2 at 4 GPUs) run on the group kernel with two
    // clusters per workgroup set (lstm_group_kernels.hip) instead of the persistent kernels at ONE row tile per CU
    // (every CU streams all weights every step there): 26.5 -> 23.4 ms at 16 utterances
    const bool grp_shape = d.Hs == 384 && fsn_round_up(2 * c->sb_num_neighbors + 2, 16) == 32 && c->arith == FSN_ARITH_F32;
    if (grp_shape && d.rec.tiles >= kGroupTwoFromTiles && d.rec.tiles <= kGroupMaxTiles && d.rec.main_wgs > 0 &&
        4 * fsn_lstm2_group_clusters(d.rec.tiles) + 8 >= d.rec.tiles) {  // ... and the device holds (nearly) all of them
        d.rec.rt = 1;
        d.rec.main_wgs = 0;
        d.rec.left_tiles = d.rec.tiles;
    }
    d.Npad = d.rec.npad;
    d.den_stride = n_rows < 0 ? d.Npad : fsn_round_up(B * d.F, 16);
    d.fc_fused = d.rec.main_wgs > 0 && fsn_lstm_rec_can_fuse_fc(d.rec.rt, false);
    d.l1x = d.fc_fused && c->arith == FSN_ARITH_F32 && fsn_lstm_rec_x_supported(d.Hs, d.rec.rt);
    // 96 - 159 row tiles (6 - 9 utterances; below that the two-layer wavefront of per-step launches is as fast)
    d.grp_clusters = 0;
    if (d.rec.main_wgs == 0 && d.rec.left_tiles >= kWavefrontBelowTiles && grp_shape)  // fp32 only: the group kernel has no f16x3 form
        d.grp_clusters = fsn_lstm2_group_clusters(d.rec.left_tiles);
    return d;
}
struct CoreWs {
    float *gx_fb, *hseq_fb0, *hseq_fb1, *c_fb, *fb_out, *den_fb, *den_sb, *gx_sb, *hseq_sb0, *hseq_sb1, *c_left;
    float* hseq_left0;  // l1x: layer-0 hidden sequence of the left-over rows, compact [t][left rows][H]
    float* grp_exchange;  // group kernel: h exchange buffers of the clusters
    unsigned* grp_flags;
    float* fb_exchange;   // full-band chain kernel: per-step h / projection hand-off buffers
    unsigned* fb_flags;
    double* binsum;
};
static CoreWs core_carve(Carver& cv, const CoreDims& d, int norm_type) {
    CoreWs w;
    const size_t rows_fb = (size_t)d.Tp * d.Npad_fb, rows_sb = (size_t)d.Tp * d.Npad;
    w.gx_fb = cv.take<float>(rows_fb * 4 * d.Hf);
    w.hseq_fb0 = cv.take<float>(rows_fb * d.Hf);
    w.hseq_fb1 = cv.take<float>(rows_fb * d.Hf);
    w.c_fb = cv.take<float>((size_t)2 * d.Npad_fb * d.Hf);  // one cell state per layer (wavefront)
    w.fb_out = cv.take<float>((size_t)d.B * d.Tp * d.FP);
    w.binsum = cv.take<double>((size_t)d.B * d.FP);
    const bool cum = norm_type == FSN_NORM_CUMULATIVE_LAPLACE;
    w.den_fb = cv.take<float>(cum ? (size_t)d.B * d.Tp : (size_t)d.B);
    w.den_sb = cv.take<float>(cum ? (size_t)d.Tp * d.den_stride : (size_t)d.B);
    // l1x: only the left-over rows (which run step by step) still need a precomputed projection
    const size_t rows_left = (size_t)d.Tp * (d.rec.left_tiles > 0 ? d.rec.left_tiles : 1) * 16;
    if (d.grp_clusters > 0) {
        // group kernel: projections and hidden sequences only exist for the rows that do not fill a cluster
        const int aux_tiles = d.rec.tiles - 4 * d.grp_clusters;
        const size_t rows_aux = (size_t)d.Tp * (aux_tiles > 0 ? aux_tiles : 1) * 16;
        w.gx_sb = cv.take<float>(rows_aux * 4 * d.Hs);
        w.hseq_sb0 = cv.take<float>(rows_aux * d.Hs);
        w.hseq_left0 = nullptr;
        w.hseq_sb1 = cv.take<float>(rows_aux * d.Hs);
    } else {
        w.gx_sb = cv.take<float>((d.l1x ? rows_left : rows_sb) * 4 * d.Hs);
        w.hseq_sb0 = cv.take<float>(rows_sb * d.Hs);
        w.hseq_left0 = d.l1x ? cv.take<float>(rows_left * d.Hs) : nullptr;
        // fused output layer: only the left-over rows of layer 1 are ever stored, [t][left rows][H]
        w.hseq_sb1 = cv.take<float>(d.fc_fused ? (size_t)d.Tp * (d.rec.left_tiles > 0 ? d.rec.left_tiles : 1) * 16 * d.Hs
                                               : rows_sb * d.Hs);
    }
    w.c_left = cv.take<float>((size_t)2 * (d.rec.left_tiles > 0 ? d.rec.left_tiles : 1) * 16 * d.Hs);
    w.grp_exchange = d.grp_clusters ? cv.take<float>(fsn_lstm2_group_exchange_floats(d.grp_clusters)) : nullptr;
    w.grp_flags = d.grp_clusters ? cv.take<unsigned>(fsn_lstm2_group_flag_words(d.grp_clusters)) : nullptr;
    w.fb_exchange = d.fb_chain ? cv.take<float>(fsn_fb_chain_exchange_floats(d.Tp, d.Npad_fb)) : nullptr;
    w.fb_flags = d.fb_chain ? cv.take<unsigned>(fsn_fb_chain_flag_words()) : nullptr;
    return w;
}

// One sub-band LSTM layer over all Tp steps: the persistent kernel on `s` and, concurrently, the
// few left-over row tiles as per-step launches on the auxiliary stream (the fields of RecArgs, fsn_api_internal.h).
// How run_recurrence spreads the rows that run step by step (also what fsn_debug_core_call_plan reports).
// No persistent part (fewer than ~160 tiles): the steps run on the caller's stream itself - groups of four tiles through
// the one-workgroup-per-CU step kernel (cu_tiles), the up to three tiles that do not fill a group beside it on the
// auxiliary stream (a 33rd group of 8 workgroups would be a second round on 8 CUs and double the step).
struct StepSplit {
    int cu_tiles, aux_tiles;
};
static StepSplit step_split(const FsnRecPlan& r) {
    const int cu_tiles = r.main_wgs == 0 && r.left_tiles >= 8 ? r.left_tiles / 4 * 4 : 0;
    return StepSplit{cu_tiles, r.left_tiles - cu_tiles};
}
int run_recurrence(const RecArgs& a, hipStream_t s) {
    const FsnRecPlan& r = a.plan;
    const int Tp = a.Tp, Npad = a.Npad, H = a.H;
    const StepSplit split = step_split(r);
    const int cu_tiles = split.cu_tiles, aux_tiles = split.aux_tiles;
    const bool fork = aux_tiles > 0 && (r.main_wgs > 0 || cu_tiles > 0);
    hipStream_t ls = s;
    if (fork) FSN_TRY(aux_fork(s, &ls));
    if (r.main_wgs > 0) {
        if (a.x_main)
            FSN_TRY(fsn_launch_lstm_rec_x(a.x_main, a.wih_main, a.whh, a.bias_main, Tp, Npad, H, r.rt, r.main_wgs, s, a.fc,
                                          a.fc ? nullptr : a.hseq));  // no output layer: a layer inside a stack, h_t stored
        else if (a.xin && !a.fc && !a.whh_f16x3 && fsn_lstm_rec_in_supported(a.xin, a.whh, H, r.rt))
            FSN_TRY(fsn_launch_lstm_rec_in(a.xin, a.whh, a.hseq, Tp, Npad, H, r.rt, r.main_wgs, s));
        else if (a.whh_f16x3 && a.fc && !a.xin && r.rt >= 2)  // experimental split-precision persistent kernel (FSN_F16X3=1)
            FSN_TRY(fsn_launch_lstm_rec_f16x3(a.gx, a.whh_f16x3, Tp, Npad, H, r.rt, r.main_wgs, a.fc, s));
        else if (a.whh_f16x3 && a.wih_f16x3 && a.xin && !a.xin->x_rows && a.xin->kin_chunks == 2 && r.rt >= 2)
            FSN_TRY(fsn_launch_lstm_rec_xin_f16x3(a.xin, a.wih_f16x3, a.whh_f16x3, a.hseq, Tp, Npad, H, r.rt, r.main_wgs, s));
        else
            FSN_TRY(fsn_launch_lstm_rec(a.gx, a.xin, a.whh, a.hseq, Tp, Npad, H, r.rt, r.main_wgs, s, a.fc));
    }
    if (r.left_tiles > 0) {
        // left-over rows of step t: rows [main_rows, Npad) of the full [t][Npad] matrix, or - when the
        // persistent part stores nothing (fused output layer) - a compact [t][left rows] matrix
        const long left_hs_stride = a.hseq_left ? (long)r.left_tiles * 16 : a.left_hs_stride;
        float* hl = a.hseq_left ? a.hseq_left : a.hseq;
        const long hs_stride = left_hs_stride >= 0 ? left_hs_stride : Npad;
        const long hs_off = left_hs_stride >= 0 ? 0 : (long)r.main_wgs * r.rt * 16;
        for (int t = 0; t < Tp; ++t) {
            float* h_out = hl + ((size_t)t * hs_stride + hs_off) * H;
            const float* h_prev = t ? hl + ((size_t)(t - 1) * hs_stride + hs_off) * H : h_out;
            const long gx_rt0 = (long)t * a.left_stride + a.left_off;
            if (cu_tiles > 0)
                FSN_TRY(fsn_launch_lstm_step_cu(a.gx_left, a.whh, h_prev, h_out, a.c_left, gx_rt0, cu_tiles, H, t == 0, s));
            if (aux_tiles > 0) {
                const size_t ro = (size_t)cu_tiles * 16 * H;
                FSN_TRY(fsn_launch_lstm_step(a.gx_left, a.whh, h_prev + ro, h_out + ro, a.c_left + ro, gx_rt0 + cu_tiles,
                                             aux_tiles, H, t == 0, ls, fork ? 1 : 0));
            }
        }
    }
    if (fork) FSN_TRY(aux_join(s));
    return FSN_OK;
}

// ---- one core call, stage by stage ------------------------------------------------------------------------------------
// What every stage reads.  lengths (device, [d.B], may be NULL): a ragged batch (fsn_enhance_ragged) - only the offline
// norm's divisors depend on an utterance's length (magT is zero past its frames); the cumulative norm and the models are
// causal and run to d.Tp.
struct CoreCall {
    const fsn_fullsubnet_cfg* cfg;
    Packed p;
    const float* pk;
    const float* magT;
    const CoreDims& d;
    const CoreWs& w;
    ModelGeom g;
    bool cum;
    float *crm_r, *crm_i;
    const int* lengths;
    hipStream_t s;
};
static CoreCall core_call(const fsn_fullsubnet_cfg* cfg, const float* pk, const float* magT, const CoreDims& d, const CoreWs& w,
                          float* crm_r, float* crm_i, hipStream_t s, const int* lengths) {
    return CoreCall{cfg, packed_layout(cfg), pk, magT, d, w, ModelGeom{d.B, d.Tp, d.T, d.F, d.FP, d.nb, d.la},
                    cfg->norm_type == FSN_NORM_CUMULATIVE_LAPLACE, crm_r, crm_i, lengths, s};
}

// full-band norm divisor (fullsubnet/model.py:92) and model (model.py:95): 2 LSTM layers + Linear + ReLU -> w.fb_out
static int core_fullband(const CoreCall& k) {
    const CoreDims& d = k.d;
    const CoreWs& w = k.w;
    const Packed& p = k.p;
    const float* pk = k.pk;
    hipStream_t s = k.s;
    {
        StageTimer st(ST_NORM, s);
        if (k.cum) {
            FSN_TRY(fsn_launch_cumulative_den_fb(k.magT, w.den_fb, d.B, d.Tp, d.F, d.FP, s));
        } else {
            FSN_TRY(fsn_launch_binsum(k.magT, w.binsum, d.B, d.Tp, d.FP, s));
            FSN_TRY(fsn_launch_offline_den(w.binsum, nullptr, w.den_fb, nullptr, d.B, d.Tp, d.F, d.FP, d.nb, 0, s,
                                           k.lengths, d.T));
        }
    }
    const int fb_rt = d.Tp * d.Npad_fb / 16;
    {
        StageTimer st(ST_FB_GEMM, s);
        FSN_TRY(fsn_launch_gemm(gemm_a_fullband(k.g, k.magT, w.den_fb, k.cum ? 1 : 0, d.Npad_fb), pk + p.fb_wih0,
                                gemm_c_frag(w.gx_fb, pk + p.fb_b0), fb_rt, 4 * d.Hf / 16, d.FP / 16, s));
    }
    {
        // N = B rows only: a chain of tiny dependent launches, so the two layers advance as a wavefront
        // (layer 1 at step t next to layer 0 at step t + 1): T' + 1 launches instead of 2 T'
        StageTimer st(ST_FB_REC, s);
        if (d.fb_chain) {  // up to 64 utterances, H = 512: the whole chain as one persistent launch
            FSN_PERSIST_BEGIN(s);
            FSN_TRY(fsn_launch_fb_chain(w.gx_fb, pk + p.fb_whh0, pk + p.fb_wih1, pk + p.fb_whh1, pk + p.fb_b1,
                                        w.fb_exchange, w.fb_flags, w.hseq_fb1, d.Tp, d.Npad_fb, d.Hf, s));
            FSN_TRY(fsn_launch_poison_if(w.fb_flags + fsn_fb_chain_status_word(), w.hseq_fb1,
                                         (size_t)d.Tp * d.Npad_fb * d.Hf, s));
        } else {
            FSN_TRY(fsn_launch_lstm_wavefront2(w.gx_fb, d.Npad_fb / 16, 0, pk + p.fb_whh0, pk + p.fb_wih1,
                                               pk + p.fb_b1_frag, pk + p.fb_whh1, w.hseq_fb0, w.hseq_fb1, d.Npad_fb, 0,
                                               w.c_fb, w.c_fb + (size_t)d.Npad_fb * d.Hf, d.Tp, d.Npad_fb / 16, d.Hf, s));
        }
    }
    StageTimer st(ST_FB_GEMM, s);
    return fsn_launch_gemm(gemm_a_rows(w.hseq_fb1, d.Hf), pk + p.fb_fc, gemm_c_fb_out(k.g, w.fb_out, pk + p.fb_fcb, d.Npad_fb),
                           fb_rt, d.FP / 16, d.Hf / 16, s);
}

// sub-band norm divisor over the (virtual) concatenated sub-band input (model.py:110-111)
static int core_sb_divisor(const CoreCall& k) {
    const CoreDims& d = k.d;
    const CoreWs& w = k.w;
    StageTimer st(ST_NORM, k.s);
    if (k.cum) return fsn_launch_cumulative_den_sb(k.magT, w.fb_out, w.den_sb, d.B, d.Tp, d.F, d.FP, d.nb, d.den_stride, k.s);
    return fsn_launch_offline_den(w.binsum, w.fb_out, nullptr, w.den_sb, d.B, d.Tp, d.F, d.FP, d.nb, 1, k.s, k.lengths, d.T);
}

// Projection of layer 0 for the `tiles` row tiles per step from local row `first` on -> w.gx_sb (rows that run step by step)
static int core_sb_projection(const CoreCall& k, const FsnSbInput& xin, long first, int tiles) {
    StageTimer st(ST_SB_GEMM_L0, k.s);
    fsn_trace(FSN_TR_GEMM_SB_PROJ);
    // the provider works on global rows: first row and row limit
    return fsn_launch_gemm(gemm_a_subband(xin, k.d.row0 + first, tiles * 16), k.pk + k.p.sb_wih0,
                           gemm_c_frag(k.w.gx_sb, k.pk + k.p.sb_b0), k.d.Tp * tiles, 4 * k.d.Hs / 16, k.p.sb_kin_pad / 16, k.s);
}
// Output layer (model.py:53-61,129-135) of the `tiles` row tiles per step from local row `first` on, w.hseq_sb1 -> mask planes
static int core_sb_output(const CoreCall& k, long first, int tiles, hipStream_t s) {
    const CoreDims& d = k.d;
    fsn_trace(FSN_TR_GEMM_SB_OUT);
    // global rows, like the A provider above
    return fsn_launch_gemm(gemm_a_rows(k.w.hseq_sb1, d.Hs), k.pk + k.p.sb_fc,
                           gemm_c_masks(k.g, k.crm_r, k.crm_i, k.pk + k.p.sb_fcb, tiles * 16, d.row0 + first, d.row0 + d.N),
                           d.Tp * tiles, 1, d.Hs / 16, s);
}

// Few rows (6 - 9 utterances): both layers + output layer of the first 64 x clusters rows as ONE persistent launch
// (lstm_group_kernels.hip); what does not fill a cluster runs beside it on the auxiliary stream as the two-layer
// wavefront of per-step launches (its projection GEMM first, its output layer last).
static int core_sb_group(const CoreCall& k, const FsnSbInput& xin, const FsnRecFc& fc) {
    const CoreDims& d = k.d;
    const CoreWs& w = k.w;
    const Packed& p = k.p;
    const float* pk = k.pk;
    hipStream_t s = k.s;
    const long grp_rows = (long)d.grp_clusters * 64;
    const int aux_tiles = d.rec.tiles - d.grp_clusters * 4;
    FsnSbInput gin = xin;  // the launch's own rows only
    gin.N = d.N < grp_rows ? d.N : (int)grp_rows;
    FsnRecFc gfc = fc;
    gfc.N = gin.N;
    // The group kernel fills every CU with two 216-register workgroups: what runs beside it must fit in the 80
    // registers per lane that are left - the two-layer wavefront step kernel (78) and the output-layer GEMM (52) do,
    // the projection GEMM of the left-over rows does not, so it goes first, on the caller's stream.
    hipStream_t as = s;
    if (aux_tiles > 0) {
        FSN_TRY(core_sb_projection(k, xin, grp_rows, aux_tiles));
        FSN_TRY(aux_fork(s, &as));
    }
    {
        StageTimer st(ST_SB_REC_L0, s);
        FSN_PERSIST_BEGIN(s);
        FSN_TRY(fsn_launch_lstm2_group(&gin, pk + p.sb_whh0, pk + p.sb_wih1, pk + p.sb_whh1, pk + p.sb_b1,
                                       w.grp_exchange, w.grp_flags, &gfc, d.Tp, d.grp_clusters, d.Hs, s));
    }
    if (aux_tiles > 0) {
        FSN_TRY(fsn_launch_lstm_wavefront2(w.gx_sb, aux_tiles, 0, pk + p.sb_whh0, pk + p.sb_wih1, pk + p.sb_b1_frag,
                                           pk + p.sb_whh1, w.hseq_sb0, w.hseq_sb1, (long)aux_tiles * 16, 0, w.c_left,
                                           w.c_left + (size_t)aux_tiles * 16 * d.Hs, d.Tp, aux_tiles, d.Hs, as, nullptr,
                                           nullptr, 1));
        FSN_TRY(core_sb_output(k, grp_rows, aux_tiles, as));
        FSN_TRY(aux_join(s));
    }
    // a spin bound hit inside the group launch (see fsn_launch_poison_if): the mask planes become NaN instead of
    // garbage - AFTER the join: the left-over rows' output layer on the auxiliary stream writes into the same planes
    // (poisoned before it, a launch that gave up early left those rows finite: one run of the residency test in many)
    const unsigned* st_word = w.grp_flags + fsn_lstm2_group_status_word(d.grp_clusters);
    FSN_TRY(fsn_launch_poison_if(st_word, k.crm_r, (size_t)d.B * d.T * d.FP, s));
    return fsn_launch_poison_if(st_word, k.crm_i, (size_t)d.B * d.T * d.FP, s);
}

// Small batches (no persistent part, below the group kernel's range): the projection of every row, both layers as one
// wavefront of per-step launches on it, the output layer as a GEMM.
static int core_sb_wavefront(const CoreCall& k, const FsnSbInput& xin) {
    const CoreDims& d = k.d;
    const CoreWs& w = k.w;
    const Packed& p = k.p;
    const float* pk = k.pk;
    hipStream_t s = k.s;
    FSN_TRY(core_sb_projection(k, xin, 0, d.rec.left_tiles));
    {
        StageTimer st(ST_SB_REC_L0, s);
        FSN_TRY(fsn_launch_lstm_wavefront2(w.gx_sb, d.rec.left_tiles, 0, pk + p.sb_whh0, pk + p.sb_wih1, pk + p.sb_b1_frag,
                                           pk + p.sb_whh1, w.hseq_sb0, w.hseq_sb1, d.Npad, 0, w.c_left,
                                           w.c_left + (size_t)d.rec.left_tiles * 16 * d.Hs, d.Tp, d.rec.left_tiles,
                                           d.Hs, s));
    }
    StageTimer st(ST_SB_FC, s);
    return core_sb_output(k, 0, d.Npad / 16, s);
}

// The persistent pair: each layer as one persistent launch over its main rows, the few left-over row tiles step by step
// beside it (run_recurrence).
static int core_sb_persistent(const CoreCall& k, const FsnSbInput& xin, const FsnRecFc& fc) {
    const CoreDims& d = k.d;
    const CoreWs& w = k.w;
    const Packed& p = k.p;
    const float* pk = k.pk;
    hipStream_t s = k.s;
    const int sb_rt = (int)((long)d.Tp * d.Npad / 16);
    const long main_rows = (long)d.rec.main_wgs * d.rec.rt * 16;
    const bool f16x3 = k.cfg->arith == FSN_ARITH_F16X3;  // opt-in experiment, chosen by the caller
    // Output layer: where the persistent 4-pass kernel runs layer 1 it forms the two mask values of a row from h_t in
    // LDS and that layer's 4.8 GB hidden sequence is never written or read back; only rows that went step by step
    // (the left-over tiles) go through the GEMM at the end.
    const bool fc_fused = d.fc_fused;
    RecArgs both;  // what the two layers' calls share
    both.gx_left = w.gx_sb;
    both.c_left = w.c_left;
    both.Tp = d.Tp;
    both.Npad = d.Npad;
    both.H = d.Hs;
    both.plan = d.rec;
    // Layer 0: the K = 2nb+2 input projection is fused into the persistent recurrent kernel (no 19 GB
    // gx round trip); only the few left-over tiles, which run step by step, get a precomputed gx.
    if (d.rec.left_tiles > 0) FSN_TRY(core_sb_projection(k, xin, main_rows, d.rec.left_tiles));
    {
        StageTimer st(ST_SB_REC_L0, s);
        const bool l0_split = f16x3 && d.Hs == 384 && 2 * d.nb + 2 == 32;
        RecArgs l0 = both;
        l0.xin = &xin;
        l0.left_stride = d.rec.left_tiles;
        l0.whh = pk + p.sb_whh0;
        l0.hseq = w.hseq_sb0;
        l0.whh_f16x3 = l0_split ? pk + p.sb_whh0_f16x3 : nullptr;
        l0.wih_f16x3 = l0_split ? pk + p.sb_wih0_f16x3 : nullptr;
        l0.hseq_left = d.l1x ? w.hseq_left0 : nullptr;
        FSN_TRY(run_recurrence(l0, s));
    }
    RecArgs l1 = both;
    l1.whh = pk + p.sb_whh1;
    l1.hseq = w.hseq_sb1;
    l1.fc = fc_fused ? &fc : nullptr;
    l1.left_hs_stride = fc_fused ? (long)d.rec.left_tiles * 16 : -1;
    if (d.l1x) {
        // the main rows form this projection inside lstm_rec_x_kernel; only the left-over rows (step kernels) get one
        if (d.rec.left_tiles > 0) {
            StageTimer st(ST_SB_GEMM_L1, s);
            fsn_trace(FSN_TR_GEMM_SB_L1);
            FSN_TRY(fsn_launch_gemm(gemm_a_rows(w.hseq_left0, d.Hs), pk + p.sb_wih1, gemm_c_frag(w.gx_sb, pk + p.sb_b1),
                                    d.Tp * d.rec.left_tiles, 4 * d.Hs / 16, d.Hs / 16, s));
        }
        l1.left_stride = d.rec.left_tiles;
        l1.x_main = w.hseq_sb0;
        l1.wih_main = pk + p.sb_wih1;
        l1.bias_main = pk + p.sb_b1;
    } else {
        StageTimer st(ST_SB_GEMM_L1, s);
        fsn_trace(FSN_TR_GEMM_SB_L1);
        if (f16x3)
            FSN_TRY(fsn_launch_gemm_f16x3(w.hseq_sb0, d.Hs, pk + p.sb_wih1_f16x3, pk + p.sb_b1, w.gx_sb, sb_rt, 4 * d.Hs,
                                          d.Hs, s));
        else
            FSN_TRY(fsn_launch_gemm(gemm_a_rows(w.hseq_sb0, d.Hs), pk + p.sb_wih1, gemm_c_frag(w.gx_sb, pk + p.sb_b1), sb_rt,
                                    4 * d.Hs / 16, d.Hs / 16, s));
        l1.gx = w.gx_sb;
        l1.left_stride = d.rec.tiles;
        l1.left_off = main_rows / 16;
        l1.whh_f16x3 = f16x3 && fc_fused ? pk + p.sb_whh1_f16x3 : nullptr;
    }
    {
        StageTimer st(ST_SB_REC_L1, s);
        FSN_TRY(run_recurrence(l1, s));
    }
    if (!fc_fused || d.rec.left_tiles > 0) {
        StageTimer st(ST_SB_FC, s);
        // fused: only the left-over rows, hseq_sb1 is the compact [t][left rows][H] matrix
        FSN_TRY(fc_fused ? core_sb_output(k, main_rows, d.rec.left_tiles, s) : core_sb_output(k, 0, d.Npad / 16, s));
    }
    return FSN_OK;
}

// magT [B][Tp][FP] -> crm_r, crm_i [B][T][FP]: the full-band model, then the sub-band model (model.py:121-128: N = B F
// sequences, 2 LSTM layers + Linear(2)) in the regime of the plan `d`
static int run_core(const fsn_fullsubnet_cfg* cfg, const float* pk, const float* magT, const CoreDims& d,
                    const CoreWs& w, float* crm_r, float* crm_i, hipStream_t s, const int* lengths = nullptr) {
    const CoreCall k = core_call(cfg, pk, magT, d, w, crm_r, crm_i, s, lengths);
    FSN_TRY(core_fullband(k));
    FSN_TRY(core_sb_divisor(k));
    const FsnSbInput xin = sb_input_model(k.g, magT, w.fb_out, w.den_sb, k.cum ? 1 : 0, d.den_stride, pk + k.p.sb_wih0,
                                          pk + k.p.sb_b0, k.p.sb_kin_pad / 16, d.N, d.row0);
    const FsnRecFc fc = rec_fc(pk + k.p.sb_fc, pk + k.p.sb_fcb, crm_r, crm_i, d.N, d.row0, d.F, d.FP, d.T, d.la);
    if (d.grp_clusters > 0) return core_sb_group(k, xin, fc);
    if (d.rec.main_wgs == 0 && d.rec.left_tiles < kWavefrontBelowTiles) return core_sb_wavefront(k, xin);
    return core_sb_persistent(k, xin, fc);
}

static int check_bt(int B, int T) {
    FSN_REQUIRE(B >= 1 && B <= 4096, "batch %d out of range", B);
    FSN_REQUIRE(T >= 1 && T <= 100000, "frames %d out of range", T);
    return FSN_OK;
}

// Batches beyond what ONE round of the persistent kernels holds at 4 row tiles per workgroup (64 utterances of 257 bins
// on 256 CUs) run as whole chunks of that size plus a remainder, one after the other: the model has no cross-utterance
// term (both norms are per utterance), and a workgroup walks its RT tiles one after the other every step, so a batch
// that does not fill rounds x RT x CUs tiles pays for the full round - 104 utterances took 171 ms as two rounds of 4,
// 64 + 40 take 84 + 63.  Returns the chunk size (B itself: no chunking).
static int core_chunk(const fsn_fullsubnet_cfg* cfg, int B) {
    const int cus = plan_cus();
    const long b0 = ((long)cus * 4 + 16) * 16 / cfg->num_freqs;
    return b0 >= 1 && B > b0 ? (int)b0 : B;
}
// Below one round the same holds between the regimes: 40 utterances take as long as 48 (one round of 3 tiles per
// workgroup), 24 as long as 32, 10 - 13 run at one tile per CU - where 32 + 8, 16 + 8 and 8 + 2 as separate calls are 12 -
// 18 % faster.  Time of one core call in microseconds per frame step, from the plan it would take (calibrated on
// config 2's clips: 1 / 2 / 4 / 8 / 16 / 32 / 48 / 64 utterances = 24 / 37 / 60 / 66 / 122 / 229 / 337 / 441 us per step):
static double core_cost(const fsn_fullsubnet_cfg* cfg, int b) {
    const int cus = plan_cus();
    const CoreDims d = core_dims(cfg, b, 64);
    double c = 6.0;  // the full-band chain and the fixed launches of a call
    if (d.rec.main_wgs > 0) {
        const int rounds = (d.rec.main_wgs + cus - 1) / cus;
        c += rounds * (d.rec.rt == 1 ? 120.0 : 110.0 * d.rec.rt);  // one tile per CU streams all weights for 16 rows
    } else if (d.grp_clusters > 0) {
        c += (d.grp_clusters > cus / 8 ? 2 : 1) * 58.0 + (d.rec.left_tiles - 4 * d.grp_clusters > 0 ? 2.0 : 0.0);
    } else {
        c += 7.0 + 0.67 * d.rec.left_tiles;  // two-layer wavefront of per-step launches
    }
    return c;
}
// the chunk sizes of a batch, largest first: whole rounds of core_chunk(), then the cheapest split of the remainder into
// {itself, 48, 32, 16, 8}-utterance calls by core_cost
static int core_chunks_search(const fsn_fullsubnet_cfg* cfg, int B, int* sizes, int max_sizes);
// The search evaluates core_cost / core_dims ~5 x (remainder) times, each with device-attribute and occupancy lookups:
// ~10^4 host calls at B = 64, three times per fsn_enhance (workspace query, workspace check, run).  The plan depends
// only on (configuration, B, device, persistent mode): memoised.
static int core_chunks(const fsn_fullsubnet_cfg* cfg, int B, int* sizes, int max_sizes) {
    static std::mutex mu;
    static std::map<std::string, std::vector<int>> memo;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::string key(reinterpret_cast<const char*>(cfg), sizeof(*cfg));
    const int tail[4] = {B, dev, fsn_persistent_allowed() ? 1 : 0, max_sizes};
    key.append(reinterpret_cast<const char*>(tail), sizeof(tail));
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = memo.find(key);
        if (it != memo.end()) {
            for (size_t i = 0; i < it->second.size(); ++i) sizes[i] = it->second[i];
            return (int)it->second.size();
        }
    }
    const int n = core_chunks_search(cfg, B, sizes, max_sizes);
    std::lock_guard<std::mutex> lk(mu);
    if (memo.size() > 4096) memo.clear();
    memo[key] = std::vector<int>(sizes, sizes + n);
    return n;
}
static int core_chunks_search(const fsn_fullsubnet_cfg* cfg, int B, int* sizes, int max_sizes) {
    int n = 0;
    const int full = core_chunk(cfg, B);
    int rem = B;
    while (rem > full && n < max_sizes - 8) {
        sizes[n++] = full;
        rem -= full;
    }
    if (rem > 64 || !fsn_persistent_allowed() || cfg->arith != FSN_ARITH_F32) {  // outside the calibrated range: as one call
        sizes[n++] = rem;
        return n;
    }
    double best[65];
    int first[65];
    best[0] = 0.0;
    first[0] = 0;
    for (int b = 1; b <= rem; ++b) {
        best[b] = core_cost(cfg, b);
        first[b] = b;
        for (int c : {48, 32, 16, 8}) {
            if (c >= b) continue;
            const double v = core_cost(cfg, c) + best[b - c];
            if (v < 0.97 * best[b]) {  // a split has to be worth it
                best[b] = v;
                first[b] = c;
            }
        }
    }
    const int rem_begin = n;
    for (int b = rem; b > 0 && n < max_sizes; b -= first[b]) sizes[n++] = first[b];
    // largest first, as documented: the search puts the round size it picked before what is left, which may be the
    // larger (17 utterances: 8, then 9 - found on the device by tests/test_host_cpu.py, whose plans need one)
    std::sort(sizes + rem_begin, sizes + n, std::greater<int>());
    return n;
}
constexpr int kMaxChunks = 80;  // 4096 utterances (check_bt) in rounds of >= 64, plus the remainder's few calls
// the core's scratch behind the per-batch planes: sized for the largest chunk's plan (the chunks reuse it)
static void core_carve_chunks(Carver& cv, const fsn_fullsubnet_cfg* cfg, int B, int T) {
    int sizes[kMaxChunks];
    const int n = core_chunks(cfg, B, sizes, kMaxChunks);
    size_t most = 0;
    for (int i = 0; i < n; ++i) {
        if (i > 0 && sizes[i] == sizes[i - 1]) continue;
        Carver c2(nullptr);
        core_carve(c2, core_dims(cfg, sizes[i], T), cfg->norm_type);
        most = c2.off > most ? c2.off : most;
    }
    cv.take<char>(most);
}
// run_core over the chunks; `scratch` = a region of at least core_carve_chunks' size; lengths: see run_core
static int run_core_chunks(const fsn_fullsubnet_cfg* cfg, const float* pk, const float* magT, int B, int T, void* scratch,
                           float* crm_r, float* crm_i, hipStream_t s, const int* lengths = nullptr) {
    int sizes[kMaxChunks];
    const int n = core_chunks(cfg, B, sizes, kMaxChunks);
    int b0 = 0;
    for (int i = 0; i < n; ++i) {
        const int b = sizes[i];
        const CoreDims d = core_dims(cfg, b, T);
        Carver cv(scratch);
        const CoreWs w = core_carve(cv, d, cfg->norm_type);
        FSN_TRY(run_core(cfg, pk, magT + (size_t)b0 * d.Tp * d.FP, d, w, crm_r + (size_t)b0 * d.T * d.FP,
                         crm_i + (size_t)b0 * d.T * d.FP, s, lengths ? lengths + b0 : nullptr));
        b0 += b;
    }
    FSN_REQUIRE(b0 == B, "internal: the chunks cover %d of %d utterances", b0, B);
    return FSN_OK;
}

// test hook: the utterance counts of the core calls a batch of B runs as (sum = B); returns their number
extern "C" int fsn_debug_core_chunks(const fsn_fullsubnet_cfg* cfg, int B, int* sizes, int max_sizes) {
    if (check_cfg(cfg) != FSN_OK || B < 1 || B > 4096 || !sizes || max_sizes < kMaxChunks) return -1;
    return core_chunks(cfg, B, sizes, kMaxChunks);
}

extern "C" int fsn_debug_core_plan(const fsn_fullsubnet_cfg* cfg, int B, int T, int* plan, int n) {
    if (check_cfg(cfg) != FSN_OK || check_bt(B, T) != FSN_OK || !plan || n < 8) return -1;
    int sizes[kMaxChunks];
    const int chunks = core_chunks(cfg, B, sizes, kMaxChunks);
    const CoreDims d = core_dims(cfg, chunks > 0 ? sizes[0] : B, T);
    plan[0] = d.N;
    plan[1] = d.rec.tiles;
    plan[2] = d.rec.rt;
    plan[3] = d.rec.main_wgs;
    plan[4] = d.rec.left_tiles;
    plan[5] = d.grp_clusters;
    plan[6] = d.fb_chain ? 1 : 0;
    plan[7] = chunks;
    if (n >= 9) {  // rows on the persistent recurrent pair over ALL chunks (whole rounds and a remainder have different plans)
        long rows = 0;
        for (int c = 0; c < (chunks > 0 ? chunks : 1); ++c) {
            const CoreDims dc = core_dims(cfg, chunks > 0 ? sizes[c] : B, T);
            rows += (long)dc.rec.main_wgs * dc.rec.rt * 16;
        }
        plan[8] = (int)rows;
    }
    return FSN_OK;
}

// the CoreDims of one core call, whole utterances or a row slice (defined with the row-range form below)
static int core_call_dims(const fsn_fullsubnet_cfg* cfg, int B, int T, long row_begin, long row_end, CoreDims* d);

extern "C" int fsn_debug_core_call_plan(const fsn_fullsubnet_cfg* cfg, int B, int T, long row_begin, long row_end, int* plan,
                                        int n) {
    if (check_cfg(cfg) != FSN_OK || check_bt(B, T) != FSN_OK || !plan || n < 15) return -1;
    CoreDims d;
    if (core_call_dims(cfg, B, T, row_begin, row_end, &d) != FSN_OK) return -1;
    const StepSplit split = step_split(d.rec);
    const bool persistent = d.grp_clusters == 0 && !(d.rec.main_wgs == 0 && d.rec.left_tiles < kWavefrontBelowTiles);
    plan[0] = d.N;
    plan[1] = d.rec.tiles;
    plan[2] = d.Npad;
    plan[3] = d.rec.rt;
    plan[4] = d.rec.main_wgs;
    plan[5] = d.rec.left_tiles;
    plan[6] = d.grp_clusters;
    plan[7] = d.grp_clusters > 0 ? d.rec.tiles - 4 * d.grp_clusters : 0;
    plan[8] = persistent ? split.cu_tiles : 0;   // run_recurrence is only reached in the persistent / step regime
    plan[9] = persistent ? split.aux_tiles : 0;
    plan[10] = d.fb_chain ? 1 : 0;
    plan[11] = d.Npad_fb;
    plan[12] = d.fc_fused ? 1 : 0;
    plan[13] = d.l1x ? 1 : 0;
    plan[14] = packed_layout(cfg).sb_kin_pad / 16;
    return FSN_OK;
}

extern "C" size_t fsn_fullsubnet_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int T) {
    if (check_cfg(cfg) != FSN_OK || check_bt(B, T) != FSN_OK) return 0;
    const CoreDims d = core_dims(cfg, B, T);
    Carver cv(nullptr);
    cv.take<float>((size_t)B * d.Tp * d.FP);     // magT
    cv.take<float>((size_t)B * d.T * d.FP);      // crm_r
    cv.take<float>((size_t)B * d.T * d.FP);      // crm_i
    // the whole batch's plan (what the stage-level entries carve) is never smaller than a chunk's; both are checked
    Carver whole(nullptr), parts(nullptr);
    core_carve(whole, d, cfg->norm_type);
    core_carve_chunks(parts, cfg, B, T);
    cv.take<char>(whole.off > parts.off ? whole.off : parts.off);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_fullsubnet_forward(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* noisy_mag,
                                      int B, int T, float* crm_out, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_cfg(cfg));
    FSN_TRY(check_bt(B, T));
    FSN_REQUIRE(packed && noisy_mag && crm_out && workspace, "NULL pointer argument");
    const size_t need = fsn_fullsubnet_workspace_bytes(cfg, B, T);
    if (workspace_bytes < need) {
        fsn_set_error("workspace too small: %zu < %zu bytes", workspace_bytes, need);
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CoreDims d = core_dims(cfg, B, T);
    Carver cv(workspace);
    float* magT = cv.take<float>((size_t)B * d.Tp * d.FP);
    float* crm_r = cv.take<float>((size_t)B * d.T * d.FP);
    float* crm_i = cv.take<float>((size_t)B * d.T * d.FP);
    void* scratch = cv.take<char>(0);  // the rest: the core's scratch (fsn_fullsubnet_workspace_bytes)
    prof_reset();
    // [B,1,F,T] -> frame-major [B][Tp][FP]; look-ahead frames (model.py:85) and padded bins are zeros
    FSN_TRY(fsn_launch_transpose(noisy_mag, magT, B, d.FP, d.Tp, T, (long)d.F * T, d.FP, (long)d.Tp * d.FP, d.F, T, s));
    FSN_TRY(run_core_chunks(cfg, static_cast<const float*>(packed), magT, B, T, scratch, crm_r, crm_i, s));
    // frame-major planes -> [B, 2, F, T] (model.py:129-135)
    FSN_TRY(fsn_launch_transpose(crm_r, crm_out, B, T, d.F, d.FP, (long)T * d.FP, T, 2L * d.F * T, T, d.F, s));
    FSN_TRY(fsn_launch_transpose(crm_i, crm_out + (size_t)d.F * T, B, T, d.F, d.FP, (long)T * d.FP, T, 2L * d.F * T,
                                 T, d.F, s));
    return FSN_OK;
}

// ---- the full-band stage alone: model.py:85-95 ---------------------------------------------------
// look-ahead pad -> norm -> fb_model, i.e. the tensor `fb_output` of model.py:95 in the reference's layout
// [B, F, T + look_ahead].  Stage-level parity checks read it; a batch-sharded full-band model would too.
extern "C" int fsn_fullsubnet_fullband(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* noisy_mag,
                                       int B, int T, float* fb_output, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_cfg(cfg));
    FSN_TRY(check_bt(B, T));
    FSN_REQUIRE(packed && noisy_mag && fb_output && workspace, "NULL pointer argument");
    const size_t need = fsn_fullsubnet_workspace_bytes(cfg, B, T);
    if (workspace_bytes < need) {
        fsn_set_error("workspace too small: %zu < %zu bytes", workspace_bytes, need);
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CoreDims d = core_dims(cfg, B, T);
    Carver cv(workspace);
    float* magT = cv.take<float>((size_t)B * d.Tp * d.FP);
    cv.take<float>((size_t)B * d.T * d.FP);
    cv.take<float>((size_t)B * d.T * d.FP);
    const CoreWs w = core_carve(cv, d, cfg->norm_type);
    prof_reset();
    FSN_TRY(fsn_launch_transpose(noisy_mag, magT, B, d.FP, d.Tp, T, (long)d.F * T, d.FP, (long)d.Tp * d.FP, d.F, T, s));
    FSN_TRY(core_fullband(core_call(cfg, static_cast<const float*>(packed), magT, d, w, nullptr, nullptr, s, nullptr)));
    // frame-major [B][T'][FP] -> [B, F, T']
    FSN_TRY(fsn_launch_transpose(w.fb_out, fb_output, B, d.Tp, d.F, d.FP, (long)d.Tp * d.FP, d.Tp, (long)d.F * d.Tp,
                                 d.Tp, d.F, s));
    return FSN_OK;
}

// ---- row-range form: the sub-band model on a contiguous slice of the flattened (b, f) rows -------------------
// "rank r owns a contiguous slice of the flattened (b, f) index space".  Only the utterances the
// slice touches are looked at: their full-band model and norm statistics are computed whole (they couple all
// bins of an utterance), the sub-band model only on rows [row_begin, row_end).  A slice that is aligned to
// utterances is exactly fsn_fullsubnet_forward on those utterances.
struct RowSlice {
    int b_lo, Bs;
    long r0, n;
};
static int row_slice(const fsn_fullsubnet_cfg* cfg, int B, long row_begin, long row_end, RowSlice* out) {
    const long F = cfg->num_freqs;
    FSN_REQUIRE(row_begin >= 0 && row_begin < row_end && row_end <= (long)B * F,
                "row range [%ld, %ld) is not inside the %ld sub-band rows of the batch", row_begin, row_end, (long)B * F);
    out->b_lo = (int)(row_begin / F);
    out->Bs = (int)((row_end - 1) / F) - out->b_lo + 1;
    out->r0 = row_begin - (long)out->b_lo * F;
    out->n = row_end - row_begin;
    return FSN_OK;
}

// The CoreDims of ONE core call: row_end < 0 - the B utterances whole, as a chunk of fsn_fullsubnet_forward runs them;
// otherwise the slice [row_begin, row_end) exactly as fsn_fullsubnet_forward_rows forms it.
static int core_call_dims(const fsn_fullsubnet_cfg* cfg, int B, int T, long row_begin, long row_end, CoreDims* d) {
    if (row_end < 0) {
        *d = core_dims(cfg, B, T);
        return FSN_OK;
    }
    RowSlice r;
    FSN_TRY(row_slice(cfg, B, row_begin, row_end, &r));
    *d = core_dims(cfg, r.Bs, T, r.r0, r.n);
    return FSN_OK;
}

extern "C" size_t fsn_fullsubnet_rows_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int T, long row_begin,
                                                      long row_end) {
    RowSlice r;
    if (check_cfg(cfg) != FSN_OK || check_bt(B, T) != FSN_OK || row_slice(cfg, B, row_begin, row_end, &r) != FSN_OK)
        return 0;
    CoreDims d;
    if (core_call_dims(cfg, B, T, row_begin, row_end, &d) != FSN_OK) return 0;
    Carver cv(nullptr);
    cv.take<float>((size_t)r.Bs * d.Tp * d.FP);  // magT
    cv.take<float>((size_t)r.Bs * d.T * d.FP);   // crm_r
    cv.take<float>((size_t)r.Bs * d.T * d.FP);   // crm_i
    core_carve(cv, d, cfg->norm_type);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_fullsubnet_forward_rows(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* noisy_mag,
                                           int B, int T, long row_begin, long row_end, float* crm_rows,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_cfg(cfg));
    FSN_TRY(check_bt(B, T));
    RowSlice r;
    FSN_TRY(row_slice(cfg, B, row_begin, row_end, &r));
    FSN_REQUIRE(packed && noisy_mag && crm_rows && workspace, "NULL pointer argument");
    const size_t need = fsn_fullsubnet_rows_workspace_bytes(cfg, B, T, row_begin, row_end);
    if (workspace_bytes < need) {
        fsn_set_error("workspace too small: %zu < %zu bytes", workspace_bytes, need);
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    CoreDims d;
    FSN_TRY(core_call_dims(cfg, B, T, row_begin, row_end, &d));
    Carver cv(workspace);
    float* magT = cv.take<float>((size_t)r.Bs * d.Tp * d.FP);
    float* crm_r = cv.take<float>((size_t)r.Bs * d.T * d.FP);
    float* crm_i = cv.take<float>((size_t)r.Bs * d.T * d.FP);
    const CoreWs w = core_carve(cv, d, cfg->norm_type);
    prof_reset();
    const float* mag_lo = noisy_mag + (size_t)r.b_lo * d.F * T;  // [B, 1, F, T]: utterances are contiguous
    FSN_TRY(fsn_launch_transpose(mag_lo, magT, r.Bs, d.FP, d.Tp, T, (long)d.F * T, d.FP, (long)d.Tp * d.FP, d.F, T, s));
    FSN_TRY(run_core(cfg, static_cast<const float*>(packed), magT, d, w, crm_r, crm_i, s));
    // this slice's rows of the frame-major planes -> [row][2][T] (what the ranks all-gather)
    FSN_TRY(fsn_launch_crm_rows(crm_r, crm_i, crm_rows, r.r0, r.n, d.F, d.FP, T, s));
    return FSN_OK;
}


// ---- streaming: k more frames of the model with carried state -------------------------------------
// State (caller-owned, zero-filled for a new stream): (h, c) of the four LSTM layers and the running sums
// of the two cumulative Laplace norms.
struct StreamState {
    float *fb_h0, *fb_h1, *fb_c0, *fb_c1, *sb_h0, *sb_h1, *sb_c0, *sb_c1;
    double *fb_sum, *sb_sum;
};
static StreamState stream_carve(Carver& cv, const fsn_fullsubnet_cfg* cfg, int B) {
    StreamState st;
    const size_t nfb = (size_t)fsn_round_up(B, 16) * cfg->fb_hidden;
    const size_t nsb = (size_t)fsn_round_up(B * cfg->num_freqs, 16) * cfg->sb_hidden;
    st.fb_h0 = cv.take<float>(nfb);
    st.fb_h1 = cv.take<float>(nfb);
    st.fb_c0 = cv.take<float>(nfb);
    st.fb_c1 = cv.take<float>(nfb);
    st.sb_h0 = cv.take<float>(nsb);
    st.sb_h1 = cv.take<float>(nsb);
    st.sb_c0 = cv.take<float>(nsb);
    st.sb_c1 = cv.take<float>(nsb);
    st.fb_sum = cv.take<double>((size_t)B);
    st.sb_sum = cv.take<double>((size_t)B * cfg->num_freqs);
    return st;
}
struct StreamWs {
    float *magT, *crm_r, *crm_i, *den_fb, *gx_fb, *hseq_fb0, *hseq_fb1, *fb_out, *den_sb, *gx_sb, *hseq_sb0, *hseq_sb1;
};
static StreamWs stream_ws_carve(Carver& cv, const fsn_fullsubnet_cfg* cfg, int B, int k) {
    StreamWs w;
    const int FP = fsn_fpad(cfg->num_freqs), Npad_fb = fsn_round_up(B, 16), Npad = fsn_round_up(B * cfg->num_freqs, 16);
    const size_t plane = (size_t)B * k * FP;
    w.magT = cv.take<float>(plane);
    w.crm_r = cv.take<float>(plane);
    w.crm_i = cv.take<float>(plane);
    w.den_fb = cv.take<float>((size_t)B * k);
    w.gx_fb = cv.take<float>((size_t)k * Npad_fb * 4 * cfg->fb_hidden);
    w.hseq_fb0 = cv.take<float>((size_t)k * Npad_fb * cfg->fb_hidden);
    w.hseq_fb1 = cv.take<float>((size_t)k * Npad_fb * cfg->fb_hidden);
    w.fb_out = cv.take<float>(plane);
    w.den_sb = cv.take<float>((size_t)k * Npad);
    w.gx_sb = cv.take<float>((size_t)k * Npad * 4 * cfg->sb_hidden);
    w.hseq_sb0 = cv.take<float>((size_t)k * Npad * cfg->sb_hidden);
    w.hseq_sb1 = cv.take<float>((size_t)k * Npad * cfg->sb_hidden);
    return w;
}
static int check_stream(const fsn_fullsubnet_cfg* cfg, int B, int k) {
    FSN_TRY(check_cfg(cfg));
    FSN_REQUIRE(cfg->norm_type == FSN_NORM_CUMULATIVE_LAPLACE, "streaming needs the causal norm (FSN_NORM_CUMULATIVE_LAPLACE)");
    FSN_REQUIRE(B >= 1 && B <= 4096 && k >= 1 && k <= 4096, "streaming: batch %d / frames %d out of range", B, k);
    return FSN_OK;
}
extern "C" size_t fsn_fullsubnet_stream_state_bytes(const fsn_fullsubnet_cfg* cfg, int B) {
    if (check_stream(cfg, B, 1) != FSN_OK) return 0;
    Carver cv(nullptr);
    stream_carve(cv, cfg, B);
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" size_t fsn_fullsubnet_stream_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int k) {
    if (check_stream(cfg, B, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    stream_ws_carve(cv, cfg, B, k);
    return fsn_round_up_sz(cv.off, 256);
}

// The two halves of the model step on n rows for k frames with carried state.  den_mode: how the half's divisors are laid out (0: one per row of the batch, the offline
// norm of the segment entries; 1: one per frame - w.den_fb [n][k], w.den_sb [k][Npad] - the cumulative norm).
// Full-band half: w.magT / w.den_fb -> w.fb_out [n][k][FP]; fb = the (h0, h1, c0, c1) rows of its two layers.
static int stream_fullband(const fsn_fullsubnet_cfg* cfg, const float* pk, const StreamWs& w, float* const fb[4], int n, int k,
                           int den_mode, hipStream_t s) {
    const Packed p = packed_layout(cfg);
    const int F = cfg->num_freqs, FP = fsn_fpad(F), Hf = cfg->fb_hidden;
    const int Npad_fb = fsn_round_up(n, 16);
    // la = 0: every model step is handed back; the caller matches step s to output frame s - look_ahead
    const ModelGeom g{n, k, k, F, FP, cfg->sb_num_neighbors, 0};
    const int fb_rt = k * Npad_fb / 16;
    FSN_TRY(fsn_launch_gemm(gemm_a_fullband(g, w.magT, w.den_fb, den_mode, Npad_fb), pk + p.fb_wih0,
                            gemm_c_frag(w.gx_fb, pk + p.fb_b0), fb_rt, 4 * Hf / 16, FP / 16, s));
    FSN_TRY(fsn_launch_lstm_wavefront2(w.gx_fb, Npad_fb / 16, 0, pk + p.fb_whh0, pk + p.fb_wih1, pk + p.fb_b1_frag,
                                       pk + p.fb_whh1, w.hseq_fb0, w.hseq_fb1, Npad_fb, 0, fb[2], fb[3], k, Npad_fb / 16, Hf,
                                       s, fb[0], fb[1]));
    return fsn_launch_gemm(gemm_a_rows(w.hseq_fb1, Hf), pk + p.fb_fc, gemm_c_fb_out(g, w.fb_out, pk + p.fb_fcb, Npad_fb), fb_rt,
                           FP / 16, Hf / 16, s);
}
// Sub-band half: w.magT / w.fb_out / w.den_sb -> w.crm_r / w.crm_i -> crm_out [n, 2, F, k]; sb = its layers' state rows.
static int stream_subband(const fsn_fullsubnet_cfg* cfg, const float* pk, const StreamWs& w, float* const sb[4], int n, int k,
                          int den_mode, float* crm_out, hipStream_t s) {
    const Packed p = packed_layout(cfg);
    const int F = cfg->num_freqs, FP = fsn_fpad(F), Hs = cfg->sb_hidden;
    const int N = n * F, Npad = fsn_round_up(N, 16);
    const ModelGeom g{n, k, k, F, FP, cfg->sb_num_neighbors, 0};
    const FsnSbInput xin = sb_input_model(g, w.magT, w.fb_out, w.den_sb, den_mode, Npad, pk + p.sb_wih0, pk + p.sb_b0,
                                          p.sb_kin_pad / 16, N, 0);
    const int sb_rt = (int)((long)k * Npad / 16);
    FSN_TRY(fsn_launch_gemm(gemm_a_subband(xin, 0, Npad), pk + p.sb_wih0, gemm_c_frag(w.gx_sb, pk + p.sb_b0), sb_rt,
                            4 * Hs / 16, p.sb_kin_pad / 16, s));
    FSN_TRY(fsn_launch_lstm_wavefront2(w.gx_sb, Npad / 16, 0, pk + p.sb_whh0, pk + p.sb_wih1, pk + p.sb_b1_frag,
                                       pk + p.sb_whh1, w.hseq_sb0, w.hseq_sb1, Npad, 0, sb[2], sb[3], k, Npad / 16, Hs, s,
                                       sb[0], sb[1]));
    FSN_TRY(fsn_launch_gemm(gemm_a_rows(w.hseq_sb1, Hs), pk + p.sb_fc,
                            gemm_c_masks(g, w.crm_r, w.crm_i, pk + p.sb_fcb, Npad, 0, N), sb_rt, 1, Hs / 16, s));
    FSN_TRY(fsn_launch_transpose(w.crm_r, crm_out, n, k, F, FP, (long)k * FP, k, 2L * F * k, k, F, s));
    return fsn_launch_transpose(w.crm_i, crm_out + (size_t)F * k, n, k, F, FP, (long)k * FP, k, 2L * F * k, k, F, s);
}
// The model step on n rows for k frames with carried state: w.magT [n][k][FP] -> w.crm_r / w.crm_i -> crm_out [n, 2, F, k].
// fb / sb: the (h0, h1, c0, c1) rows of the full-band / sub-band layers, updated in place; den_fb() / den_sb() launch the
// cumulative norm's divisors (w.den_fb from w.magT; w.den_sb from w.magT and w.fb_out) from wherever the carries live.
template <class DenFb, class DenSb>
static int stream_sequence(const fsn_fullsubnet_cfg* cfg, const float* pk, const StreamWs& w, float* const fb[4],
                           float* const sb[4], int n, int k, float* crm_out, const DenFb& den_fb, const DenSb& den_sb,
                           hipStream_t s) {
    FSN_TRY(den_fb());
    FSN_TRY(stream_fullband(cfg, pk, w, fb, n, k, 1, s));
    FSN_TRY(den_sb());
    return stream_subband(cfg, pk, w, sb, n, k, 1, crm_out, s);
}

extern "C" int fsn_fullsubnet_stream_step(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state,
                                          size_t state_bytes, int steps_done, const float* mag, int B, int k,
                                          float* crm_out, void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_stream(cfg, B, k));
    FSN_REQUIRE(packed && state && mag && crm_out && workspace && steps_done >= 0, "NULL pointer argument / negative step count");
    if (state_bytes < fsn_fullsubnet_stream_state_bytes(cfg, B) ||
        workspace_bytes < fsn_fullsubnet_stream_workspace_bytes(cfg, B, k)) {
        fsn_set_error("streaming: state / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->num_freqs, FP = fsn_fpad(F), nb = cfg->sb_num_neighbors, Npad = fsn_round_up(B * F, 16);
    Carver cs(state), cw(workspace);
    const StreamState st = stream_carve(cs, cfg, B);
    const StreamWs w = stream_ws_carve(cw, cfg, B, k);
    float* const fb[4] = {st.fb_h0, st.fb_h1, st.fb_c0, st.fb_c1};
    float* const sb[4] = {st.sb_h0, st.sb_h1, st.sb_c0, st.sb_c1};
    // [B, 1, F, k] -> frame-major [B][k][FP]
    FSN_TRY(fsn_launch_transpose(mag, w.magT, B, FP, k, k, (long)F * k, FP, (long)k * FP, F, k, s));
    return stream_sequence(
        cfg, static_cast<const float*>(packed), w, fb, sb, B, k, crm_out,
        [&] { return fsn_launch_cumulative_den_fb(w.magT, w.den_fb, B, k, F, FP, s, st.fb_sum, steps_done); },
        [&] {
            return fsn_launch_cumulative_den_sb(w.magT, w.fb_out, w.den_sb, B, k, F, FP, nb, Npad, s, st.sb_sum, steps_done);
        },
        s);
}

// ---- streaming pool: the same step over a subset of the slots of a pool --------------------------------------------
// State: one record per slot (FsnPoolLayout, fsn_common.h).  A step gathers the listed slots' (h, c) rows into compact
// tiles in the workspace, runs stream_sequence on them with per-slot norm carries and step counts, and scatters the rows
// back (stream_pool_kernels.hip).
static FsnPoolLayout pool_layout(const fsn_fullsubnet_cfg* cfg) {
    return fsn_pool_layout(cfg->num_freqs, cfg->fb_hidden, cfg->sb_hidden, cfg->look_ahead);
}
static int check_pool(const fsn_fullsubnet_cfg* cfg, int capacity) {
    FSN_TRY(check_stream(cfg, 1, 1));
    FSN_REQUIRE(capacity >= 1 && capacity <= 4096, "streaming pool: capacity %d out of range [1, 4096]", capacity);
    return FSN_OK;
}
static int check_pool_call(const fsn_fullsubnet_cfg* cfg, const void* state, size_t state_bytes, int capacity,
                           const int* slots, int n) {
    FSN_TRY(check_pool(cfg, capacity));
    FSN_REQUIRE(state && slots, "NULL pointer argument");
    FSN_REQUIRE(n >= 1 && n <= capacity, "streaming pool: %d slots listed, need 1 .. capacity = %d", n, capacity);
    if (state_bytes < (size_t)capacity * pool_layout(cfg).slot_bytes) {
        fsn_set_error("streaming pool: state buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}
struct PoolTilesWs {
    float *fb[4], *sb[4];  // h0, h1, c0, c1
};
static PoolTilesWs pool_tiles_carve(Carver& cv, const fsn_fullsubnet_cfg* cfg, int n) {
    PoolTilesWs t;
    const size_t nfb = (size_t)fsn_round_up(n, 16) * cfg->fb_hidden;
    const size_t nsb = (size_t)fsn_round_up(n * cfg->num_freqs, 16) * cfg->sb_hidden;
    for (int a = 0; a < 4; ++a) t.fb[a] = cv.take<float>(nfb);
    for (int a = 0; a < 4; ++a) t.sb[a] = cv.take<float>(nsb);
    return t;
}

extern "C" size_t fsn_fullsubnet_stream_pool_state_bytes(const fsn_fullsubnet_cfg* cfg, int capacity) {
    if (check_pool(cfg, capacity) != FSN_OK) return 0;
    return (size_t)capacity * pool_layout(cfg).slot_bytes;
}
extern "C" size_t fsn_fullsubnet_stream_pool_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int n, int k) {
    if (check_stream(cfg, n, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    stream_ws_carve(cv, cfg, n, k);
    pool_tiles_carve(cv, cfg, n);
    return fsn_round_up_sz(cv.off, 256);
}

extern "C" int fsn_fullsubnet_stream_pool_reset(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes,
                                                int capacity, const int* slots, int n, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    return fsn_launch_pool_reset(state, pool_layout(cfg), capacity, slots, n, static_cast<hipStream_t>(stream));
}

extern "C" int fsn_fullsubnet_stream_pool_step(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state,
                                               size_t state_bytes, int capacity, const int* slots, int n, const float* mag,
                                               int k, float* crm_out, void* workspace, size_t workspace_bytes,
                                               void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_stream(cfg, n, k));
    FSN_REQUIRE(packed && mag && crm_out && workspace, "NULL pointer argument");
    if (workspace_bytes < fsn_fullsubnet_stream_pool_workspace_bytes(cfg, n, k)) {
        fsn_set_error("streaming pool: workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const FsnPoolLayout L = pool_layout(cfg);
    const int F = cfg->num_freqs, FP = fsn_fpad(F), nb = cfg->sb_num_neighbors;
    const int Npad_fb = fsn_round_up(n, 16), Npad = fsn_round_up(n * F, 16);
    Carver cw(workspace);
    const StreamWs w = stream_ws_carve(cw, cfg, n, k);
    const PoolTilesWs t = pool_tiles_carve(cw, cfg, n);
    // [n, 1, F, k] -> frame-major [n][k][FP]
    FSN_TRY(fsn_launch_transpose(mag, w.magT, n, FP, k, k, (long)F * k, FP, (long)k * FP, F, k, s));
    FSN_TRY(fsn_launch_pool_gather(state, L, capacity, slots, n, 0, t.fb[0], t.fb[1], t.fb[2], t.fb[3], Npad_fb, s));
    FSN_TRY(fsn_launch_pool_gather(state, L, capacity, slots, n, 1, t.sb[0], t.sb[1], t.sb[2], t.sb[3], Npad, s));
    FSN_TRY(stream_sequence(
        cfg, static_cast<const float*>(packed), w, t.fb, t.sb, n, k, crm_out,
        [&] { return fsn_launch_pool_den_fb(w.magT, w.den_fb, state, L, capacity, slots, n, k, s); },
        [&] { return fsn_launch_pool_den_sb(w.magT, w.fb_out, w.den_sb, state, L, capacity, slots, n, k, nb, Npad, s); }, s));
    FSN_TRY(fsn_launch_pool_scatter(state, L, capacity, slots, n, 0, t.fb[0], t.fb[1], t.fb[2], t.fb[3], Npad_fb, k, s));
    // last: it advances the listed slots' step counts
    return fsn_launch_pool_scatter(state, L, capacity, slots, n, 1, t.sb[0], t.sb[1], t.sb[2], t.sb[3], Npad, k, s);
}

// test hooks (host only): where the arrays of the two state blobs lie, from the code the entries carve them with
extern "C" int fsn_debug_stream_state_layout(const fsn_fullsubnet_cfg* cfg, int B, long* out, int n) {
    if (check_cfg(cfg) != FSN_OK || B < 1 || B > 4096 || !out || n < 13) return -1;
    char* const base = reinterpret_cast<char*>((uintptr_t)1 << 20);  // never dereferenced: only differences are taken
    Carver cv(base);
    const StreamState st = stream_carve(cv, cfg, B);
    const void* const at[10] = {st.fb_h0, st.fb_h1, st.fb_c0, st.fb_c1, st.sb_h0, st.sb_h1, st.sb_c0, st.sb_c1, st.fb_sum, st.sb_sum};
    for (int i = 0; i < 10; ++i) out[i] = (long)(static_cast<const char*>(at[i]) - base);
    out[10] = fsn_round_up(B, 16);
    out[11] = fsn_round_up(B * cfg->num_freqs, 16);
    out[12] = (long)fsn_round_up_sz(cv.off, 256);
    return FSN_OK;
}
extern "C" int fsn_debug_stream_pool_layout(const fsn_fullsubnet_cfg* cfg, long* out, int n) {
    if (check_cfg(cfg) != FSN_OK || !out || n < 21) return -1;
    const FsnPoolLayout L = pool_layout(cfg);
    for (int a = 0; a < 4; ++a) {
        out[a] = (long)L.fb[a];
        out[4 + a] = (long)L.sb[a];
    }
    const size_t rest[8] = {L.fb_sum, L.sb_sum, L.steps, L.in_tail, L.ola_tail, L.ring_re, L.ring_im, L.slot_bytes};
    for (int i = 0; i < 8; ++i) out[8 + i] = (long)rest[i];
    const int dims[5] = {L.F, L.FP, L.Hf, L.Hs, L.R};
    for (int i = 0; i < 5; ++i) out[16 + i] = dims[i];
    return FSN_OK;
}

// ---- recordings of any length: the model in segments of k frames, both norms --------------------------------------------
// The stream step's two halves as entries of their own, so that the offline norm - whose divisors are means over the whole
// recording - can run in three passes over the segments: (1) per-bin magnitude sums, (2) the full-band model, which needs
// the first divisor and yields the sum of its own output, (3) the sub-band model, which needs the second.  State: the
// stream step's blob (same layout, so a cumulative-norm cfg does here exactly what the stream step does) followed by the
// fp64 accumulators of the offline norm.
struct SegmentState {
    StreamState st;
    double *binsum, *fbsum;  // [B][FP] per-bin magnitude sums; [B] sums of the full-band output
};
static SegmentState segment_carve(Carver& cv, const fsn_fullsubnet_cfg* cfg, int B) {
    SegmentState g;
    g.st = stream_carve(cv, cfg, B);
    g.binsum = cv.take<double>((size_t)B * fsn_fpad(cfg->num_freqs));
    g.fbsum = cv.take<double>((size_t)B);
    return g;
}
static int check_segment(const fsn_fullsubnet_cfg* cfg, int B, int k) {
    FSN_TRY(check_cfg(cfg));
    FSN_REQUIRE(cfg->arith == FSN_ARITH_F32, "segments: only the fp32 arithmetic is built (arith %d)", cfg->arith);
    FSN_REQUIRE(B >= 1 && B <= 4096, "segments: batch %d out of range [1, 4096]", B);
    FSN_REQUIRE(k >= 1 && k <= 4096, "segments: frames %d out of range [1, 4096]", k);
    return FSN_OK;
}
extern "C" size_t fsn_fullsubnet_segment_state_bytes(const fsn_fullsubnet_cfg* cfg, int B) {
    if (check_segment(cfg, B, 1) != FSN_OK) return 0;
    Carver cv(nullptr);
    segment_carve(cv, cfg, B);
    return fsn_round_up_sz(cv.off, 256);
}
extern "C" size_t fsn_fullsubnet_segment_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int k) {
    if (check_segment(cfg, B, k) != FSN_OK) return 0;
    Carver cv(nullptr);
    stream_ws_carve(cv, cfg, B, k);  // one layout for both model passes: each uses its half of it
    return fsn_round_up_sz(cv.off, 256);
}
// what every segment entry checks about its state (and workspace, when it has one: workspace_bytes = 0 with ws = NULL)
static int check_segment_call(const fsn_fullsubnet_cfg* cfg, const void* state, size_t state_bytes, int B, int k,
                              const void* workspace, size_t workspace_bytes) {
    FSN_TRY(check_segment(cfg, B, k));
    FSN_REQUIRE(state, "segments: state is NULL");
    if (state_bytes < fsn_fullsubnet_segment_state_bytes(cfg, B) ||
        (workspace && workspace_bytes < fsn_fullsubnet_segment_workspace_bytes(cfg, B, k))) {
        fsn_set_error("segments: state / workspace buffer too small");
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}

extern "C" int fsn_fullsubnet_segment_stats(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, const float* mag,
                                            int B, int k, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, state, state_bytes, B, k, nullptr, 0));
    FSN_REQUIRE(mag, "NULL pointer argument");
    if (cfg->norm_type == FSN_NORM_CUMULATIVE_LAPLACE) return FSN_OK;  // causal: the model passes keep running sums
    Carver cs(state);
    const SegmentState g = segment_carve(cs, cfg, B);
    return fsn_launch_binsum_accumulate(mag, g.binsum, B, cfg->num_freqs, fsn_fpad(cfg->num_freqs), k,
                                        static_cast<hipStream_t>(stream));
}

extern "C" int fsn_fullsubnet_segment_divisors(const fsn_fullsubnet_cfg* cfg, const void* state, size_t state_bytes,
                                               const int* total_frames, int B, float* den_fb, float* den_sb, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_segment_call(cfg, state, state_bytes, B, 1, nullptr, 0));
    FSN_REQUIRE(cfg->norm_type == FSN_NORM_OFFLINE_LAPLACE, "segments: only the offline norm has per-recording divisors");
    FSN_REQUIRE(total_frames && den_fb && den_sb, "NULL pointer argument");
    Carver cs(const_cast<void*>(state));
    const SegmentState g = segment_carve(cs, cfg, B);
    return fsn_launch_segment_den(g.binsum, g.fbsum, total_frames, den_fb, den_sb, B, cfg->num_freqs, fsn_fpad(cfg->num_freqs),
                                  cfg->sb_num_neighbors, static_cast<hipStream_t>(stream));
}

extern "C" int fsn_fullsubnet_segment_fullband(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state,
                                               size_t state_bytes, int frames_done, const int* total_frames, const float* mag,
                                               int B, int k, float* fb_out, void* workspace, size_t workspace_bytes,
                                               void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(workspace, "NULL pointer argument");
    FSN_TRY(check_segment_call(cfg, state, state_bytes, B, k, workspace, workspace_bytes));
    const bool cum = cfg->norm_type == FSN_NORM_CUMULATIVE_LAPLACE;
    FSN_REQUIRE(packed && mag && fb_out && frames_done >= 0 && (cum || total_frames),
                "NULL pointer argument / negative frame count");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->num_freqs, FP = fsn_fpad(F);
    Carver cs(state), cw(workspace);
    const SegmentState g = segment_carve(cs, cfg, B);
    const StreamWs w = stream_ws_carve(cw, cfg, B, k);
    float* const fb[4] = {g.st.fb_h0, g.st.fb_h1, g.st.fb_c0, g.st.fb_c1};
    // [B, 1, F, k] -> frame-major [B][k][FP]
    FSN_TRY(fsn_launch_transpose(mag, w.magT, B, FP, k, k, (long)F * k, FP, (long)k * FP, F, k, s));
    if (cum)
        FSN_TRY(fsn_launch_cumulative_den_fb(w.magT, w.den_fb, B, k, F, FP, s, g.st.fb_sum, frames_done));
    else
        FSN_TRY(fsn_launch_segment_den(g.binsum, g.fbsum, total_frames, w.den_fb, nullptr, B, F, FP, cfg->sb_num_neighbors, s));
    FSN_TRY(stream_fullband(cfg, static_cast<const float*>(packed), w, fb, B, k, cum ? 1 : 0, s));
    if (!cum) FSN_TRY(fsn_launch_masked_sum_accumulate(w.fb_out, g.fbsum, total_frames, frames_done, B, k, FP, s));
    // frame-major [B][k][FP] -> [B, F, k]
    return fsn_launch_transpose(w.fb_out, fb_out, B, k, F, FP, (long)k * FP, k, (long)F * k, k, F, s);
}

extern "C" int fsn_fullsubnet_segment_subband(const fsn_fullsubnet_cfg* cfg, const void* packed, void* state,
                                              size_t state_bytes, int frames_done, const int* total_frames, const float* mag,
                                              const float* fb_out, int B, int k, float* crm_out, void* workspace,
                                              size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(workspace, "NULL pointer argument");
    FSN_TRY(check_segment_call(cfg, state, state_bytes, B, k, workspace, workspace_bytes));
    const bool cum = cfg->norm_type == FSN_NORM_CUMULATIVE_LAPLACE;
    FSN_REQUIRE(packed && mag && fb_out && crm_out && frames_done >= 0 && (cum || total_frames),
                "NULL pointer argument / negative frame count");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = cfg->num_freqs, FP = fsn_fpad(F), nb = cfg->sb_num_neighbors, Npad = fsn_round_up(B * F, 16);
    Carver cs(state), cw(workspace);
    const SegmentState g = segment_carve(cs, cfg, B);
    const StreamWs w = stream_ws_carve(cw, cfg, B, k);
    float* const sb[4] = {g.st.sb_h0, g.st.sb_h1, g.st.sb_c0, g.st.sb_c1};
    // [B, 1, F, k] and [B, F, k] -> frame-major [B][k][FP], padded bins zero
    FSN_TRY(fsn_launch_transpose(mag, w.magT, B, FP, k, k, (long)F * k, FP, (long)k * FP, F, k, s));
    FSN_TRY(fsn_launch_transpose(fb_out, w.fb_out, B, FP, k, k, (long)F * k, FP, (long)k * FP, F, k, s));
    if (cum)
        FSN_TRY(fsn_launch_cumulative_den_sb(w.magT, w.fb_out, w.den_sb, B, k, F, FP, nb, Npad, s, g.st.sb_sum, frames_done));
    else
        FSN_TRY(fsn_launch_segment_den(g.binsum, g.fbsum, total_frames, nullptr, w.den_sb, B, F, FP, nb, s));
    return stream_subband(cfg, static_cast<const float*>(packed), w, sb, B, k, cum ? 1 : 0, crm_out, s);
}

// ---- STFT / iSTFT boundary -------------------------------------------------------------------
static bool fast_fft(int n_fft, int hop) { return n_fft == 512 && hop == 256; }

// Streaming pool, frame analysis / synthesis for a list of sessions (fft_kernels.hip): 512 / 256 only, like fsn_enhance
static int check_pool_fft(const fsn_fullsubnet_cfg* cfg, int n_fft, int hop) {
    FSN_REQUIRE(fast_fft(n_fft, hop), "streaming pool: only n_fft = 512, hop = 256 is built (got %d/%d)", n_fft, hop);
    FSN_REQUIRE(cfg->num_freqs == n_fft / 2 + 1, "num_freqs %d != n_fft/2+1", cfg->num_freqs);
    return FSN_OK;
}
extern "C" int fsn_stream_pool_analysis(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                        const int* slots, int n, const float* hops, const float* prime,
                                        const int* frame_no, int n_fft, int hop, const float* window, float* mag,
                                        void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_pool_fft(cfg, n_fft, hop));
    FSN_REQUIRE(hops && frame_no && window && mag, "NULL pointer argument");
    return fsn_launch_pool_analysis(state, pool_layout(cfg), capacity, slots, n, hops, prime, frame_no, window, mag,
                                    static_cast<hipStream_t>(stream));
}
extern "C" int fsn_stream_pool_synthesis(const fsn_fullsubnet_cfg* cfg, void* state, size_t state_bytes, int capacity,
                                         const int* slots, int n, const float* crm, int k, const int* first_frame,
                                         const int* tail_samples, int n_fft, int hop, const float* window, float* out,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_pool_call(cfg, state, state_bytes, capacity, slots, n));
    FSN_TRY(check_pool_fft(cfg, n_fft, hop));
    FSN_REQUIRE(crm && first_frame && tail_samples && window && out && workspace, "NULL pointer argument");
    FSN_REQUIRE(k >= 1 && k <= 4096, "streaming pool: frames %d out of range", k);
    if (workspace_bytes < (size_t)n * k * n_fft * sizeof(float)) {
        fsn_set_error("streaming pool: synthesis workspace too small (n k n_fft floats)");
        return FSN_ERR_WORKSPACE;
    }
    return fsn_launch_pool_synthesis(state, pool_layout(cfg), capacity, slots, n, crm, k, first_frame, tail_samples, window,
                                     static_cast<float*>(workspace), out, static_cast<hipStream_t>(stream));
}

// fsn_enhance's fused path is built for the FullSubNet recipe's transform only
static int check_fft(int n_fft, int hop, int win_length) {
    FSN_REQUIRE(n_fft == 512 && hop == 256 && win_length == 512,
                "fsn_enhance: only n_fft = win_length = 512, hop = 256 is built (got %d/%d/%d)", n_fft, win_length, hop);
    return FSN_OK;
}

// fsn_stft / fsn_istft: 512 / 256 on the radix-8 kernels, any other even size / hop on the direct DFT
static int check_fft_generic(int n_fft, int hop, int win_length) {
    FSN_REQUIRE(win_length == n_fft, "win_length %d != n_fft %d is not built", win_length, n_fft);
    FSN_REQUIRE(n_fft >= 16 && n_fft <= 4096 && n_fft % 2 == 0, "n_fft %d: need an even size in [16, 4096]", n_fft);
    FSN_REQUIRE(hop >= 1 && hop <= n_fft, "hop %d out of range for n_fft %d", hop, n_fft);
    return FSN_OK;
}

extern "C" int fsn_stft(const float* y, int B, int L, int n_fft, int hop, int win_length, const float* window,
                        float* real, float* imag, float* mag, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_fft_generic(n_fft, hop, win_length));
    FSN_REQUIRE(y && window, "NULL pointer argument");
    FSN_REQUIRE(B >= 1 && L > n_fft / 2, "need B >= 1 and L > n_fft/2 (reflect padding), got B=%d L=%d", B, L);
    const int T = 1 + L / hop, F = n_fft / 2 + 1;
    FSN_REQUIRE((long)B * T <= 0x7fffffffL, "too many frames");
    if (!fast_fft(n_fft, hop))
        return fsn_launch_dft_stft(y, B, L, window, real, imag, mag, T, n_fft, hop, static_cast<hipStream_t>(stream));
    return fsn_launch_stft(y, B, L, window, real, imag, mag, T, T, F, fsn_fpad(F), false,
                           static_cast<hipStream_t>(stream));
}

extern "C" size_t fsn_istft_workspace_bytes(int B, int T, int n_fft) {
    if (B < 1 || T < 1 || n_fft < 16 || n_fft > 4096 || n_fft % 2) return 0;
    return fsn_round_up_sz((size_t)B * T * n_fft * sizeof(float), 256);
}

extern "C" int fsn_istft(const float* real, const float* imag, int B, int T, int n_fft, int hop, int win_length,
                         const float* window, int length, float* y, void* workspace, size_t workspace_bytes,
                         void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_fft_generic(n_fft, hop, win_length));
    FSN_TRY(check_bt(B, T));
    FSN_REQUIRE(real && imag && window && y && workspace, "NULL pointer argument");
    FSN_REQUIRE(length >= 1, "length %d < 1", length);
    if (workspace_bytes < fsn_istft_workspace_bytes(B, T, n_fft)) {
        fsn_set_error("workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = n_fft / 2 + 1;
    float* wf = static_cast<float*>(workspace);
    if (!fast_fft(n_fft, hop)) return fsn_launch_dft_istft(real, imag, window, wf, y, B, T, n_fft, hop, length, s);
    FSN_TRY(fsn_launch_mask_irfft(real, imag, nullptr, nullptr, B, T, F, fsn_fpad(F), false, window, wf, s));
    return fsn_launch_ola(wf, window, B, T, length, y, s);
}

// ragged batches in the reference layout: 512 / 256 only (the radix-8 kernels' lengths path)
extern "C" int fsn_stft_ragged(const float* y, const int* lengths, int B, int L_max, int n_fft, int hop, int win_length,
                               const float* window, float* real, float* imag, float* mag, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(fast_fft(n_fft, hop) && win_length == n_fft,
                "fsn_stft_ragged: only n_fft = win_length = 512, hop = 256 is built (got %d/%d/%d)", n_fft, win_length, hop);
    FSN_REQUIRE(y && lengths && window, "NULL pointer argument");
    FSN_REQUIRE(B >= 1 && L_max > n_fft / 2, "need B >= 1 and L_max > n_fft/2 (reflect padding), got B=%d L_max=%d", B, L_max);
    const int T = 1 + L_max / hop, F = n_fft / 2 + 1;
    FSN_REQUIRE((long)B * T <= 0x7fffffffL, "too many frames");
    return fsn_launch_stft(y, B, L_max, window, real, imag, mag, T, T, F, fsn_fpad(F), false, static_cast<hipStream_t>(stream),
                           lengths);
}

// ragged batches at every shape fsn_stft / fsn_istft take: 512 / 256 on the radix-8 kernels' lengths path, any other
// transform on the ragged forms of the direct-DFT kernels (improved_fullsubnet/model.py:550-557, 582-589: 512 / 128, 960 / 480)
extern "C" int fsn_stft_ragged_generic(const float* y, const int* lengths, int B, int L_max, int n_fft, int hop, int win_length,
                                       const float* window, float* real, float* imag, float* mag, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_fft_generic(n_fft, hop, win_length));
    FSN_REQUIRE(y && lengths && window, "NULL pointer argument");
    FSN_REQUIRE(B >= 1 && L_max > n_fft / 2, "need B >= 1 and L_max > n_fft/2 (reflect padding), got B=%d L_max=%d", B, L_max);
    const int T = 1 + L_max / hop, F = n_fft / 2 + 1;
    FSN_REQUIRE((long)B * T <= 0x7fffffffL, "too many frames");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!fast_fft(n_fft, hop)) return fsn_launch_dft_stft(y, B, L_max, window, real, imag, mag, T, n_fft, hop, s, lengths);
    return fsn_launch_stft(y, B, L_max, window, real, imag, mag, T, T, F, fsn_fpad(F), false, s, lengths);
}

extern "C" size_t fsn_istft_ragged_workspace_bytes(int B, int T, int n_fft) { return fsn_istft_workspace_bytes(B, T, n_fft); }

extern "C" int fsn_istft_ragged(const float* real, const float* imag, const int* lengths, int B, int T, int n_fft, int hop,
                                int win_length, const float* window, int length, float* y, void* workspace,
                                size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_TRY(check_fft_generic(n_fft, hop, win_length));
    FSN_TRY(check_bt(B, T));
    FSN_REQUIRE(real && imag && lengths && window && y && workspace, "NULL pointer argument");
    FSN_REQUIRE(length > n_fft / 2 && T == 1 + length / hop,
                "fsn_istft_ragged: need length > n_fft/2 and T = 1 + length / hop (got length %d, T %d)", length, T);
    if (workspace_bytes < fsn_istft_ragged_workspace_bytes(B, T, n_fft)) {
        fsn_set_error("workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int F = n_fft / 2 + 1;
    float* wf = static_cast<float*>(workspace);
    if (!fast_fft(n_fft, hop)) return fsn_launch_dft_istft(real, imag, window, wf, y, B, T, n_fft, hop, length, s, lengths);
    FSN_TRY(fsn_launch_mask_irfft(real, imag, nullptr, nullptr, B, T, F, fsn_fpad(F), false, window, wf, s, lengths));
    return fsn_launch_ola(wf, window, B, T, length, y, s, lengths);
}

extern "C" size_t fsn_mask_istft_workspace_bytes(int B, int T, int n_fft) {
    if (B < 1 || T < 1 || n_fft != 512) return 0;
    return fsn_istft_workspace_bytes(B, T, n_fft);
}

// inferencer.py:134-141 on a model's output: decompress_cIRM + complex mask + iSTFT, the [B][2][F][T] mask read in place
extern "C" int fsn_mask_istft(const float* crm, const float* real, const float* imag, const int* lengths, int B, int F, int T,
                              int n_fft, int hop, int win_length, const float* window, int length, float* y, void* workspace,
                              size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(fast_fft(n_fft, hop) && win_length == n_fft,
                "fsn_mask_istft: only n_fft = win_length = 512, hop = 256 is built (got %d/%d/%d)", n_fft, win_length, hop);
    FSN_TRY(check_bt(B, T));
    FSN_REQUIRE(F == n_fft / 2 + 1, "fsn_mask_istft: F = %d, need n_fft / 2 + 1 = %d", F, n_fft / 2 + 1);
    FSN_REQUIRE(crm && real && imag && window && y && workspace, "NULL pointer argument");
    FSN_REQUIRE(length >= 1, "length %d < 1", length);
    FSN_REQUIRE(!lengths || (length > n_fft / 2 && T == 1 + length / hop),
                "fsn_mask_istft: with lengths, need length > n_fft/2 and T = 1 + length / hop (got length %d, T %d)", length, T);
    if (workspace_bytes < fsn_mask_istft_workspace_bytes(B, T, n_fft)) {
        fsn_set_error("workspace too small");
        return FSN_ERR_WORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* wf = static_cast<float*>(workspace);
    FSN_TRY(fsn_launch_mask_irfft(real, imag, crm, crm + (size_t)F * T, B, T, F, fsn_fpad(F), false, window, wf, s, lengths,
                                  2L * F * T));
    return fsn_launch_ola(wf, window, B, T, length, y, s, lengths);
}

// ---- elementwise boundary --------------------------------------------------------------------
extern "C" int fsn_decompress_cirm(const float* mask, float* out, size_t n, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(mask && out, "NULL pointer argument");
    return n ? fsn_launch_decompress(mask, out, n, static_cast<hipStream_t>(stream)) : FSN_OK;
}
extern "C" int fsn_compress_cirm(const float* mask, float* out, size_t n, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(mask && out, "NULL pointer argument");
    return n ? fsn_launch_compress(mask, out, n, static_cast<hipStream_t>(stream)) : FSN_OK;
}
extern "C" int fsn_build_cirm(const float* nr, const float* ni, const float* cr, const float* ci, float* out,
                              size_t n, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(nr && ni && cr && ci && out, "NULL pointer argument");
    return n ? fsn_launch_build_cirm(nr, ni, cr, ci, out, n, static_cast<hipStream_t>(stream)) : FSN_OK;
}

// ---- the whole path: inferencer.py:130-145 ---------------------------------------------------
extern "C" size_t fsn_enhance_workspace_bytes(const fsn_fullsubnet_cfg* cfg, int B, int L, int n_fft, int hop) {
    if (check_cfg(cfg) != FSN_OK || check_fft(n_fft, hop, n_fft) != FSN_OK || B < 1 || L <= n_fft / 2) return 0;
    const int T = 1 + L / hop;
    if (check_bt(B, T) != FSN_OK || cfg->num_freqs != n_fft / 2 + 1) return 0;
    const CoreDims d = core_dims(cfg, B, T);
    Carver cv(nullptr);
    cv.take<float>((size_t)B * d.Tp * d.FP);  // magT
    cv.take<float>((size_t)B * d.T * d.FP);   // re
    cv.take<float>((size_t)B * d.T * d.FP);   // im
    cv.take<float>((size_t)B * d.T * d.FP);   // crm_r
    cv.take<float>((size_t)B * d.T * d.FP);   // crm_i
    cv.take<float>((size_t)B * d.T * n_fft);  // windowed frames
    Carver whole(nullptr), parts(nullptr);
    core_carve(whole, d, cfg->norm_type);
    core_carve_chunks(parts, cfg, B, T);
    cv.take<char>(whole.off > parts.off ? whole.off : parts.off);
    return fsn_round_up_sz(cv.off, 256);
}

// fsn_enhance and fsn_enhance_ragged: lengths == NULL is the rectangular batch
static int enhance(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* window, const float* noisy,
                   const int* lengths, int B, int L, int n_fft, int hop, float* enhanced, float* crm_out, void* workspace,
                   size_t workspace_bytes, hipStream_t s) {
    FSN_TRY(check_cfg(cfg));
    FSN_TRY(check_fft(n_fft, hop, n_fft));
    FSN_REQUIRE(packed && window && noisy && enhanced && workspace, "NULL pointer argument");
    FSN_REQUIRE(B >= 1 && L > n_fft / 2, "need B >= 1 and L > n_fft/2, got B=%d L=%d", B, L);
    FSN_REQUIRE(cfg->num_freqs == n_fft / 2 + 1, "num_freqs %d != n_fft/2+1", cfg->num_freqs);
    const int T = 1 + L / hop;
    FSN_TRY(check_bt(B, T));
    const size_t need = fsn_enhance_workspace_bytes(cfg, B, L, n_fft, hop);
    if (workspace_bytes < need) {
        fsn_set_error("workspace too small: %zu < %zu bytes", workspace_bytes, need);
        return FSN_ERR_WORKSPACE;
    }
    const CoreDims d = core_dims(cfg, B, T);
    Carver cv(workspace);
    float* magT = cv.take<float>((size_t)B * d.Tp * d.FP);
    float* re = cv.take<float>((size_t)B * d.T * d.FP);
    float* im = cv.take<float>((size_t)B * d.T * d.FP);
    float* crm_r = cv.take<float>((size_t)B * d.T * d.FP);
    float* crm_i = cv.take<float>((size_t)B * d.T * d.FP);
    float* wf = cv.take<float>((size_t)B * d.T * n_fft);
    void* scratch = cv.take<char>(0);  // the rest: the core's scratch (fsn_enhance_workspace_bytes)
    prof_reset();
    {
        StageTimer st(ST_STFT, s);
        FSN_TRY(fsn_launch_stft(noisy, B, L, window, re, im, magT, d.T, d.Tp, d.F, d.FP, true, s, lengths));
    }
    FSN_TRY(run_core_chunks(cfg, static_cast<const float*>(packed), magT, B, T, scratch, crm_r, crm_i, s, lengths));
    {
        StageTimer st(ST_MASK_ISTFT, s);
        FSN_TRY(fsn_launch_mask_irfft(re, im, crm_r, crm_i, B, d.T, d.F, d.FP, true, window, wf, s, lengths));
        FSN_TRY(fsn_launch_ola(wf, window, B, d.T, L, enhanced, s, lengths));
    }
    if (crm_out) {
        FSN_TRY(fsn_launch_transpose(crm_r, crm_out, B, d.T, d.F, d.FP, (long)d.T * d.FP, d.T, 2L * d.F * d.T, d.T,
                                     d.F, s, lengths));
        FSN_TRY(fsn_launch_transpose(crm_i, crm_out + (size_t)d.F * d.T, B, d.T, d.F, d.FP, (long)d.T * d.FP, d.T,
                                     2L * d.F * d.T, d.T, d.F, s, lengths));
    }
    return FSN_OK;
}

extern "C" int fsn_enhance(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* window,
                           const float* noisy, int B, int L, int n_fft, int hop, float* enhanced, float* crm_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    CallScope scope(stream);
    return enhance(cfg, packed, window, noisy, nullptr, B, L, n_fft, hop, enhanced, crm_out, workspace, workspace_bytes,
                   static_cast<hipStream_t>(stream));
}

extern "C" int fsn_enhance_ragged(const fsn_fullsubnet_cfg* cfg, const void* packed, const float* window,
                                  const float* noisy, const int* lengths, int B, int L_max, int n_fft, int hop,
                                  float* enhanced, float* crm_out, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(lengths, "NULL pointer argument");
    return enhance(cfg, packed, window, noisy, lengths, B, L_max, n_fft, hop, enhanced, crm_out, workspace,
                   workspace_bytes, static_cast<hipStream_t>(stream));
}
