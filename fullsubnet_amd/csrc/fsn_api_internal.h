// Host-side names shared by the files of the C ABI (fsn_api*.hip); kernel sources do not include this header.
// Everything else of those files is static to its file.  libfsn_hip.so exports only the fsn_* entries of
// include/fsn_hip.h (fsn_exports.map).
#pragma once

#include <mutex>
#include <vector>

#include "fsn_common.h"

#define FSN_TRY(x)                \
    do {                          \
        const int _rc = (x);      \
        if (_rc != FSN_OK) return _rc; \
    } while (0)

// ---- runtime (fsn_api.hip) ------------------------------------------------------------------------------------------
// per-stage profiler
enum Stage {
    ST_STFT = 0,
    ST_NORM,
    ST_FB_GEMM,
    ST_FB_REC,
    ST_SB_GEMM_L0,
    ST_SB_REC_L0,
    ST_SB_GEMM_L1,
    ST_SB_REC_L1,
    ST_SB_FC,
    ST_MASK_ISTFT,
    ST_COUNT
};
constexpr int kMaxSpans = 4;  // a stage may be entered several times per call (once per layer)

// ---- per-(device, caller stream) state ---------------------------------------------------------------
// Everything a call needs beyond its arguments.  Two caller streams (or two devices, or two host threads that
// each drive their own stream) never see each other's events; calls that share ONE stream must be issued
// from one thread at a time, like any stream-ordered API.
struct StreamCtx {
    int dev = 0;
    hipStream_t aux = nullptr;           // left-over sub-band tiles beside the persistent kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool prof_on = false;                // per-stage profiler requested for this stream (fsn_profile_enable_stream)
    bool prof_events = false;            // profiler events exist
    hipEvent_t ev[ST_COUNT][kMaxSpans][2];
    int spans[ST_COUNT] = {0};
    // sticky status record of the persistent kernels launched on this stream: pinned host memory the device writes
    // ({status word of the first launch that ran out of time, number of such launches}); NULL until first needed
    unsigned* sticky_host = nullptr;
    unsigned* sticky_dev = nullptr;
    // fsn_stream_timeout_policy: a raised record does not refuse later persistent launches on this stream (a training
    // step in flight: NaN poison + the optimizer's skip contain the damage; the caller looks at the end of the step)
    bool timeout_defer = false;
};
StreamCtx* cur_ctx();          // the record of the running call's (device, stream), set up by CallScope
// Work beside the running call's stream `s`: fork hands out the record's auxiliary stream (created on first use), ordered
// behind everything issued on `s` so far; join orders `s` behind everything issued on the auxiliary stream since.
int aux_fork(hipStream_t s, hipStream_t* aux);
int aux_join(hipStream_t s);
typedef FsnCallScope CallScope;

// Times one stage of the running call on `stream` when the profiler is on for it (fsn_profile_enable).
struct StageTimer {
    int st, span;
    hipStream_t s;
    StreamCtx* c;
    StageTimer(int stage, hipStream_t stream);
    ~StageTimer();
};
void prof_reset();  // a new profiled call: forget the spans of the last one

// Residency gate of the persistent kernels (see fsn_api.hip): an entry that launches one opens
// FSN_PERSIST_BEGIN(stream) in the scope of that launch.
struct PersistEntry {
    hipEvent_t ev;
    hipStream_t stream;
    double frac;  // grid / (occ x CUs)
    int occ;
};
struct PersistGate;
class PersistLaunch {
  public:
    explicit PersistLaunch(hipStream_t s);
    void admit(double frac, int occ);  // the launcher's report, right before its launch (fsn_persist_admit)
    ~PersistLaunch();
    PersistLaunch(const PersistLaunch&) = delete;
    PersistLaunch& operator=(const PersistLaunch&) = delete;

  private:
    hipStream_t s_;
    std::unique_lock<std::mutex> lock_;
    PersistGate* gate_ = nullptr;
    std::vector<hipEvent_t>* pool_ = nullptr;  // where events come from: the device's pool (a capture's gate has none of its own)
    PersistEntry me_{};
    bool admitted_ = false;
};
int persist_precheck();  // FSN_ERR_TIMEOUT while the stream's sticky record is raised (fsn_stream_status)
#define FSN_PERSIST_BEGIN(s)        \
    FSN_TRY(persist_precheck());    \
    PersistLaunch gate(s)

// ---- workspace carving -----------------------------------------------------------------------
struct Carver {
    char* base;
    size_t off;
    explicit Carver(void* p) : base(static_cast<char*>(p)), off(0) {}
    template <class T>
    T* take(size_t count) {
        off = fsn_round_up_sz(off, 256);
        T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return r;
    }
};

// ---- descriptor builders ---------------------------------------------------------------------
// One per descriptor kind (fsn_common.h).  Each starts from {} and sets only what its kind reads: every other field is zero.
struct ModelGeom {  // the planes of one FullSubNet call: [B][Tp][FP] inputs, [B][T][FP] masks
    int B, Tp, T, F, FP, nb, la;
};
// A operand, kind 0: a row-major matrix (n_valid: the valid rows, for the launches whose last row tile is partial)
inline FsnGemmA gemm_a_rows(const float* p, long ld, int n_valid = 0) {
    FsnGemmA a{};
    a.kind = 0;
    a.p0 = p;
    a.ld = ld;
    a.N = n_valid;
    return a;
}
// kind 1: the full-band model's input, mag / den, Npad rows per step
inline FsnGemmA gemm_a_fullband(const ModelGeom& g, const float* mag, const float* den, int den_mode, int Npad) {
    FsnGemmA a{};
    a.kind = 1;
    a.p0 = mag;
    a.den = den;
    a.den_mode = den_mode;
    a.B = g.B;
    a.Tp = g.Tp;
    a.F = g.F;
    a.FP = g.FP;
    a.Npad = Npad;
    return a;
}
// kind 2: the sub-band model's input `x` (model form) for Npad rows per step from GLOBAL row `first_row` on; rows from
// x.row0 + x.N on are padding
inline FsnGemmA gemm_a_subband(const FsnSbInput& x, long first_row, int Npad) {
    FsnGemmA a{};
    a.kind = 2;
    a.p0 = x.mag;
    a.p1 = x.fb_out;
    a.den = x.den;
    a.den_mode = x.den_mode;
    a.den_stride = x.den_stride;
    a.B = x.B;
    a.Tp = x.Tp;
    a.F = x.F;
    a.FP = x.FP;
    a.Npad = Npad;
    a.n_offset = (int)first_row;
    a.N = (int)(x.row0 + x.N);
    a.nb = x.nb;
    return a;
}
// C store, kind 0: accumulator-fragment order + bias (the projection tiles the recurrent kernels read)
inline FsnGemmC gemm_c_frag(float* p, const float* bias) {
    FsnGemmC c{};
    c.kind = 0;
    c.p0 = p;
    c.bias = bias;
    return c;
}
// kind 1: rows of fb_out [B][Tp][FP] (bias + ReLU) from Npad rows per step
inline FsnGemmC gemm_c_fb_out(const ModelGeom& g, float* fb_out, const float* bias, int Npad) {
    FsnGemmC c{};
    c.kind = 1;
    c.p0 = fb_out;
    c.bias = bias;
    c.B = g.B;
    c.Tp = g.Tp;
    c.F = g.F;
    c.FP = g.FP;
    c.Npad = Npad;
    return c;
}
// kind 2: the two mask planes [B][T][FP]; row r of the product is step r / Npad, GLOBAL row first_row + r % Npad, rows
// from row_limit on are padding
inline FsnGemmC gemm_c_masks(const ModelGeom& g, float* crm_r, float* crm_i, const float* bias, int Npad, long first_row,
                             long row_limit) {
    FsnGemmC c{};
    c.kind = 2;
    c.p0 = crm_r;
    c.p1 = crm_i;
    c.bias = bias;
    c.T = g.T;
    c.F = g.F;
    c.FP = g.FP;
    c.Npad = Npad;
    c.N = (int)row_limit;
    c.n_off = (int)first_row;
    c.la = g.la;
    return c;
}
// kind 3: plain rows [rows][ld], `cols` valid columns (+ bias, + ReLU when given)
inline FsnGemmC gemm_c_rows(float* p, long ld, int rows, int cols, const float* bias = nullptr, bool relu = false) {
    FsnGemmC c{};
    c.kind = 3;
    c.p0 = p;
    c.bias = bias;
    c.ld = ld;
    c.rows = rows;
    c.cols = cols;
    c.la = relu ? 1 : 0;  // kind 3: la doubles as the ReLU flag
    return c;
}
// the sub-band model's layer-0 input, model form: local rows [0, N) are rows row0 .. of the flattened (b, f) space
inline FsnSbInput sb_input_model(const ModelGeom& g, const float* mag, const float* fb_out, const float* den, int den_mode,
                                 int den_stride, const float* wih_p, const float* bias, int kin_chunks, int N, long row0) {
    FsnSbInput x{};
    x.mag = mag;
    x.fb_out = fb_out;
    x.den = den;
    x.wih_p = wih_p;
    x.bias = bias;
    x.den_mode = den_mode;
    x.den_stride = den_stride;
    x.row0 = row0;
    x.B = g.B;
    x.Tp = g.Tp;
    x.F = g.F;
    x.FP = g.FP;
    x.N = N;
    x.nb = g.nb;
    x.kin_chunks = kin_chunks;
    return x;
}
// ... x_rows form: N valid rows of a plain row-major input, element (t, n, c) at x[(t * step + n) * ld + c]
inline FsnSbInput sb_input_rows(const float* x_rows, long ld, long step, int N, int kin_chunks, const float* wih_p,
                                const float* bias) {
    FsnSbInput x{};
    x.x_rows = x_rows;
    x.x_ld = ld;
    x.x_step = step;
    x.N = N;
    x.kin_chunks = kin_chunks;
    x.wih_p = wih_p;
    x.bias = bias;
    return x;
}
// the output layer fused into a persistent kernel: the two outputs of local row n (N valid ones, global row n + row0 of
// groups of F rows) go to the planes crm_r / crm_i [..][T][FP], `la` look-ahead steps dropped
inline FsnRecFc rec_fc(const float* w_p, const float* bias, float* crm_r, float* crm_i, int N, long row0, int F, int FP, int T,
                       int la) {
    FsnRecFc fc{};
    fc.w_p = w_p;
    fc.bias = bias;
    fc.crm_r = crm_r;
    fc.crm_i = crm_i;
    fc.N = N;
    fc.row0 = row0;
    fc.F = F;
    fc.FP = FP;
    fc.T = T;
    fc.la = la;
    return fc;
}

// ---- FullSubNet model (fsn_api_fullsubnet.hip) ----------------------------------------------------------------------
// below this many sub-band row tiles (batch <= 5) the two layers of the small-batch step path run as a wavefront of
// per-step launches; from here up to the persistent regime (160 tiles) they run on the group kernel
constexpr int kWavefrontBelowTiles = 96;
// One LSTM layer of Npad rows over all Tp steps on the plan `plan`: the persistent kernel on `s` and, concurrently, the
// few left-over row tiles as per-step launches on the auxiliary stream.
struct RecArgs {
    // Main kernel: input projection either precomputed (`gx`, tile (t, i) at t * tiles + i) or built in-kernel from `xin`.
    const float* gx = nullptr;
    const FsnSbInput* xin = nullptr;
    // Left-over tiles: projection tiles in `gx_left` at t * left_stride + left_off + i.
    const float* gx_left = nullptr;
    long left_stride = 0, left_off = 0;
    const float* whh = nullptr;
    float* hseq = nullptr;
    float* c_left = nullptr;
    int Tp = 0, Npad = 0, H = 0;
    FsnRecPlan plan{};
    const FsnRecFc* fc = nullptr;
    // >= 0: the persistent part stores nothing (fused output layer) and the left-over rows' hidden sequence in `hseq` is a
    // compact [t][left_hs_stride rows][H] matrix instead of rows [main rows, Npad) of the full [t][Npad] one
    long left_hs_stride = -1;
    const void* whh_f16x3 = nullptr;
    const void* wih_f16x3 = nullptr;
    // x_main (with wih_main, bias_main): the main rows run on lstm_rec_x_kernel, which reads the hidden sequence of the
    // layer below (x_main [Tp][Npad][H]) and forms its input projection itself.
    const float* x_main = nullptr;
    const float* wih_main = nullptr;
    const float* bias_main = nullptr;
    // hseq_left: the left-over rows' hidden sequence goes to this compact [t][left rows][H] buffer instead of rows
    // [main rows, Npad) of hseq.
    float* hseq_left = nullptr;
};
int run_recurrence(const RecArgs& a, hipStream_t s);

// ---- stand-alone LSTM layers (fsn_api_layers.hip) -------------------------------------------------------------------
int check_lstm_layer(int T, int N, int I, int H, long ldx);
bool lstm2_on_chain(int T, int N, int H);  // two stacked layers of N rows that the full-band chain kernel takes
// Rows [row0, row0 + left) of every step of src [T][N] rows of `ld` floats, their first K columns, into the compact
// dst [T][left][K] (one 2-D copy when the rows are exactly K wide, one per step otherwise); and the inverse.
int gather_step_rows(float* dst, const float* src, long ld, int T, int N, int row0, int left, int K, hipStream_t s);
int scatter_step_rows(float* dst, long ld, const float* src, int T, int N, int row0, int left, int K, hipStream_t s);
// the blob of fsn_lstm_layer_pack: W_ih and W_hh as MFMA fragments, b_ih + b_hh
struct LayerPacked {
    size_t wih, whh, bias, total;  // float offsets
};
inline LayerPacked layer_packed_layout(int I, int H) {
    LayerPacked p;
    const size_t Ipad = fsn_round_up(I, 16);
    p.wih = 0;
    p.whh = fsn_round_up_sz(4 * (size_t)H * Ipad, 64);
    p.bias = p.whh + fsn_round_up_sz(4 * (size_t)H * H, 64);
    p.total = p.bias + fsn_round_up_sz(4 * (size_t)H, 64);
    return p;
}
