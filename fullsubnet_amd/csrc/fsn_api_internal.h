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
int aux_init(StreamCtx* c);    // the record's auxiliary stream and fork / join events, created on first use
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

// ---- FullSubNet model (fsn_api_fullsubnet.hip) ----------------------------------------------------------------------
// below this many sub-band row tiles (batch <= 5) the two layers of the small-batch step path run as a wavefront of
// per-step launches; from here up to the persistent regime (160 tiles) they run on the group kernel
constexpr int kWavefrontBelowTiles = 96;
// One LSTM layer of Npad rows over all Tp steps on the plan `r`: the persistent kernel on `s`, the left-over row tiles
// step by step beside it (see the definition).
int run_recurrence(const float* gx, const FsnSbInput* xin, const float* gx_left, long left_stride, long left_off,
                   const float* whh, float* hseq, float* c_left, int Tp, int Npad, int H, const FsnRecPlan& r, hipStream_t s,
                   const FsnRecFc* fc = nullptr, long left_hs_stride = -1, const void* whh_f16x3 = nullptr,
                   const void* wih_f16x3 = nullptr, const float* x_main = nullptr, const float* wih_main = nullptr,
                   const float* bias_main = nullptr, float* hseq_left = nullptr);

// ---- stand-alone LSTM layers (fsn_api_layers.hip) -------------------------------------------------------------------
int check_lstm_layer(int T, int N, int I, int H, long ldx);
bool lstm2_on_chain(int T, int N, int H);  // two stacked layers of N rows that the full-band chain kernel takes
