// C ABI of libfsn_hip.so (see include/fsn_hip.h), runtime part: errors, the per-stream state, the residency gate
// of the persistent kernels, the profiler and the status / debug entries.  The entries that enqueue model work
// live beside it: fsn_api_fullsubnet.hip (the FullSubNet model and the enhancement path), fsn_api_layers.hip
// (stand-alone LSTM layers and stacks), fsn_api_gru.hip (GRU layers) and fsn_api_train.hip (training).
// No allocation and no host synchronisation on the hot path.  The only state the library owns is a small
// per-(device, caller stream) record - an auxiliary stream with its fork / join events for the left-over sub-band
// tiles and the events of the optional per-stage profiler - created on first use and never shared between two
// caller streams or two devices.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <utility>

#include "fsn_api_internal.h"

// ---- errors ---------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void fsn_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int fsn_check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fsn_set_error("%s: %s", what, hipGetErrorString(e));
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}
extern "C" const char* fsn_last_error(void) { return g_err; }
extern "C" int fsn_version(void) { return FSN_ABI_VERSION; }

// ---- per-stage profiler ----------------------------------------------------------------------
static const char* kStageNames[ST_COUNT] = {"stft",       "norm",       "fb_gemm",    "fb_rec", "sb_gemm_l0",
                                            "sb_rec_l0",  "sb_gemm_l1", "sb_rec_l1",  "sb_fc",  "mask_istft"};

// ---- per-(device, caller stream) state (StreamCtx) and the residency gate -------------------------------------------
static std::mutex g_ctx_mutex;
static std::map<std::pair<int, hipStream_t>, StreamCtx*> g_ctx;
static std::atomic<int> g_persist_mode{0};          // fsn_set_persistent_mode: 0 auto, 1 never
static std::atomic<int> g_persist_timeout_ms{20000};  // fsn_set_persistent_timeout_ms

// Persistent kernels whose workgroups wait for each other (the group kernel, the full-band chain) need ALL their
// workgroups resident at once.  Two of them launched from different streams could each take a part of the chip and wait
// for the rest until the spin bound.  So these launches are admitted against a residency budget per device: every
// launcher reports its kernel's footprint (fsn_persist_admit: grid, resident workgroups per CU by the occupancy API)
// right before the launch, and the launch waits for the completion events of earlier persistent launches on OTHER
// streams, oldest first, until the set that may run beside it is provably placeable whatever order the dispatcher
// hands out workgroups in:
//   a CU holding a_j workgroups of kernel j is "used" u = sum_j a_j / occ_j in the model (occ_j = resident workgroups
//   per CU of kernel j alone; the model is conservative: where it has room for a workgroup, the hardware has);
//   a workgroup of kernel k finds no CU only if EVERY CU has u > 1 - 1 / occ_k, i.e. u >= umin(k), the smallest sum of
//   the set's workgroup sizes above that threshold; all CUs together then hold >= CUs x umin(k), while the kernels of
//   the set can place at most sum_j grid_j / occ_j = CUs x sum_j frac_j.  Hence: admitted iff sum_j frac_j < umin(k)
//   for every k of the set.
// One kernel alone is always admitted (its own grid was checked against occ x CUs at plan time).  Examples on 256 CUs:
// two chain launches of H = 384 with two row tiles (192 workgroups, 2 per CU each) run side by side, a third waits; two
// group launches of 28 clusters (448 workgroups, 2 per CU) do not.  Nothing else of the streams is ordered.
// Under stream capture (round 6) the same rule orders the persistent launches of ONE capture among themselves, through
// captured event edges: a graph's replay runs the captured streams' kernels side by side exactly as far as the edges allow, and
// a call with several persistent launches on side streams (Improved FullSubNet's band sections at a few utterances: chain
// launches of one workgroup per CU) replayed without them stalled or ran out of time in ~1 % of the replays
// (tools/diag_stall.py).  Nothing can be retired during a capture: every earlier launch of the capture counts as live.  The
// replays of DIFFERENT graphs (and eager calls beside them) are ordered by whoever launches them.
struct PersistGate {
    std::vector<PersistEntry> live;
    std::vector<hipEvent_t> pool;
};
static std::mutex g_persist_mutex;
static std::map<int, PersistGate> g_persist;
static std::map<std::pair<int, unsigned long long>, PersistGate> g_persist_capture;  // (device, capture id) -> the capture's launches
// umin(k) in units of 1 / 840 (= lcm(1 .. 8); occupancies above 8 count as 8, which only makes workgroups larger)
static int persist_umin(const std::vector<int>& occs, int occ_k) {
    bool reach[841] = {};
    reach[0] = true;
    for (int o : occs) {
        const int sz = 840 / o;
        for (int u = sz; u <= 840; ++u)
            if (reach[u - sz]) reach[u] = true;  // unbounded multiples, ascending
    }
    for (int u = 840 - 840 / occ_k + 1; u <= 840; ++u)
        if (reach[u]) return u;
    return 1 << 20;  // no CU state blocks kernel k
}
static bool persist_set_fits(const std::vector<const PersistEntry*>& set) {
    std::vector<int> occs;
    double sum = 0.0;
    for (const PersistEntry* e : set) {
        occs.push_back(e->occ);
        sum += e->frac;
    }
    for (const PersistEntry* e : set)
        if (!(sum * 840.0 < (double)persist_umin(occs, e->occ))) return false;
    return true;
}
static thread_local PersistLaunch* t_persist = nullptr;
static std::atomic<unsigned> g_persist_launches{0}, g_persist_waits{0}, g_persist_unreported{0};
PersistLaunch::PersistLaunch(hipStream_t s) : s_(s), lock_(g_persist_mutex) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    unsigned long long cap_id = 0;
    if (hipStreamGetCaptureInfo(s, &cap, &cap_id) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (cap == hipStreamCaptureStatusActive) {
        // the capture's own gate: its launches, ordered by captured event edges; events come from (and return to) the
        // device's pool; the gates of finished captures are dropped once a few newer ones exist
        pool_ = &g_persist[dev].pool;
        const std::pair<int, unsigned long long> key(dev, cap_id);
        if (!g_persist_capture.count(key)) {
            while (g_persist_capture.size() >= 4) {
                auto old = g_persist_capture.begin();  // smallest (device, id): an earlier capture
                if (old->first.first == dev)
                    for (PersistEntry& e : old->second.live) g_persist[dev].pool.push_back(e.ev);
                g_persist_capture.erase(old);
            }
        }
        gate_ = &g_persist_capture[key];
        t_persist = this;
        return;
    }
    if (cap != hipStreamCaptureStatusNone) return;  // an invalidated capture: nothing to order
    gate_ = &g_persist[dev];
    pool_ = &gate_->pool;
    // retire what has completed
    std::vector<PersistEntry>& live = gate_->live;
    for (size_t i = 0; i < live.size();) {
        if (hipEventQuery(live[i].ev) == hipSuccess) {
            gate_->pool.push_back(live[i].ev);
            live.erase(live.begin() + (long)i);
        } else {
            (void)hipGetLastError();
            ++i;
        }
    }
    t_persist = this;
}
void PersistLaunch::admit(double frac, int occ) {
    if (!gate_) return;
    me_.frac = frac;
    me_.occ = occ < 1 ? 1 : occ > 8 ? 8 : occ;
    admitted_ = true;
    std::vector<const PersistEntry*> set;
    for (const PersistEntry& e : gate_->live)
        if (e.stream != s_) set.push_back(&e);  // same stream: ordered anyway
    set.push_back(&me_);
    while (set.size() > 1 && !persist_set_fits(set)) {
        (void)hipStreamWaitEvent(s_, set.front()->ev, 0);  // oldest first
        set.erase(set.begin());
        g_persist_waits.fetch_add(1, std::memory_order_relaxed);
    }
    g_persist_launches.fetch_add(1, std::memory_order_relaxed);
}
PersistLaunch::~PersistLaunch() {
    t_persist = nullptr;
    if (!gate_) return;
    hipEvent_t ev = nullptr;
    const bool capturing = pool_ != &gate_->pool;
    if (!pool_->empty()) {
        ev = pool_->back();
        pool_->pop_back();
    } else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (!capturing) (void)hipStreamSynchronize(s_);  // no event to order later launches by: drain instead
        return;
    }
    if (hipEventRecord(ev, s_) != hipSuccess) {
        (void)hipGetLastError();
        pool_->push_back(ev);
        if (!capturing) (void)hipStreamSynchronize(s_);
        return;
    }
    me_.ev = ev;
    me_.stream = s_;
    if (!admitted_) {  // a launcher that did not report (a bug, counted): treated as filling the chip from now on
        me_.frac = 1.0;
        me_.occ = 1;
        g_persist_unreported.fetch_add(1, std::memory_order_relaxed);
    }
    gate_->live.push_back(me_);
}

// What the running call works on (set by CallScope for the duration of one entry point on this host thread).
static thread_local StreamCtx* t_ctx = nullptr;
static thread_local hipStream_t t_stream = nullptr;
static thread_local int t_dev = 0;
static thread_local unsigned t_launch_trace = 0;  // FsnTraceBit mask of the running (or last) call on this thread
void fsn_trace(unsigned bit) { t_launch_trace |= bit; }

static StreamCtx* ctx_lookup(int dev, hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_ctx_mutex);
    StreamCtx*& c = g_ctx[std::make_pair(dev, s)];
    if (!c) {
        c = new StreamCtx();
        c->dev = dev;
    }
    return c;
}
StreamCtx* cur_ctx() {
    if (!t_ctx) t_ctx = ctx_lookup(t_dev, t_stream);
    return t_ctx;
}

// Every entry point that enqueues work opens one of these: the device the caller's stream belongs to becomes
// the current device for the duration of the call (restored afterwards), so that a process that drives several
// GPUs needs no device bookkeeping around the C ABI, and the per-stream record is resolved lazily.
FsnCallScope::FsnCallScope(void* stream) : prev(-1), switched(false) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    int cur = 0;
    (void)hipGetDevice(&cur);
    hipDevice_t sd = cur;
    if (s && hipStreamGetDevice(s, &sd) != hipSuccess) {
        (void)hipGetLastError();
        sd = cur;
    }
    if ((int)sd != cur && hipSetDevice((int)sd) == hipSuccess) {
        prev = cur;
        switched = true;
    }
    t_dev = (int)sd;
    t_stream = s;
    t_ctx = nullptr;
    t_launch_trace = 0;
}
FsnCallScope::~FsnCallScope() {
    t_ctx = nullptr;
    if (switched) (void)hipSetDevice(prev);
}

StageTimer::StageTimer(int stage, hipStream_t stream) : st(stage), span(-1), s(stream), c(nullptr) {
    c = cur_ctx();
    if (!c->prof_on) {
        c = nullptr;
        return;
    }
    if (!c->prof_events) {
        for (int i = 0; i < ST_COUNT; ++i)
            for (int j = 0; j < kMaxSpans; ++j) {
                (void)hipEventCreate(&c->ev[i][j][0]);
                (void)hipEventCreate(&c->ev[i][j][1]);
            }
        c->prof_events = true;
    }
    if (c->spans[st] >= kMaxSpans) return;
    span = c->spans[st];
    (void)hipEventRecord(c->ev[st][span][0], s);
}
StageTimer::~StageTimer() {
    if (span < 0) return;
    (void)hipEventRecord(c->ev[st][span][1], s);
    c->spans[st] = span + 1;
}
void prof_reset() {
    StreamCtx* c = cur_ctx();
    if (!c->prof_on) return;
    for (int i = 0; i < ST_COUNT; ++i) c->spans[i] = 0;
}

// ---- residency contract of the persistent kernels (fsn_common.h) -------------------------------------------------
bool fsn_persistent_allowed() { return g_persist_mode.load(std::memory_order_relaxed) == 0; }
unsigned long long fsn_spin_ticks() {
    int khz = 0, dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        khz = 100000;  // gfx9: the constant-rate counter runs at 100 MHz
    }
    return (unsigned long long)g_persist_timeout_ms.load(std::memory_order_relaxed) * (unsigned long long)khz;
}
// resident workgroups per CU of `kernel` alone (occupancy API, cached per device); 0 on failure
static int persist_occupancy(const void* kernel, int block_threads, int* cus_out) {
    static std::mutex m;
    static std::map<std::pair<const void*, int>, int> per_cu;  // (kernel, device) -> resident workgroups per CU
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    if (cus_out) *cus_out = cus;
    std::lock_guard<std::mutex> lock(m);
    auto it = per_cu.find(std::make_pair(kernel, dev));
    if (it == per_cu.end()) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, block_threads, 0) != hipSuccess) {
            (void)hipGetLastError();
            n = 0;
        }
        it = per_cu.emplace(std::make_pair(kernel, dev), n).first;
    }
    return it->second;
}
bool fsn_grid_fits(const void* kernel, int block_threads, unsigned grid) {
    int cus = 0;
    const int occ = persist_occupancy(kernel, block_threads, &cus);
    return (unsigned long long)occ * (unsigned long long)cus >= grid;
}
// Called by every launcher of a kernel that needs its whole grid resident, right before the launch (inside the API
// function's FSN_PERSIST_BEGIN scope; a no-op outside one, e.g. under stream capture).
void fsn_persist_admit(const void* kernel, int block_threads, unsigned grid) {
    if (!t_persist) return;
    int cus = 0;
    const int occ = persist_occupancy(kernel, block_threads, &cus);
    if (occ < 1 || cus < 1) {
        t_persist->admit(1.0, 1);
        return;
    }
    t_persist->admit((double)grid / ((double)occ * (double)cus), occ);
}
// The sticky record of the running call's stream (created on first use; not under stream capture, where pinned
// allocations are not allowed: a captured launch then only poisons its outputs).
unsigned* fsn_ctx_sticky() {
    StreamCtx* c = cur_ctx();
    if (c->sticky_dev) return c->sticky_dev;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(t_stream, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;
    }
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    memset(h, 0, 64);
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(h);
        return nullptr;
    }
    c->sticky_host = static_cast<unsigned*>(h);
    c->sticky_dev = static_cast<unsigned*>(d);
    return c->sticky_dev;
}
// Called before every persistent launch: a stream on which such a launch ran out of time keeps failing until the
// caller has looked (fsn_stream_status) and cleared the record - garbage is never consumed silently.
int persist_precheck() {
    StreamCtx* c = cur_ctx();
    if (c->sticky_host) {
        const unsigned st = __atomic_load_n(&c->sticky_host[0], __ATOMIC_ACQUIRE);
        if (st != 0 && !c->timeout_defer) {
            fsn_set_error("a persistent kernel launched earlier on this stream ran out of time waiting for its partner "
                          "workgroups (status %u, %u such launches): its outputs are NaN; see fsn_stream_status / "
                          "fsn_stream_status_clear", st, __atomic_load_n(&c->sticky_host[1], __ATOMIC_ACQUIRE));
            return FSN_ERR_TIMEOUT;
        }
    }
    (void)fsn_ctx_sticky();
    return FSN_OK;
}

extern "C" int fsn_set_persistent_mode(int mode) {
    FSN_REQUIRE(mode == FSN_PERSISTENT_AUTO || mode == FSN_PERSISTENT_NEVER, "persistent mode %d unknown", mode);
    g_persist_mode.store(mode, std::memory_order_relaxed);
    return FSN_OK;
}
// Test hooks without a device: the gate's admission rule on a hypothetical set (n launches, fractions of the chip and
// resident workgroups per CU), and the K-split plan of a weight-gradient product against the bound its scratch is sized by.
extern "C" int fsn_debug_persist_set_fits(int n, const double* fracs, const int* occs) {
    if (n < 1 || n > 64 || !fracs || !occs) return -1;
    std::vector<PersistEntry> e((size_t)n);
    std::vector<const PersistEntry*> set;
    for (int i = 0; i < n; ++i) {
        e[(size_t)i].frac = fracs[i];
        e[(size_t)i].occ = occs[i] < 1 ? 1 : occs[i] > 8 ? 8 : occs[i];
        set.push_back(&e[(size_t)i]);
    }
    return n == 1 || persist_set_fits(set) ? 1 : 0;
}
extern "C" int fsn_debug_tn_plan(int M, int Nc, long K, int arith, int* splits, long* bound) {
    if (M < 1 || Nc < 1 || K < 1) return -1;
    fsn_tn_plan_splits(M, Nc, K, arith, splits, bound);
    return 0;
}
void fsn_tn16h_wide(int on);
extern "C" int fsn_debug_tn16h_wide(int on) {
    fsn_tn16h_wide(on);
    return FSN_OK;
}
extern "C" int fsn_debug_persist_stats(unsigned* launches, unsigned* waits, unsigned* unreported) {
    if (launches) *launches = g_persist_launches.load(std::memory_order_relaxed);
    if (waits) *waits = g_persist_waits.load(std::memory_order_relaxed);
    if (unreported) *unreported = g_persist_unreported.load(std::memory_order_relaxed);
    return FSN_OK;
}
extern "C" unsigned fsn_debug_core_last_launches(void) { return t_launch_trace; }
extern "C" int fsn_set_persistent_timeout_ms(int ms) {
    FSN_REQUIRE(ms >= 1 && ms <= 3600000, "timeout %d ms out of range [1, 3600000]", ms);
    g_persist_timeout_ms.store(ms, std::memory_order_relaxed);
    return FSN_OK;
}
extern "C" int fsn_stream_status(void* stream, int synchronize, unsigned* status_out, unsigned* events_out) {
    CallScope scope(stream);
    if (synchronize && hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) {
        fsn_set_error("fsn_stream_status: hipStreamSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
        return FSN_ERR_LAUNCH;
    }
    StreamCtx* c = cur_ctx();
    const unsigned st = c->sticky_host ? __atomic_load_n(&c->sticky_host[0], __ATOMIC_ACQUIRE) : 0u;
    const unsigned ev = c->sticky_host ? __atomic_load_n(&c->sticky_host[1], __ATOMIC_ACQUIRE) : 0u;
    if (status_out) *status_out = st;
    if (events_out) *events_out = ev;
    if (st != 0) {
        fsn_set_error("a persistent kernel on this stream ran out of time waiting for its partner workgroups (status %u, "
                      "%u such launches): something else held the CUs longer than the bound (fsn_set_persistent_timeout_ms)",
                      st, ev);
        return FSN_ERR_TIMEOUT;
    }
    return FSN_OK;
}
extern "C" int fsn_stream_timeout_policy(void* stream, int policy) {
    FSN_REQUIRE(policy == FSN_TIMEOUT_REFUSE || policy == FSN_TIMEOUT_DEFER, "timeout policy %d unknown", policy);
    CallScope scope(stream);
    cur_ctx()->timeout_defer = policy == FSN_TIMEOUT_DEFER;
    return FSN_OK;
}
extern "C" int fsn_stream_status_clear(void* stream) {
    CallScope scope(stream);
    StreamCtx* c = cur_ctx();
    if (c->sticky_host) {
        __atomic_store_n(&c->sticky_host[0], 0u, __ATOMIC_RELEASE);
        __atomic_store_n(&c->sticky_host[1], 0u, __ATOMIC_RELEASE);
    }
    return FSN_OK;
}
// Test hook for the safety net of the persistent kernels (fsn_launch_poison_if): out[0..n) becomes NaN iff *status != 0.
extern "C" int fsn_debug_poison_if(const void* status, float* out, size_t n, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(status && out, "NULL pointer argument");
    return fsn_launch_poison_if(static_cast<const unsigned*>(status), out, n, static_cast<hipStream_t>(stream));
}

// Test hook: a foreign kernel of `workgroups` x 256 threads that holds its CUs (lds_bytes of LDS each, ~200 registers
// per lane when heavy) for `ms` milliseconds on `stream`; sink is one device float it never writes.
extern "C" int fsn_debug_hog(int workgroups, int lds_bytes, int heavy, float ms, float* sink, void* stream) {
    CallScope scope(stream);
    FSN_REQUIRE(workgroups >= 1 && workgroups <= 65536 && lds_bytes >= 4 && lds_bytes <= 160 * 1024 && ms >= 0.f &&
                    ms <= 10000.f && sink,
                "fsn_debug_hog: workgroups in [1, 65536], lds_bytes in [4, 163840], ms in [0, 10000], sink non-NULL");
    int khz = 100000;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, t_dev);
    if (khz <= 0) khz = 100000;
    return fsn_launch_hog(workgroups, lds_bytes, heavy, (unsigned long long)((double)ms * khz), sink,
                          static_cast<hipStream_t>(stream));
}
extern "C" int fsn_profile_enable(void* stream, int on) {
    CallScope scope(stream);
    cur_ctx()->prof_on = on != 0;
    return FSN_OK;
}
extern "C" int fsn_profile_num_stages(void) { return ST_COUNT; }
extern "C" const char* fsn_profile_stage_name(int stage) {
    return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : "";
}
// Milliseconds per stage of the LAST profiled call on `stream`; waits for that call's events only.
extern "C" int fsn_profile_read(void* stream, float* ms, int n) {
    if (!ms || n < ST_COUNT) {
        fsn_set_error("fsn_profile_read: need room for %d stages", (int)ST_COUNT);
        return FSN_ERR_ARG;
    }
    CallScope scope(stream);
    StreamCtx* c = cur_ctx();
    for (int i = 0; i < ST_COUNT; ++i) {
        float v = 0.f;
        for (int j = 0; j < c->spans[i]; ++j) {
            float e = 0.f;
            if (hipEventSynchronize(c->ev[i][j][1]) != hipSuccess ||
                hipEventElapsedTime(&e, c->ev[i][j][0], c->ev[i][j][1]) != hipSuccess) {
                fsn_set_error("fsn_profile_read: event query failed for stage %s", kStageNames[i]);
                return FSN_ERR_LAUNCH;
            }
            v += e;
        }
        ms[i] = v;
    }
    return FSN_OK;
}

// ---- auxiliary stream for the left-over sub-band rows (see fsn_lstm_rec_plan) -------------------
// One per (device, caller stream), created lazily on the caller stream's device (StreamCtx).  The fork / join
// below uses events only, so it is also legal under stream capture.
static int aux_init(StreamCtx* c) {
    if (c->aux) return FSN_OK;
    if (hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        fsn_set_error("cannot create the auxiliary stream / events");
        c->aux = nullptr;
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}
int aux_fork(hipStream_t s, hipStream_t* aux) {
    StreamCtx* c = cur_ctx();
    FSN_TRY(aux_init(c));
    if (hipEventRecord(c->ev_fork, s) != hipSuccess || hipStreamWaitEvent(c->aux, c->ev_fork, 0) != hipSuccess) {
        fsn_set_error("aux stream fork failed");
        return FSN_ERR_LAUNCH;
    }
    *aux = c->aux;
    return FSN_OK;
}
int aux_join(hipStream_t s) {
    StreamCtx* c = cur_ctx();
    if (hipEventRecord(c->ev_join, c->aux) != hipSuccess || hipStreamWaitEvent(s, c->ev_join, 0) != hipSuccess) {
        fsn_set_error("aux stream join failed");
        return FSN_ERR_LAUNCH;
    }
    return FSN_OK;
}
