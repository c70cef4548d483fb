// What the kernels that run a whole recurrence as ONE launch share (lstm_group_kernels.hip, lstm_group_bptt_kernels.hip,
// lstm_group16_kernels.hip, fb_chain_kernels.hip, fb_chain_bptt_kernels.hip, lstm_rec_in_kernels.hip, lstm_rec_x_kernels.hip):
// the cache-policy operand and the buffer accessors that take it, the flag handshake between workgroups (write-through
// payload, drain, ONE flag store; one wave polls, bounded by the clock; status word), and the LDS-DMA fragment.  A primitive
// that is slightly wrong here is a hang or silently stale data, not a failing assert: there is one copy of each, and the
// variants of the protocol stand side by side.  Device code only.
#pragma once
#include "fsn_common.h"

#ifdef __HIPCC__
// ---- cache policy of a memory access (the aux operand of the buffer builtins) ---------------------------------------------
// The scope of an exchanged payload.  sc1 = device scope: never from this CU's L1, and lines written by a CU of another XCD
// are fetched through the fabric - valid wherever the workgroups run; as a store it is a write-through store.  sc0: never
// from this CU's L1, served by this XCD's L2 - valid only between workgroups of ONE XCD (whose L2 is their point of
// coherence); lstm2_g16_fwd_kernel takes it when every workgroup of a cluster reports the same XCD at start (HW_REG_XCC_ID).
constexpr int FSN_CP_PLAIN = 0;
constexpr int FSN_CP_SC0 = 1;
constexpr int FSN_CP_SC1 = 16;

// ---- buffer resources -----------------------------------------------------------------------------------------------------
// Word 3 of a raw buffer descriptor on gfx950: DATA_FORMAT = 32 bits (bits 15 - 18 = 4), everything else zero (no swizzle, no
// index stride, no tid): byte offsets (lane offset + scalar offset), range-checked against `bytes`.
constexpr int FSN_RSRC_RAW32 = 0x00020000;
// `bytes` (at most 2 GB - 1, the reach of a resource's offsets): loads beyond it return zero, stores beyond it are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fsn_buffer_rsrc(const void* p, unsigned bytes = 0x7fffffff) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, FSN_RSRC_RAW32);
}
// 4 / 8 / 16 bytes per lane at (lane byte offset voff) + (wave-uniform byte offset soff) of resource r, cache policy CP
template <typename T, int CP = FSN_CP_PLAIN>
__device__ __forceinline__ T fsn_buffer_load(const __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "one dword, two or four per lane");
    if constexpr (sizeof(T) == 16) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, CP));
    else if constexpr (sizeof(T) == 8) return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, CP));
    else return __builtin_bit_cast(T, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, CP));
}
// (Exchanged payloads go out as whole 16-byte groups wherever the layout allows it, never as single dwords: a step of
// fb_chain_kernel publishes ~0.8 MB, and as dword stores that was 200 k partial-line write transactions per step - measured:
// 2 us of a 9.6 us step.)
template <int CP = FSN_CP_PLAIN, typename T>
__device__ __forceinline__ void fsn_buffer_store(const __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, const T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "one dword, two or four per lane");
    if constexpr (sizeof(T) == 16) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(fsn_u32x4, v), r, voff, soff, CP);
    else if constexpr (sizeof(T) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(fsn_u32x2, v), r, voff, soff, CP);
    else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, CP);
}
// write-through store (sc1): the line leaves this XCD's L2, any CU of the chip reads it after an agent-scope acquire (or
// with sc1 loads, which need none)
__device__ __forceinline__ void fsn_store_sc1(float* p, float v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the lane's fragment at element offset `ofs` of the packed weight buffer behind resource r (FsnWFrag, fsn_common.h)
template <int AR>
__device__ __forceinline__ typename FsnWFrag<AR>::type fsn_load_wfrag(const __amdgpu_buffer_rsrc_t r, unsigned lane,
                                                                     unsigned ofs) {
    if constexpr (AR == FSN_ARITH_F32) return fsn_buffer_load<f32x4>(r, lane * 16u, ofs * 4u);
    else return fsn_buffer_load<fsn_u32x2>(r, lane * 8u, ofs * 2u);
}

// ---- bounded waits ----------------------------------------------------------------------------------------------------------
// One 256-poll round of a bounded wait has passed: give up?  The first round only takes the time (t0), so that a wait
// that succeeds at once never touches the clock.  `code` identifies the wait (1 + step) in the status word.
__device__ __forceinline__ bool fsn_wait_give_up(unsigned* status, unsigned spins, unsigned long long& t0,
                                                 unsigned long long ticks, unsigned code) {
    const unsigned st = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long now = (unsigned long long)wall_clock64();
    if (spins < 256u) t0 = now;
    if (st == 0 && now - t0 <= ticks) return false;
    if ((threadIdx.x & 63) == 0 && st == 0) __hip_atomic_store(status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}
// The polling loops form their own lane index (they run in a cold branch: a value of the caller's would have to be kept
// alive for them); the early look and the check after it take the caller's own `wave` (wave-uniform: the kernels derive
// it through readfirstlane; recomputed from threadIdx.x it changes the generated code) and `lane`.

// Group family (clusters of M members per layer, one flag word per member): ONE wave polls the M member flags of a layer
// (relaxed agent-scope loads, never served by this CU's L1) until all have reached `epoch`; bounded.  Returns false after a
// timeout (status raised: all later waits fall through, the results are garbage, never a hang).
template <int M>
__device__ __forceinline__ bool fsn_group_poll(unsigned* flags, unsigned epoch, unsigned* status, unsigned long long ticks) {
    const int lane = threadIdx.x & 63;
    unsigned long long t0 = 0;
    for (unsigned spins = 0;; ++spins) {
        unsigned v = epoch;
        if (lane < M) v = __hip_atomic_load(flags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__all((int)(v >= epoch))) return true;
        if ((spins & 255u) == 255u && fsn_wait_give_up(status, spins, t0, ticks, 1u + epoch)) return false;
        __builtin_amdgcn_s_sleep(1);
    }
}
// the whole workgroup waits: wave 0 polls, a barrier tells the others
template <int M>
__device__ __forceinline__ void fsn_group_wait(unsigned* flags, unsigned epoch, unsigned* status, unsigned long long ticks) {
    if ((threadIdx.x >> 6) == 0) (void)fsn_group_poll<M>(flags, epoch, status, ticks);
    __syncthreads();  // one wave looked for all
}
// The same in two halves: the flags are looked at EARLY (before a K loop) and checked after it - in the steady state the
// early look already shows the awaited epoch and the check costs nothing; only otherwise does wave 0 poll.
// The early look is a closure over the kernel's `wave` and `lane` (`const FsnGroupPeek<M> peek{wave, lane};`), the shape of
// the lambda it was in every kernel: as a function of (wave, lane) by value the compiler merges the two conditions into one
// mask that lives through the time loop - same registers and LDS, but 1 - 4 more SGPR spills in the group kernels.
// It holds REFERENCES: bind it to the kernel's named locals, which outlive it - never to temporaries.
template <int M>
struct FsnGroupPeek {
    const int &wave, &lane;
    __device__ unsigned operator()(unsigned* flags) const {
        unsigned v = 0xffffffffu;
        if (wave == 0 && lane < M) v = __hip_atomic_load(flags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return v;
    }
};
template <int M>
__device__ __forceinline__ void fsn_group_wait_peeked(int wave, unsigned v, unsigned* flags, unsigned epoch, unsigned* status,
                                                      unsigned long long ticks) {
    if (wave == 0 && !__all((int)(v >= epoch))) (void)fsn_group_poll<M>(flags, epoch, status, ticks);
    __syncthreads();  // one wave looked for all
}

// Chain family (a stage of many workgroups, one flag word each, the array replicated): wave 0 waits until all `nflags` flags
// of a stage copy have reached `epoch` (read as 64-bit pairs) and, optionally, one more flag its own epoch - both looked at
// in the same round trip; bounded.  No sleep: a step of the chain is a few microseconds.
__device__ __forceinline__ bool fsn_chain_wait(const unsigned* flags, int nflags, unsigned epoch, const unsigned* one,
                                               unsigned one_epoch, unsigned* status, unsigned long long ticks) {
    const int lane = threadIdx.x & 63;
    const unsigned long long* f = reinterpret_cast<const unsigned long long*>(flags) + lane;
    unsigned long long t0 = 0;
    for (unsigned spins = 0;; ++spins) {
        unsigned long long v = ~0ull;
        unsigned w = ~0u;
        if (epoch > 0 && 2 * lane < nflags) v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (one && lane == 0) w = __hip_atomic_load(one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__all((int)((unsigned)v >= epoch && (unsigned)(v >> 32) >= epoch && w >= one_epoch))) return true;
        if ((spins & 255u) == 255u && fsn_wait_give_up(status, spins, t0, ticks, 1u + epoch)) return false;
    }
}
// the same for a stage of NF <= 64 workgroups, one flag per lane (fb_chain_bptt_kernel)
template <int NF>
__device__ __forceinline__ bool fsn_chain_wait_words(const unsigned* flags, unsigned epoch, const unsigned* one,
                                                     unsigned one_epoch, unsigned* status, unsigned long long ticks) {
    const int lane = threadIdx.x & 63;
    unsigned long long t0 = 0;
    for (unsigned spins = 0;; ++spins) {
        unsigned v = ~0u, w = ~0u;
        if (epoch > 0 && lane < NF) v = __hip_atomic_load(flags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (one && lane == 0) w = __hip_atomic_load(one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__all((int)(v >= epoch && w >= one_epoch))) return true;
        if ((spins & 255u) == 255u && fsn_wait_give_up(status, spins, t0, ticks, 1u + epoch)) return false;
    }
}

// ---- publish --------------------------------------------------------------------------------------------------------------
// The workgroup's write-through stores of this step are in flight: EVERY wave drains its own, a barrier, then ONE lane
// bumps the flag (relaxed, agent scope).  The barrier also closes the step's use of whatever LDS the callers say it does.
__device__ __forceinline__ void fsn_publish(unsigned* flag, unsigned epoch) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Chain family: workgroup j of a stage writes COPIES copies of its flag, STRIDE words apart (one store instruction, COPIES
// lanes); a consumer polls copy (its index % COPIES) - hundreds of pollers on the same few cache lines doubled the step time.
template <int COPIES, int STRIDE>
__device__ __forceinline__ void fsn_publish_copies(unsigned* flags, int j, unsigned epoch) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if ((int)threadIdx.x < COPIES)
        __hip_atomic_store(flags + (size_t)threadIdx.x * STRIDE + j, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- LDS-DMA --------------------------------------------------------------------------------------------------------------
// One 16-byte-per-lane LDS-DMA fragment (1 KB per wave, no registers, nothing for the waves to wait on): lane l's 16 bytes at
// `g` land at LDS byte address lds_base + 16 l (wave-uniform: it travels in M0, which is saved and restored).  Written as asm
// so that the compiler neither serialises later LDS reads behind it (it cannot tell ring stages apart and would wait for
// vmcnt(0) before every ds_read) nor counts it in its own vmcnt bookkeeping (an extra, OLDER request in the queue can only
// make its counted waits longer, never too short).  The READER owns the wait: it states its own s_waitcnt vmcnt before it
// touches the landing zone.
__device__ __forceinline__ void fsn_lds_dma(const void* g, unsigned lds_base) {
    unsigned saved;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, off\n\t"
        "s_nop 0\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(saved)
        : "s"(lds_base), "v"(g)
        : "memory");
}
// The same with the source address as a wave-uniform base (scalar registers) + this lane's byte offset: no per-fragment
// vector arithmetic at all.
__device__ __forceinline__ void fsn_lds_dma_s(const void* sbase, unsigned lane_bytes, unsigned lds_base) {
    unsigned saved;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %2, %3\n\t"
        "s_nop 0\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(saved)
        : "s"(lds_base), "v"(lane_bytes), "s"(sbase)
        : "memory");
}
#endif  // __HIPCC__
