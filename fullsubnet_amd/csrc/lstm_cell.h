// What the two persistent kernels with the input projection inside (lstm_rec_in_kernels.hip, lstm_rec_x_kernels.hip) share
// beyond fsn_common.h: the gate non-linearities on pairs of values and the GRU-as-four-gate-cell convention.  Device code only.
#pragma once
#include "fsn_common.h"

// Gate non-linearities on PAIRS of values (round 5): fp32 MFMAs and vector instructions do not overlap on a SIMD
// (tools/probe_overlap.hip: the times add whoever issues them), so every vector instruction of the persistent kernels is
// paid in full; v_pk_mul / v_pk_add / v_pk_fma_f32 do two lanes' worth of the multiplies and adds around the
// transcendentals per issue.  Same IEEE operations as sigmoid_fast / tanh_fast (1 - 2 r == fma(-2, r, 1) exactly).
__device__ __forceinline__ f32x2 sigmoid_fast2(f32x2 x) {
    const f32x2 t = x * f32x2{-1.4426950408889634f, -1.4426950408889634f};
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + f32x2{1.0f, 1.0f};
    return f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}
__device__ __forceinline__ f32x2 tanh_fast2(f32x2 x) {
    const f32x2 t = x * f32x2{2.8853900817779268f, 2.8853900817779268f};
    const f32x2 d = f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])} + f32x2{1.0f, 1.0f};
    const f32x2 r = f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    return __builtin_elementwise_fma(r, f32x2{-2.0f, -2.0f}, f32x2{1.0f, 1.0f});
}
__device__ __forceinline__ f32x2 lo2(f32x4 v) { return __builtin_shufflevector(v, v, 0, 1); }
__device__ __forceinline__ f32x2 hi2(f32x4 v) { return __builtin_shufflevector(v, v, 2, 3); }
__device__ __forceinline__ f32x4 cat2(f32x2 a, f32x2 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3); }

// GRU as a four-gate cell (template parameter GRU of lstm_rec_in_kernel / lstm_rec_x_kernel): nn.GRU (audio_zen/model/module/
// sequence_model.py:59-66) on the same kernels, written as a FOUR-gate cell whose gate slots follow the kernels' order of evaluation
// (slot 1, 0, 2, 3):  slot 1 = r (W_ir x + W_hr h + b_ir + b_hr), slot 0 = nh (W_hn h + b_hn: zero input block),
// slot 2 = nx (W_in x + b_in: zero recurrent block), slot 3 = z (fsn_launch_gru_expand4, order 1).  Passes:
//   r:  tmp = sig(a)      nh: tmp = tmp a      nx: tmp = tanh(a + tmp) = n      z: h = n + sig(a) (h_{t-1} - n)
// (= (1 - z) n + z h_{t-1}); `cst` holds h in fp32 where the LSTM holds c.  The products of the two zero blocks are
// skipped (nx: no recurrent K loop; nh: no input chunks / slices from step 1 on): 3/4 of the LSTM's matrix work.

// One gate pass' update of the accumulator-shaped state, on pairs: VAR[rt][u] = EXPR(a, c, m) for every (row tile, unit group)
// of the wave, with a / c / m the halves of acc / cst / tmp[rt][u] - names of the kernel's own arrays, as are RT and UG.
// (The four-pass chain that uses it is written out in both kernels; as one shared template it does not compile to the same
// instruction stream: profiles/persist_sync_refactor.md.)
#define FSN_CELL_PASS2(VAR, EXPR)                                                                     \
    _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                                 \
    _Pragma("unroll") for (int u = 0; u < UG; ++u) {                                                  \
        const f32x4 A = acc[rt][u], C = cst[rt][u], M = tmp[rt][u];                                   \
        (void)A, (void)C, (void)M;                                                                    \
        auto half = [&](f32x2 a, f32x2 c, f32x2 m) { (void)a, (void)c, (void)m; return EXPR; };       \
        VAR[rt][u] = cat2(half(lo2(A), lo2(C), lo2(M)), half(hi2(A), hi2(C), hi2(M)));                \
        asm volatile("" : "+v"(VAR[rt][u]));                                                          \
    }
