"""The table, the references and the checkers of tests/test_gpu_infer_glue_sweep.py, tried without a GPU.

* The references: the ragged fast-glue reference (a batch of one per row) equals the oracle called on the whole batch when every
  row has T0 frames; the fp64 references agree with the oracle's fp32 functions to fp32 accuracy on every arithmetic row; the
  fp64 cIRM transcriptions agree with the oracle's fp32 functions and with the golden `elementwise` file.
* The checkers accept the fp32 stand-in (the oracle at np.float32; torch on the CPU for the cIRM algebra) on every arithmetic
  row under the hard and the sharp rule, and reject each of fourteen wrong stand-ins on the row that exists for its path.
* The size queries (fsn_fast_glue_workspace_bytes, fsn_fast_low_rate_frames, fsn_improved_section_input_workspace_bytes) and the
  argument refusals, which launch nothing and need no device.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

import test_gpu_infer_glue_sweep as S

ROW = {r.id: r for r in S.TABLE}
ARITH = [r for r in S.TABLE if r.kind in ("norm", "bneck", "section")]
CIRM = [r for r in S.TABLE if r.kind in ("compress", "decompress", "build")]
ENTRIES = ["fsn_fast_spec_rows", "fsn_fast_spec_rows_ragged", "fsn_fast_norm_rows", "fsn_fast_norm_rows_ragged", "fsn_fast_bottleneck_input",
           "fsn_fast_bottleneck_input_ragged", "fsn_fast_decoder_input", "fsn_fast_mask_out", "fsn_fast_mask_out_ragged",
           "fsn_fast_low_rate_frames", "fsn_fast_glue_workspace_bytes", "fsn_improved_section_input", "fsn_improved_front",
           "fsn_bft_to_rows", "fsn_rows_to_bft", "fsn_improved_mask_apply", "compress", "decompress", "build"]


def _frame_sets(row):
    if row.kind == "section":
        return (None,)
    return ((None,) if row.frames is None else (None, row.frames)) if row.la == 0 else (row.frames,)


def _outs(row, ops, frames, dtype, variant=""):
    """What the entries return for one draw, from the reference at `dtype` (with a variant: a wrong one), as fp32."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    if row.kind == "norm":
        out, den, valid = S.norm_reference(row, ops, frames, dtype, variant)
        _, _, v0 = S.norm_reference(row, ops, frames)
        return dict(norm=f32(out[v0]), den=f32(den))
    if row.kind == "bneck":
        _, live, dl, _ = S.bneck_want(row, *ops, frames)
        r = S.bneck_reference(row, *ops, frames, dtype, variant)
        return dict(units=f32(r["units"][live]), ds=f32(r["ds"][dl]), bden=f32(r["den"]))
    out, den = S.section_reference(row, *ops, dtype, variant)
    return dict(section=f32(out), sden=f32(den))


def _want(row, ops, frames):
    if row.kind == "norm":
        return S.norm_want(row, ops, frames)[0]
    if row.kind == "bneck":
        return S.bneck_want(row, *ops, frames)[0]
    return S.section_want(row, *ops)


def _ops(row, draw):
    return {"norm": S.make_norm_ops, "bneck": S.make_bneck_ops, "section": S.make_section_ops}[row.kind](row, draw)


def _judge(row, dtype, variant="", names=None):
    """Pooled over draws like the GPU test."""
    stats, draw = {}, -1
    while not S.pooled(row, stats, draw := draw + 1):
        ops = _ops(row, draw)
        for frames in _frame_sets(row):
            outs = _outs(row, ops, frames, dtype, variant)
            S.judge(stats, _want(row, ops, frames), outs if names is None else {k: outs[k] for k in names})
    for s in stats.values():
        s.check()
    return stats


def test_every_entry_has_a_row():
    src = open(S.__file__).read()
    for name in ENTRIES:
        assert name in src, name
    kinds = {r.kind for r in S.TABLE}
    assert set(S.RUNNERS) | set(S.REFUSALS) == kinds and len({r.id for r in S.TABLE}) == len(S.TABLE)


@pytest.mark.parametrize("row", ARITH, ids=lambda r: r.id)
def test_checkers_accept_the_oracle_at_float32(row):
    """The hard and the sharp rule on the fp32 CPU evaluation alone: a row it could not pass would measure nothing.  Also: the
    fp64 reference equals the oracle's fp32 functions to fp32 accuracy."""
    stats = _judge(row, np.float32)
    assert all(s.scalar or s.n >= S.POOL_ELEMS for s in stats.values())
    assert all(s.hard <= 1.0 for s in stats.values())
    ops = _ops(row, 0)
    for frames in _frame_sets(row):
        a, b = _outs(row, ops, frames, np.float64), _outs(row, ops, frames, np.float32)
        for k in a:
            np.testing.assert_allclose(b[k], a[k], rtol=2e-6, atol=0)


@pytest.mark.parametrize("row", [r for r in S.TABLE if r.kind in ("norm", "bneck")], ids=lambda r: r.id)
def test_ragged_reference_is_the_batch_reference_when_every_row_is_whole(row):
    """The per-row (batch of one) sequence with frames[b] = T0 everywhere against the oracle on the whole batch."""
    ops = _ops(row, 0)
    if row.kind == "norm":
        if row.la:
            return
        out, _, valid = S.norm_reference(row, ops, [row.T] * row.B)
        assert valid.all()
        np.testing.assert_array_equal(out, O.offline_laplace_norm(ops.transpose(1, 0, 2), np.float64).transpose(1, 0, 2))
        return
    mel, enc = ops
    r = S.bneck_reference(row, mel, enc, [row.T] * row.B)
    nu = O.freq_unfold(mel.astype(np.float64)[:, None], row.nm).reshape(row.B, row.M, -1, row.T)
    eu = O.freq_unfold(enc.astype(np.float64)[:, None], row.ne).reshape(row.B, row.M, -1, row.T)
    ds = S.MF.real_time_downsampling(np.concatenate([nu, eu], axis=2), row.shrink)
    whole = O.offline_laplace_norm(ds, np.float64)                                        # [B, M, W, Ts]
    np.testing.assert_array_equal(r["units"], whole.transpose(3, 0, 1, 2).reshape(r["units"].shape))
    plain = S.bneck_reference(row, mel, enc, None)
    for k in ("units", "ds", "den"):
        np.testing.assert_array_equal(plain[k], r[k])


WRONG = [  # (stand-in, row, the output that must give it away)
    ("edge_repeat", "bneck-nb5-0", "units"),
    ("edge_repeat", "bneck-nb-M-1-both-mirrors-on-one-band", "units"),
    ("gathered_mean", "bneck-nb2-1", "bden"),
    ("gathered_mean", "bneck-nb2-1", "units"),
    ("short_block_by_shrink", "bneck-s3-T5", "ds"),
    ("short_block_by_shrink", "bneck-s7-T3", "units"),
    ("frame0_in_block", "bneck-s2-T4", "ds"),
    ("padded_count", "norm-ragged-la0", "norm"),
    ("no_lookahead", "norm-ragged-la2", "norm"),
    ("shard_mean", "section-shard-first", "section"),
    ("shard_mean", "section-shard-tail", "sden"),
    ("fb_noisy_neighbors", "section-low-mirror", "section"),
]


@pytest.mark.parametrize("variant,row_id,name", WRONG, ids=[f"{v}-{r}-{n}" for v, r, n in WRONG])
def test_wrong_standins_are_rejected(variant, row_id, name):
    """Evaluated at float64 and rounded once, so that nothing but the defect separates the stand-in from the reference; the named
    output alone must be enough."""
    row = ROW[row_id]
    ops = _ops(row, 0)
    fr = _frame_sets(row)[-1]
    assert not np.array_equal(_outs(row, ops, fr, np.float64, variant)[name], _outs(row, ops, fr, np.float64)[name]), "not wrong here"
    _judge(row, np.float64)
    with pytest.raises(AssertionError):
        _judge(row, np.float64, variant, names=(name,))


@pytest.mark.parametrize("row_id,name", [("norm-T257-C1", "norm"), ("bneck-M64", "units"), ("section-T65", "section")])
def test_two_ulp_at_tensor_max_scale_is_rejected(row_id, name):
    row = ROW[row_id]
    stats, draw = {}, -1
    while not S.pooled(row, stats, draw := draw + 1):
        ops = _ops(row, draw)
        t = _outs(row, ops, None, np.float32)[name].copy()
        if draw == 0:
            i = np.unravel_index(int(np.argmin(np.abs(t) + (t == 0) * 1e30)), t.shape)  # the smallest element, the largest scale
            t[i] += 2 * np.spacing(np.abs(t).max())
        S.judge(stats, _want(row, ops, None), {name: t})
    with pytest.raises(AssertionError):
        stats[name].check()


# ---- the exact outputs ------------------------------------------------------------------------------------------------------

def test_upsampling_indexed_t_plus_1_is_rejected():
    for row in (r for r in S.TABLE if r.kind == "dec"):
        enc, slow = S.make_dec_ops(row)
        for relu in (0, 1):
            S.check_dec(row, enc, slow, relu, S.dec_reference(row, enc, slow, relu))
    row = ROW["dec-s3-T10"]
    enc, slow = S.make_dec_ops(row)
    with pytest.raises(AssertionError):
        S.check_dec(row, enc, slow, 0, S.dec_reference(row, enc, slow, 0, "t_plus_1"))


def test_minus_zero_through_relu_is_compared_by_value():
    row = ROW["dec-s2-T3"]
    enc, slow = S.make_dec_ops(row)
    assert np.signbit(slow[0, 0]) and slow[0, 0] == 0
    got = S.dec_reference(row, enc, slow, 1)
    assert not np.signbit(got[0, 0, row.M])
    got[0, 0, row.M] = -0.0  # what fmaxf may return
    S.check_dec(row, enc, slow, 1, got)
    got[0, 0, row.M] = 1e-30
    with pytest.raises(AssertionError):
        S.check_dec(row, enc, slow, 1, got)


def test_mask_frames_shifted_the_wrong_way_are_rejected():
    row = next(r for r in S.TABLE if r.kind == "mask" and r.la == 2 and r.T0 >= 31 and r.F > 1)
    o = S.make_mask_ops(row)
    fr = S.ragged_frames(row.T0, row.B)
    assert {S.row_frames(fr, b, row.T0) for b in range(row.B)} >= {1, row.T0}
    want = S.mask_reference(row, o, fr)
    assert not want[1, :, 1:].any() and want[1, :, 0].all()  # a row of one frame: zeros behind it
    np.testing.assert_array_equal(want[0], o[row.la:, 0].T)
    with pytest.raises(AssertionError):
        S.check_exact("mask", S.mask_reference(row, o, fr, "shift_wrong"), want)


def test_spec_reference_zeroes_what_lies_beyond_a_row():
    row = next(r for r in S.TABLE if r.kind == "spec" and r.la == 2 and r.T0 >= 33 and r.F > 1)
    mag = S.make_spec_ops(row)
    fr = S.ragged_frames(row.T0, row.B)
    want = S.spec_reference(row, mag, fr, row.B + 3, row.F + 40)
    assert want.shape == (row.T0 + row.la, row.B + 3, row.F + 40)
    assert not want[:, row.B:].any() and not want[:, :, row.F:].any() and not want[row.T0:].any() and not want[1:, 1].any()
    np.testing.assert_array_equal(want[:row.T0, 0, :row.F], mag[0].T)


@pytest.mark.parametrize("variant", ["swap_planes", "uncovered_unwritten"])
def test_wrong_mask_products_are_rejected(variant):
    row = ROW["apply-ld16-c2-T31"]
    ops = S.make_apply_ops(row)
    secs, F = ops[0], ops[1]
    assert secs[0]["lower"] > 0 and secs[2]["lower"] > secs[0]["lower"] + secs[0]["units"] * secs[0]["center"] and secs[1]["units"] == 0
    er, ei = S.apply_reference(row, *ops)
    assert not er[:, F - 1].any() and not er[:, 0].any() and er[:, secs[0]["lower"]].all()
    bad = S.apply_reference(row, *ops, variant)
    with pytest.raises(AssertionError):
        S.check_exact("er", bad[0], er)


def test_mask_apply_rows_cover_every_rows_per_workgroup_and_the_second_launch():
    R = {s["R"] for r in S.TABLE if r.kind == "apply" for s in S.apply_layout(r)[0]}
    assert R >= {8, 7, 5, 2, 1}
    big = S.apply_layout(ROW["apply-second-grid-y-launch"])[0][0]
    assert -(-big["units"] // big["R"]) > 65535


def test_front_reference_is_numpys_sqrt():
    mag = S.make_front_ops(ROW["front-special-values"])
    out = S.front_reference(mag, 1)
    assert out.dtype == np.float32 and out[0, 0, 0] == 0 and out[0, 0, 5] == 2.0 and out[0, 0, 1] > 0
    row = ROW["front-stride-loop"]
    assert row.B * (row.F - 1) * row.T > 4096 * 256


# ---- cIRM --------------------------------------------------------------------------------------------------------------------

def test_cirm_transcriptions_equal_the_oracle_and_the_golden_file():
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "elementwise.npz"))
    np.testing.assert_allclose(S.decompress64(z["m"].astype(np.float64)), z["dm"], rtol=3e-6, atol=2e-6)
    np.testing.assert_allclose(S.compress64(z["raw"].astype(np.float64)), z["comp"], rtol=3e-6, atol=1e-6)
    g = np.random.default_rng(3)
    m = g.uniform(-12, 12, 4096).astype(np.float32)
    np.testing.assert_allclose(S.decompress64(m.astype(np.float64)), O.decompress_cIRM(m), rtol=3e-6, atol=2e-6)
    raw = (g.standard_normal(4096) * 50).astype(np.float32)
    np.testing.assert_allclose(S.compress64(raw.astype(np.float64)), O.compress_cIRM(raw), rtol=3e-6, atol=1e-6)
    a = [g.standard_normal(512).astype(np.float32) for _ in range(4)]
    np.testing.assert_allclose(S.build64(*(x.astype(np.float64) for x in a)), O.build_complex_ideal_ratio_mask(*a), rtol=2e-5, atol=2e-5)
    assert np.isnan(S.compress64(np.array([np.nan]))).all() and np.isnan(S.decompress64(np.array([np.nan]))).all()


@pytest.mark.parametrize("row", CIRM, ids=lambda r: r.id)
def test_cirm_checker_accepts_torch_fp32(row):
    st, draw = S.stat({}, row.kind), -1
    while st.n < S.POOL_ELEMS:
        ops = S.make_cirm_ops(row, draw := draw + 1)
        (ref, Sabs, cpu), keep = S.cirm_want(row, ops)
        assert np.isfinite(ref[keep]).all() and np.isfinite(cpu[keep]).all()
        st.add(cpu[keep], ref[keep], Sabs[keep], cpu[keep])
    assert st.n >= S.POOL_ELEMS
    st.check()
    assert st.hard <= 1.0  # torch's own expf / logf meet the printed k: S is not too small


def test_decompress_clamped_at_10_is_rejected():
    row = ROW["decompress-n257"]
    ops = S.make_cirm_ops(row, 0)
    (ref, Sabs, cpu), keep = S.cirm_want(row, ops)
    with np.errstate(all="ignore"):
        bad = S.cirm_want(row, ops, "clamp10")[0][0].astype(np.float32)
    st = S.stat({}, "decompress")
    st.add(bad[keep], ref[keep], Sabs[keep], cpu[keep])
    with pytest.raises(AssertionError):
        st.check()
    good = ref.astype(np.float32)
    fin = np.isfinite(ops[0]) | np.isnan(ops[0])
    S.check_cirm_specials("decompress", ops[0][fin], good[fin])
    with pytest.raises(AssertionError):
        S.check_cirm_specials("decompress", ops[0][fin], bad[fin])


def test_compress_saturation_checks():
    row = ROW["compress-n256"]
    x = S.make_cirm_ops(row, 0)[0]
    fin = np.isfinite(x) | np.isnan(x)  # the tensor expression gives NaN at -inf; the kernel's clamp is held on the GPU
    good = S.compress64(x.astype(np.float64)).astype(np.float32)
    S.check_cirm_specials("compress", x[fin], good[fin])
    bad = good.copy()
    bad[np.flatnonzero(x == np.float32(2000.0))[0]] = np.float32(9.999999)
    with pytest.raises(AssertionError):
        S.check_cirm_specials("compress", x[fin], bad[fin])


# ---- size queries and refusals: host code, no device ---------------------------------------------------------------------------

def test_size_queries():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    for T in range(2, 40):
        for s in (1, 2, 3, 4, 7):
            Ts = L.fsn_fast_low_rate_frames(T, s)
            x = np.zeros((1, T))
            assert Ts == S.low_rate(T, s) == S.MF.real_time_downsampling(x, s).shape[-1]
            assert (T - 1) // s < Ts  # every frame's held low-rate frame exists
            for B, M in ((1, 2), (3, 65), (64, 300)):
                assert L.fsn_fast_glue_workspace_bytes(T, B, M, s) == S.ru(2 * Ts * B * M * 4, 256) + S.ru(B * 4, 256)
    assert L.fsn_fast_low_rate_frames(1, 2) == 0 and L.fsn_fast_low_rate_frames(4, 0) == 0
    assert L.fsn_fast_glue_workspace_bytes(1, 1, 2, 2) == 0 and L.fsn_fast_glue_workspace_bytes(4, 0, 2, 2) == 0
    for B, F in ((1, 2), (3, 33), (64, 70)):
        assert L.fsn_improved_section_input_workspace_bytes(B, F) == S.ru((4 * B * F + B + 16) * 4, 256)
    assert L.fsn_improved_section_input_workspace_bytes(1, 1) == 0


def test_argument_refusals_need_no_device():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    host = (ctypes.c_float * 16)()
    p = ctypes.cast(host, ctypes.c_void_p)
    for case in S.BNECK_REFUSALS:
        assert S.bneck_refusal_call(L, _lib, p, p, *case, None) != 0 and L.fsn_last_error(), case
    for case in S.SECTION_REFUSALS:
        assert S.section_refusal_call(L, p, p, *case, None) != 0 and L.fsn_last_error(), case
    assert L.fsn_fast_decoder_input(p, 1, p, 1, 1, 0, 65536, 1, 1, 1, 1, p, None) != 0 and b"65535" in L.fsn_last_error()
    sec = (_lib.MaskSection * 1)(_lib.MaskSection(p.value, 1, 481, 0, 1, 1))
    assert L.fsn_improved_mask_apply(1, ctypes.cast(sec, ctypes.c_void_p), p, p, 1, 2, 1, p, p, None) != 0
    assert any(float(v) == 0.0 for v in host)  # nothing was written
