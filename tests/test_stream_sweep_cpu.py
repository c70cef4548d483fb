"""The stateful reference, the table and the checkers of tests/test_gpu_stream_sweep.py (tests/stream_reference.py), tried on
the CPU with stand-ins for the device.

* The stateful step in fp64, chunked as every row of the table chunks it, agrees with the whole-sequence `model` of the core
  sweep to 1e-12 of the output's largest value: under the cumulative norm on the whole batch, under the offline norm one
  utterance at a time on its own total_frames (the frames below each row's total).
* The table: ids unique, the duplication rule, every split summing to T, every pool list distinct.
* The two layout queries: offsets strictly increasing and inside the size the *_state_bytes query returns; the pool's
  slot_bytes equal to state_bytes / capacity.
* The fp32 yardsticks themselves, fed to the checkers as the device, pass every rule - masks, fb_out, states, sums, divisors.
* Deliberately wrong stand-ins - the fp32 cell emulation with ONE thing wrong - FAIL with a message that names the row and
  the call: steps_done taken as 0 in the second call; the norm carries restarted at a chunk edge; h zeroed at a chunk edge;
  c carried but h from the neighbouring row; two slots' rows swapped in a permuted list; the running sums kept in fp32
  (caught by the sum rule at the resumed row, which it misses by several decades); a segment divisor that forgets the
  look-ahead zero frames.
"""
import ctypes
import re

import numpy as np
import pytest

import stream_reference as R
import test_gpu_core_sweep as S

QUIET = lambda s: None  # noqa: E731
BY_WHY = {r.why: r for r in R.TABLE}
SEQ_ROWS = [r for r in R.TABLE if r.entry != "pool"]


def test_table():
    ids = [r.id for r in R.TABLE]
    assert len(set(ids)) == len(ids)
    for r in R.TABLE:
        R.check_duplication(r)
        assert sum(r.split) == r.T and all(k >= 1 for k in r.split)
        assert [s0 for s0, _ in r.segments] == [sum(r.split[:c]) for c in range(len(r.split))]
        if r.entry == "pool":
            assert len(set(r.slots)) == len(r.slots) and r.split == (1, 3), r.id
            assert r.why == "ids-outside" or all(0 <= s < R.CAPACITY for s in r.slots)
        if r.totals is not None:
            assert len(r.totals) == r.B and max(r.totals) == r.T and min(r.totals) > r.la
    assert {tuple(r.slots) for r in R.TABLE if r.entry == "pool"} >= {(18,), (16, 0, 7), (7, 0, 16), tuple(range(18, -1, -1)),
                                                                     tuple(range(17, 0, -2)), (3, -1, 5, 19)}
    perm = BY_WHY["permutation"].slots
    assert sorted(perm) == list(range(R.CAPACITY)) and perm != sorted(perm) and perm != sorted(perm, reverse=True)
    assert R.pool_steps().tolist() == [3 * i for i in range(18)] + [100000]
    assert abs(R.make_inputs(257, 15, 512, 8, 2)[1].mean() - R.LEVEL) < 0.01


@pytest.mark.parametrize("row", SEQ_ROWS, ids=[r.id for r in SEQ_ROWS])
def test_chunked_step_agrees_with_the_whole_sequence_model(row):
    ref = R.reference_of(row)
    crm = np.concatenate(ref.crm["64"], axis=-1)  # [k, 2, F, T]
    fb = np.concatenate(ref.fb["64"], axis=-1)
    if row.resumed:  # no whole-sequence form starts from a state: another chunking of the same frames instead
        one = R.Ref("seq", row.k, (row.T,), row.F, row.Hf, row.nb, row.norm, True, None, row.la)
        want, want_fb = one.crm["64"][0], one.fb["64"][0]
        assert np.abs(crm - want).max() <= 1e-12 * np.abs(want).max() and np.abs(fb - want_fb).max() <= 1e-12 * np.abs(want_fb).max()
        return
    if row.norm == "cumulative":
        rows, want_fb = S.model(ref.mag, ref.params, 0, row.nb, "cumulative", np.float64, "torch")
        want = S.rows_to_mask(rows, row.k)
        assert np.abs(crm - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(fb - want_fb).max() <= 1e-12 * np.abs(want_fb).max()
        return
    for u, n in enumerate(ref.totals):  # one utterance at a time on its own total_frames = frames + look-ahead
        rows, want_fb = S.model(ref.mag[u:u + 1, :, :, :n - row.la], ref.params, row.la, row.nb, "offline", np.float64, "torch")
        want = S.rows_to_mask(rows, 1)[0]  # [2, F, n - la]: step s is the mask of frame s - la
        assert np.abs(crm[u, :, :, row.la:n] - want).max() <= 1e-12 * np.abs(want).max(), (row.id, u)
        assert np.abs(fb[u, :, :n] - want_fb[0]).max() <= 1e-12 * np.abs(want_fb).max(), (row.id, u)


def test_layout_queries():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    for row in R.TABLE:
        cfg = row.cfg(_lib)
        if row.entry == "pool":
            lay = _lib.stream_pool_layout(cfg)
            offs = [lay[k] for k in _lib.STREAM_POOL_LAYOUT[:15]]
            assert offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:])) and offs[-1] < lay["slot_bytes"]
            assert all(o % 256 == 0 for o in offs) and lay["slot_bytes"] % 256 == 0
            total = L.fsn_fullsubnet_stream_pool_state_bytes(ctypes.byref(cfg), R.CAPACITY)
            assert total > 0 and lay["slot_bytes"] * R.CAPACITY == total
            assert (lay["F"], lay["Hf"], lay["Hs"], lay["R"]) == (row.F, row.Hf, 384, row.la + 1) and lay["FP"] >= row.F
            # the arrays fit between their neighbours
            assert lay["fb_h1"] - lay["fb_h0"] >= 4 * row.Hf and lay["sb_h1"] - lay["sb_h0"] >= 4 * row.F * 384
            assert lay["sb_sum"] - lay["fb_sum"] >= 8 and lay["steps"] - lay["sb_sum"] >= 8 * row.F
            continue
        lay = _lib.stream_state_layout(cfg, row.B)
        offs = [lay[k] for k in _lib.STREAM_STATE_LAYOUT[:10]]
        assert offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:])) and all(o % 256 == 0 for o in offs)
        assert (lay["npad_fb"], lay["npad_sb"]) == (S.ru16(row.B), S.ru16(row.B * row.F))
        assert lay["fb_h1"] - lay["fb_h0"] >= 4 * lay["npad_fb"] * row.Hf and lay["sb_h1"] - lay["sb_h0"] >= 4 * lay["npad_sb"] * 384
        assert lay["sb_sum"] - lay["fb_sum"] >= 8 * row.B and lay["bytes"] - lay["sb_sum"] >= 8 * row.B * row.F
        query = L.fsn_fullsubnet_segment_state_bytes if row.entry == "segment" else L.fsn_fullsubnet_stream_state_bytes
        total = query(ctypes.byref(cfg), row.B)
        assert total > 0 and (lay["bytes"] <= total if row.entry == "segment" else lay["bytes"] == total)
    cfg = R.TABLE[0].cfg(_lib)
    buf = (ctypes.c_long * 21)()
    assert L.fsn_debug_stream_state_layout(ctypes.byref(cfg), 1, buf, 12) == -1
    assert L.fsn_debug_stream_state_layout(ctypes.byref(cfg), 0, buf, 13) == -1
    assert L.fsn_debug_stream_state_layout(ctypes.byref(cfg), 1, None, 13) == -1
    assert L.fsn_debug_stream_pool_layout(ctypes.byref(cfg), buf, 20) == -1
    assert L.fsn_debug_stream_pool_layout(None, buf, 21) == -1


# ---- the checkers on the yardsticks themselves ---------------------------------------------------------------------------

def _as_device(row, ref, crm=None, state=None):
    """What the device would hand back if it were the fp32 cell emulation: per-call crm / fb_out of the row's B rows and the
    state of its held rows."""
    sel = row.sel
    crm = ref.crm["c32"] if crm is None else crm
    state = ref.state["c32"] if state is None else state
    return [c[sel] for c in crm], [f[sel] for f in ref.fb["t32"]], R.take_state(state, sel[row.held], row.F)


@pytest.mark.parametrize("why", ["uneven-chunks", "fb-second-tile", "resumed", "permutation", "ids-outside", "ends-inside-last", "ends-on-edge"])
def test_the_yardstick_itself_passes(why):
    row = BY_WHY[why]
    ref = R.reference_of(row)
    crm, fb, state = _as_device(row, ref)
    worst = R.check_calls(row, ref, crm, fb, log=QUIET)
    assert worst["crm"][0] <= 1.0 + 1e-9 and worst["fb_out"][0] <= 1.0 + 1e-9
    ws = R.check_state(row, ref, state, log=QUIET)
    assert all(ws[n] <= 1.0 + 1e-9 for n in R.STATE_ARRAYS)
    if row.norm == "offline":
        den_fb, den_sb = ref.den["c32"]
        R.check_divisors(row, ref, den_fb[row.sel], den_sb[row.sel], np.concatenate(ref.fb["c32"], axis=-1)[row.sel], log=QUIET)
    else:
        assert ws["fb_sum"] <= 1.0 and ws["sb_sum"] <= 1.0


# ---- wrong stand-ins -------------------------------------------------------------------------------------------------------

def _flagged(row, what, check, call=None):
    pattern = re.escape(row.id) + (f".*call {call}" if call is not None else ".*call")
    with pytest.raises(AssertionError, match=pattern):
        check()
        pytest.fail(f"'{what}' passed the checker", pytrace=False)


def _tampered(row, ref, tamper, **kw):
    crm, _, state, _ = ref.run(np.float32, "cell", tamper=tamper, **kw)
    return _as_device(row, ref, crm, state)


def _at_call_1(f):
    return lambda c, st: f(st) if c == 1 else None


def test_steps_done_taken_as_zero_in_the_second_call():
    row = BY_WHY["uneven-chunks"]
    ref = R.reference_of(row)

    def wrong(st):
        st["steps"] = st["steps"] * 0
    crm, fb, _ = _tampered(row, ref, _at_call_1(wrong))
    _flagged(row, "steps_done = 0 in the second call", lambda: R.check_calls(row, ref, crm, fb, log=QUIET), call=1)


def test_norm_carry_restarted_at_a_chunk_edge():
    row = BY_WHY["uneven-chunks"]
    ref = R.reference_of(row)

    def wrong(st):
        st["fb_sum"], st["sb_sum"] = st["fb_sum"] * 0, st["sb_sum"] * 0
    crm, fb, state = _tampered(row, ref, _at_call_1(wrong))
    _flagged(row, "the norm carries restarted", lambda: R.check_calls(row, ref, crm, fb, log=QUIET), call=1)
    _flagged(row, "the norm carries restarted (sum rule)", lambda: R.check_sums(row, ref, state, log=QUIET))


def test_h_zeroed_at_a_chunk_edge():
    row = BY_WHY["uneven-chunks"]
    ref = R.reference_of(row)

    def wrong(st):
        st["sb"][0], st["sb"][1] = st["sb"][0] * 0, st["sb"][1] * 0
    crm, fb, _ = _tampered(row, ref, _at_call_1(wrong))
    _flagged(row, "h zeroed at a chunk edge", lambda: R.check_calls(row, ref, crm, fb, log=QUIET), call=1)


def test_c_carried_but_h_from_the_neighbouring_row():
    row = BY_WHY["uneven-chunks"]
    ref = R.reference_of(row)

    def wrong(st):
        st["sb"][0], st["sb"][1] = np.roll(st["sb"][0], 1, axis=0), np.roll(st["sb"][1], 1, axis=0)
    crm, fb, state = _tampered(row, ref, lambda c, st: wrong(st) if c == 3 else None)  # the LAST call: one frame of 8 and the state
    _flagged(row, "h of the neighbouring row", lambda: R.check_calls(row, ref, crm, fb, log=QUIET), call=3)
    _flagged(row, "h of the neighbouring row (state rule)", lambda: R.check_state(row, ref, state, log=QUIET))


def test_two_slots_swapped_in_a_permuted_list():
    row = BY_WHY["permutation"]
    ref = R.reference_of(row)
    crm, fb, state = _as_device(row, ref)
    swapped = [c.copy() for c in crm]
    swapped[1][[4, 11]] = swapped[1][[11, 4]]  # the k = 3 call only
    _flagged(row, "two slots' mask rows swapped", lambda: R.check_calls(row, ref, swapped, fb, log=QUIET), call=1)
    rows = np.arange(row.F)
    for a in range(4):
        state["sb"][a] = state["sb"][a].copy()
        state["sb"][a][np.concatenate([4 * row.F + rows, 11 * row.F + rows])] = state["sb"][a][np.concatenate([11 * row.F + rows, 4 * row.F + rows])]
    _flagged(row, "two slots' records swapped", lambda: R.check_state(row, ref, state, log=QUIET))


def test_fp32_running_sums_miss_the_sum_rule_by_decades():
    row = BY_WHY["resumed"]
    ref = R.reference_of(row)
    _, _, state = _tampered(row, ref, None, carry_dtype=np.float32)
    ratios = R.check_sums(row, ref, state, log=QUIET, hold=False)
    assert ratios["fb_sum"] >= 1e3 and ratios["sb_sum rounding"] >= 1e3, ratios  # 2^-24 against (terms + 2) 2^-53
    _flagged(row, "fp32 running sums", lambda: R.check_sums(row, ref, state, log=QUIET))
    # ... and the reference's own fp64 carries, summed in another order than the exact sums, are inside it
    good = R.check_sums(row, ref, R.take_state(ref.state["64"], row.sel, row.F), log=QUIET)
    assert good["fb_sum"] <= 1.0 and good["sb_sum rounding"] <= 1.0


def test_segment_divisor_that_forgets_the_look_ahead_frames():
    row = BY_WHY["ends-inside-last"]
    ref = R.reference_of(row)
    crm, fb, _ = _tampered(row, ref, None, totals=[n - row.la for n in ref.totals])
    _flagged(row, "divisors over total - look_ahead frames", lambda: R.check_calls(row, ref, crm, None, log=QUIET))
    wrong_fb, wrong_sb = R.offline_divisors(ref.mag, np.concatenate(ref.fb["c32"], axis=-1), row.nb, [n - row.la for n in ref.totals], np.float32)
    with pytest.raises(AssertionError, match=re.escape(row.id) + ".*den_"):
        R.check_divisors(row, ref, wrong_fb, wrong_sb, np.concatenate(ref.fb["c32"], axis=-1), log=QUIET)
