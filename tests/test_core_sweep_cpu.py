"""The table, the reference and the checker of tests/test_gpu_core_sweep.py, tried on the CPU with stand-ins for the device.

* The written-out fp64 model agrees with O.fullsubnet_forward(dtype=float64) to 1e-14 of the mask's largest value (both
  norms, another neighbourhood).
* torch's fp32 run of the model as the "device" passes the checker, mask and fb_output, with a plan that has main and left-over
  rows and with two core calls.
* Deliberately wrong stand-ins - the fp32 cell emulation (the yardstick itself) with ONE thing wrong - FAIL it: the sub-band
  W_hh of layer 1 with its 8 low mantissa bits cleared in the left-over region only; one 16-row tile without b_hh; one utterance
  normalised by its neighbour's divisor; the left-over rows shifted by one tile; zero padding instead of reflect padding at the
  band edges; the look-ahead off by one frame; a stale last frame.  The full-band W_hh rounded to fp16 is caught on fb_output
  and is SILENT on the mask - both asserted: that is why the `fullband` rows exist.
* The table: ids unique, every path name present, the literals of every plan consistent (tiles cover the rows, main x rt + left
  = tiles, 4 clusters + aux = tiles), the two duplication conditions hold for every row, and - where the library's plan does not
  depend on kernel occupancies, which need a device - fsn_debug_core_call_plan reports the row's literals here too.
"""
import ctypes

import numpy as np
import pytest

import test_gpu_core_sweep as S
from oracle import fullsubnet_oracle as O

LA, NB, NORM = 2, 15, "offline"
ROW = S.Row("selftest", "rows", N=5 * 257, plan=S.P(81, 1, 64, 17))  # 5 utterances: main rows 0 .. 1023, left-over 1024 .. 1284
LEFT = 1024


@pytest.fixture(scope="module")
def ref():
    return S.reference_of(ROW)


def _batch(ref):
    return ref.mag[np.arange(ROW.B) % ROW.k]


def _calls(row=ROW):
    return list(zip(row.calls(), row.plans))


def _check(ref, got, row=ROW):
    return S.check_row(row, ref, got, _calls(row), log=lambda s: None)


def _flagged(ref, got, what, match=None):
    with pytest.raises(AssertionError, match=match):
        _check(ref, got)
        pytest.fail(f"'{what}' passed the checker", pytrace=False)


def _cell32(ref, params=None, rows=slice(None), sb_in=None, keep_frames=False):
    """The fp32 cell emulation of the sub-band stage on the batch (optionally other weights / another input), [n, 2, T]."""
    params = params or ref.params
    if sb_in is None:
        x, fb = S.fullband_stage(_batch(ref), params, LA, NORM, np.float32, "cell")
        sb_in = S.subband_input(x, fb, NB, NORM, np.float32)
    return S.subband_stage(sb_in[rows], params, 0 if keep_frames else LA, np.float32, "cell")


def _with(params, key, f):
    p = dict(params)
    p[key] = f(np.ascontiguousarray(params[key], dtype=np.float32).copy())
    return p


def _drop8(w):
    return (w.view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)


@pytest.mark.parametrize("norm,nb,la,T", [("offline", 15, 2, 4), ("cumulative", 15, 2, 5), ("offline", 7, 0, 1), ("cumulative", 0, 3, 4)])
def test_reference_agrees_with_the_oracle(norm, nb, la, T):
    params, mag = S.make_inputs(257, nb, 512, T, 2.0, 3)
    mine, fb = S.model(mag, params, la, nb, norm, np.float64, "torch")
    want, inter = O.fullsubnet_forward(mag, params, look_ahead=la, sb_num_neighbors=nb, norm_type=S.NORMS[norm], dtype=np.float64,
                                       return_intermediates=True)
    assert np.abs(S.rows_to_mask(mine, 3) - want).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(fb - inter["fb_output"][:, 0]).max() <= 1e-14 * np.abs(fb).max()


def test_torch_fp32_passes(ref):
    got = ref.rows("mask_t32", 0, ROW.N)
    rf, rm, wt = _check(ref, got)["mask"]
    assert rf <= 1.0 and wt <= 1.5  # torch's activations are no worse than the cell's formulas, tile by tile nearly so
    two = S.Row("selftest", "forward", B=5, chunks=[3, 2], plan=None)
    two.plans = [S.P(49, 1, 0, 49), S.P(33, 1, 0, 33)]
    _check(ref, got, two)
    fbrow = S.Row("selftest", "fullband", B=3)
    fbref = S.reference_of(fbrow)
    S.check_row(fbrow, fbref, fbref.fb_t32.copy(), _calls(fbrow), log=lambda s: None)
    # the cell emulation as the device: the ratio the issue measured (1.2 x at T = 4) stays far inside the margin on fb_output too
    _, fbc = S.model(fbref.mag, fbref.params, fbrow.la, fbrow.nb, fbrow.norm, np.float32, "cell", fb_only=True)
    S.check_row(fbrow, fbref, fbc, _calls(fbrow), log=lambda s: None)


def test_subband_whh_with_8_bits_cleared_in_the_leftover_rows(ref):
    wrong = _cell32(ref, _with(ref.params, "sb_model.sequence_model.weight_hh_l1", _drop8), rows=slice(LEFT, None))
    got = ref.rows("mask_c32", 0, ROW.N).copy()
    got[LEFT:] = wrong
    _flagged(ref, got, "W_hh of layer 1 without its 8 low mantissa bits, left-over rows", match="left-over rows")


def test_fullband_whh_in_fp16_is_caught_on_fb_output_and_silent_on_the_mask(ref):
    p16 = _with(ref.params, "fb_model.sequence_model.weight_hh_l0", lambda w: w.astype(np.float16).astype(np.float32))
    mask, fb = S.model(_batch(ref), p16, LA, NB, NORM, np.float32, "cell")
    # no Frobenius rule on the mask (whole tensor, frame, region, tile) sees the full-band stage: 1.8 x the yardstick.  The
    # whole tensor's max-error rule is left out here: the stand-in sits AT its margin (3.5 x by the issue's figures, 3.9 - 4.6 x
    # depending on the host's BLAS), so it neither catches it reliably nor lets it through reliably.
    rf, rm, _ = S.check_row(ROW, ref, mask, _calls(), log=lambda s: None, max_rule=False)["mask"]
    assert rf <= 2.5 and rm <= 8.0, (rf, rm)
    fbrow = S.Row("selftest", "fullband", B=3)
    fbref = S.reference_of(fbrow)
    _, fb = S.model(fbref.mag, _with(fbref.params, "fb_model.sequence_model.weight_hh_l0", lambda w: w.astype(np.float16).astype(np.float32)),
                    LA, NB, NORM, np.float32, "torch", fb_only=True)
    with pytest.raises(AssertionError, match="fb_output"):
        S.check_row(fbrow, fbref, fb, _calls(fbrow), log=lambda s: None)
        pytest.fail("the full-band W_hh in fp16 passed the checker on fb_output", pytrace=False)


def test_one_tile_without_b_hh(ref):
    zero = _with(ref.params, "sb_model.sequence_model.bias_hh_l0", np.zeros_like)
    got = ref.rows("mask_c32", 0, ROW.N).copy()
    got[160:176] = _cell32(ref, zero, rows=slice(160, 176))
    _flagged(ref, got, "one tile without b_hh", match="rows 160 .. 175")


def test_one_utterance_normalised_by_its_neighbours_divisor(ref):
    x, fb = S.fullband_stage(_batch(ref), ref.params, LA, NORM, np.float32, "cell")
    units = S.subband_units(x, fb, NB).astype(np.float32)
    mu = units.mean(axis=(1, 2, 3), dtype=np.float64).astype(np.float32)
    sb_in = O.offline_laplace_norm(units)
    sb_in[1] = units[1] / (mu[2] + np.float32(1e-5))
    got = _cell32(ref, sb_in=sb_in.reshape(ROW.N, 2 * NB + 2, -1))
    _flagged(ref, got, "utterance 1 divided by utterance 2's mean")


def test_leftover_rows_shifted_by_one_tile(ref):
    got = ref.rows("mask_c32", 0, ROW.N).copy()
    got[LEFT:] = np.roll(got[LEFT:], 16, axis=0)
    _flagged(ref, got, "left-over rows one tile late", match="left-over rows")


def test_zero_padding_instead_of_reflect_padding(ref):
    def unfold_zero(x, nb):
        B, C, F, T = x.shape
        xp = np.pad(x, [(0, 0), (0, 0), (nb, nb), (0, 0)])
        src = np.arange(F)[:, None] + np.arange(2 * nb + 1)[None, :]
        return np.ascontiguousarray(xp[:, :, src, :].transpose(0, 2, 1, 3, 4))

    x, fb = S.fullband_stage(_batch(ref), ref.params, LA, NORM, np.float32, "cell")
    sb_in = O.offline_laplace_norm(S.subband_units(x, fb, NB, unfold_zero)).reshape(ROW.N, 2 * NB + 2, -1)
    _flagged(ref, _cell32(ref, sb_in=sb_in), "zero padding at the band edges")


def test_look_ahead_off_by_one_frame(ref):
    full = _cell32(ref, keep_frames=True)
    _flagged(ref, np.ascontiguousarray(full[..., LA - 1:LA - 1 + ROW.T]), "look-ahead off by one frame")


def test_stale_last_frame(ref):
    got = ref.rows("mask_c32", 0, ROW.N).copy()
    got[..., -1] = got[..., -2]
    _flagged(ref, got, "a stale last frame")


def test_unwritten_rows_are_flagged(ref):
    got = ref.rows("mask_c32", 0, ROW.N).copy()
    got[700:716] = np.nan
    _flagged(ref, got, "a tile of NaN")


# ---- the table ----------------------------------------------------------------------------------------------------------

def test_table_ids_and_paths():
    ids = [r.id for r in S.TABLE]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    assert {r.path for r in S.TABLE} == set(S.PATHS), {r.path for r in S.TABLE} ^ set(S.PATHS)
    assert {r.entry for r in S.TABLE} == {"forward", "rows", "fullband"}


@pytest.mark.parametrize("row", S.TABLE, ids=[r.id for r in S.TABLE])
def test_row_literals_and_duplication(row):
    S.check_duplication(row, row.calls())
    assert row.k % 2 == 1 and row.k >= 3 or row.entry == "fullband"
    assert row.entry == "fullband" or -(-row.B // row.k) <= 16
    for (b_lo, Bs, r0, n, g0), plan in zip(row.calls(), row.plans):
        if row.entry == "fullband":
            continue
        assert plan is not None, f"no plan written for a core call of {Bs} utterances"
        assert 0 <= r0 < row.F and r0 + n <= Bs * row.F and g0 == b_lo * row.F + r0
        assert plan["tiles"] >= -(-n // 16) and (plan["tiles"] == -(-n // 16) or plan["left_tiles"] == 0)  # padding tiles: whole rounds only
        if plan["main_wgs"]:
            assert plan["main_wgs"] * plan["rt"] + plan["left_tiles"] == plan["tiles"]
        else:
            assert plan["left_tiles"] == plan["tiles"]
        if plan["regime"] == "group":
            assert 4 * plan["grp_clusters"] + plan["grp_aux_tiles"] == plan["tiles"] and plan["grp_clusters"] <= 2 * S.SLOTS
        regions = S.regions_of(plan, n)
        assert not regions or (regions[0][1] == 0 and regions[-1][2] == n)


@pytest.mark.parametrize("row", [r for r in S.TABLE if r.entry != "fullband"], ids=[r.id for r in S.TABLE if r.entry != "fullband"])
def test_library_reports_the_rows_persistent_plan(row):
    """Which rows the group kernel and the chain take depends on compiled occupancies (none without a device); the row-tile plan
    of the persistent pair does not, outside the 224 - 264 tiles that the two-cluster group kernel takes from it."""
    from fullsubnet_amd import _lib
    cfg = row.cfg(_lib)
    for (b_lo, Bs, r0, n, g0), plan in zip(row.calls(), row.plans):
        got = _lib.core_call_plan(cfg, row.B, row.T, row.begin, row.begin + row.N) if row.entry == "rows" else _lib.core_call_plan(cfg, Bs, row.T)
        assert got["rows"] == n and got["kin_chunks"] == S.ru16(2 * row.nb + 2) // 16 and got["npad_fb"] == S.ru16(Bs)
        if plan["regime"] == "group" and plan["tiles"] >= 224:
            continue
        keys = ("tiles", "npad", "rt", "main_wgs", "left_tiles") + (("fc_fused", "l1x") if plan["main_wgs"] else ())
        assert {k: got[k] for k in keys} == {k: plan[k] for k in keys}, (got, plan)
        if plan["regime"] == "persistent":
            assert (got["cu_tiles"], got["aux_tiles"]) == (plan["cu_tiles"], plan["aux_tiles"])


def test_core_call_plan_arguments():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    cfg = _lib.Cfg(257, 2, 15, 512, 384, 0, 0)
    buf = (ctypes.c_int * 15)()
    c = ctypes.byref(cfg)
    assert L.fsn_debug_core_call_plan(c, 8, 4, 0, -1, buf, 15) == 0 and buf[0] == 8 * 257
    assert L.fsn_debug_core_call_plan(c, 8, 4, 300, 400, buf, 15) == 0 and (buf[0], buf[11]) == (100, 16)  # one utterance touched
    assert L.fsn_debug_core_call_plan(c, 8, 4, 0, -1, buf, 14) == -1
    assert L.fsn_debug_core_call_plan(c, 8, 4, 0, 8 * 257 + 1, buf, 15) == -1
    assert L.fsn_debug_core_call_plan(c, 8, 4, 5, 5, buf, 15) == -1
    assert L.fsn_debug_core_call_plan(c, 0, 4, 0, -1, buf, 15) == -1
    # the row-range entries size their workspace from the same dims
    assert L.fsn_fullsubnet_rows_workspace_bytes(c, 8, 4, 0, 8 * 257) == L.fsn_fullsubnet_workspace_bytes(c, 8, 4)
    assert isinstance(L.fsn_debug_core_last_launches(), int)
