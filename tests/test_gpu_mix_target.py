"""fsn_rir_shorten / fsn_mix_pairs_target and the loader's dereverberation targets on the device, held to the reference's
own windows (tests/golden/rts_windows.npz) and to the fp64 port (tests/mix_target_reference.py).

Taps: idx exact; out and win within 2^-22 |ref| + 2^-126 of the golden (one fp32 ulp of the window for an fp64 10^x that
differs from numpy's in the last place, half an ulp of the product, the floor for a product flushed in the denormal
range); the elements that are not bit-equal are counted and printed (a PCM slab has no negative zero: the seven taps
that are -0 in the fp32 responses come back as +0 from it and are counted).  Target rows: within what the mix sweep allows
`clean` on that row plus 2^-22 s conv(|x|, |h_s|)[n], the tap allowance carried through the convolution.  noisy and
clean: the bits of fsn_mix_pairs.  Outputs and workspaces are NaN before every call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_reference as R  # noqa: E402
import mix_target_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu
L = R.MIX_L


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def nan_bytes(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")


def rir_shorten(hs, descs, fmt, ld):
    """fsn_rir_shorten on the responses `hs` (PCM-valued fp32) in a slab of format `fmt`; descs: (q, after_max, mode) per
    row.  (out [B, ld], win [B, ld], idx [B]) as numpy arrays."""
    from fullsubnet_amd import _lib, mix
    B = len(hs)
    slab, off, lens = mix._to_slab(hs, fmt)
    tab = np.zeros(B, mix.TARGET_DTYPE)
    for b, d in enumerate(descs):
        tab[b] = d
    d_slab = torch.from_numpy(slab).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    d_tab = torch.from_numpy(tab.view(np.uint8)).cuda()
    out, win = torch.full((B, ld), float("nan"), device="cuda"), torch.full((B, ld), float("nan"), device="cuda")
    idx = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().fsn_rir_shorten(d_slab.data_ptr(), mix.SLAB_FORMATS[fmt], d_off.data_ptr(), d_len.data_ptr(), B,
                                          int(lens.max()), d_tab.data_ptr(), out.data_ptr(), ld, win.data_ptr(),
                                          idx.data_ptr(), _lib.stream_ptr()))
    return out.cpu().numpy(), win.cpu().numpy(), idx.cpu().numpy()


def tables(bank, items, room=(512, 16 * 32)):
    """The three descriptor tables of `items` in one byte block: items at 0, segments at room[0], targets behind them."""
    from fullsubnet_amd import mix
    tab, seg_tab, n_segs, longest = mix.pack_items(bank, items, L)
    tgt = mix.pack_targets(items)
    seg_at, tgt_at = room[0], room[0] + room[1]
    assert tab.nbytes <= seg_at and seg_tab.nbytes <= room[1]
    raw = np.zeros(tgt_at + tgt.nbytes, np.uint8)
    raw[:tab.nbytes] = tab.view(np.uint8)
    raw[seg_at:seg_at + seg_tab.nbytes] = seg_tab.view(np.uint8)
    raw[tgt_at:] = tgt.view(np.uint8)
    return torch.from_numpy(raw), seg_at, n_segs, tgt_at, longest


def pairs_target(bank, items, ws_rir_len=None, want_clean=True):
    """fsn_mix_pairs_target into NaN outputs with a NaN workspace sized for responses of ws_rir_len (None: the batch's
    longest): (noisy, clean or None, target) as numpy arrays."""
    from fullsubnet_amd import _lib, mix
    B = len(items)
    raw, seg_at, n_segs, tgt_at, longest = tables(bank, items)
    desc = raw.cuda()
    noisy, clean, target = (torch.full((B, L), float("nan"), device="cuda") for _ in range(3))
    nbytes = _lib.lib().fsn_mix_target_workspace_bytes(B, L, longest if ws_rir_len is None else ws_rir_len)
    assert nbytes > 0
    ws = nan_bytes(nbytes)
    mix.mix_pairs_target(bank, desc, seg_at, n_segs, tgt_at, noisy, clean if want_clean else None, target, ws)
    torch.cuda.synchronize()
    return noisy.cpu().numpy(), clean.cpu().numpy() if want_clean else None, target.cpu().numpy()


def pairs(bank, items, ws_rir_len=None):
    """fsn_mix_pairs on the same descriptors, the same way."""
    from fullsubnet_amd import _lib, mix
    B = len(items)
    raw, seg_at, n_segs, _, longest = tables(bank, items)
    desc = raw.cuda()
    noisy, clean = (torch.full((B, L), float("nan"), device="cuda") for _ in range(2))
    ws = nan_bytes(_lib.lib().fsn_mix_workspace_bytes(B, L, longest if ws_rir_len is None else ws_rir_len))
    mix.mix_pairs(bank, desc, seg_at, n_segs, noisy, clean, ws)
    torch.cuda.synchronize()
    return noisy.cpu().numpy(), clean.cpu().numpy()


@pytest.fixture(scope="module")
def banks(fsn):
    lists = R.mix_sources()
    return {fmt: fsn.MixBank(*lists, "cuda", fmt=fmt) for fmt in ("f32", "i16")}, lists


@pytest.fixture(scope="module")
def sweep(fsn, banks):
    """One call per slab format on the eight rows of the sweep, next to fsn_mix_pairs on the same descriptors."""
    by_fmt, lists = banks
    items = T.sweep_items()
    descs = [it for _, it in items]
    got = {fmt: pairs_target(by_fmt[fmt], descs) for fmt in by_fmt}
    old = {fmt: pairs(by_fmt[fmt], descs) for fmt in by_fmt}
    return items, lists, got, old


# ---- fsn_rir_shorten ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "i16"])
@pytest.mark.parametrize("ld", [6000, 6001])
def test_rir_shorten_on_the_golden_responses(fsn, golden_dir, fmt, ld):
    """Every golden response in one call: rows of whole 16-byte words (ld = 6000) and not (6001); in the slab the
    responses follow one another, so most of them start off a 16-byte boundary and the first one on it."""
    cases = T.golden_cases(golden_dir)
    out, win, idx = rir_shorten([c["h"] for c in cases], [(c["q"], c["after_max"], 1) for c in cases], fmt, ld)
    differ = {c["name"]: T.check_shorten(c, out[b], win[b], idx[b]) for b, c in enumerate(cases)}
    print(f"{fmt} ld {ld}: elements not bit-equal to the reference (out + win): {differ}")


def test_rir_shorten_modes_and_an_unknown_mode(fsn, golden_dir):
    cases = T.golden_cases(golden_dir)
    by = {c["name"]: c for c in cases}
    rows = [by["len4097_speechlike"], by["len6000_peak_at_5000"], by["len4097_two_equal_peaks"], by["len1"]]
    for mode in (0, 2):
        out, win, idx = rir_shorten([c["h"] for c in rows], [(c["q"], c["after_max"], mode) for c in rows], "i16", 6000)
        for b, c in enumerate(rows):
            want_out, want_win, want_idx = T.rts_window(c["h"], c["q"], c["after_max"], mode)
            n = len(c["h"])
            assert idx[b] == want_idx and np.array_equal(out[b, :n], want_out) and np.array_equal(win[b, :n], want_win)
            assert not out[b, n:].any() and not win[b, n:].any()
    out, win, idx = rir_shorten([c["h"] for c in rows], [(c["q"], c["after_max"], m) for c, m in zip(rows, (1, 3, -1, 1))],
                                "f32", 6000)
    for b, c in enumerate(rows):  # a mode the device does not know: NaN over the response, never a silent choice
        n = len(c["h"])
        if b in (1, 2):
            assert np.isnan(out[b, :n]).all() and np.isnan(win[b, :n]).all() and not out[b, n:].any()
        else:
            T.check_shorten(c, out[b], win[b], idx[b])


def test_python_mirror_of_the_reference_function(fsn, golden_dir):
    cases = T.golden_cases(golden_dir)
    for c in cases:  # the reference's signature, a 1-D response
        rir, win = fsn.reverberation_time_shortening(torch.from_numpy(c["h"]).cuda(), **c["kw"])
        assert rir.shape == win.shape == (len(c["h"]),) and rir.is_cuda and rir.dtype == torch.float32
        T.check_shorten(c, rir.cpu().numpy(), win.cpu().numpy(), T.first_argmax_abs(c["h"]))
    # the extension: a 2-D batch with a T60 pair per row, against the restatement (row 0 is a golden case as it stands)
    by = {c["name"]: c for c in cases}
    hs = [by["len4097_speechlike"]["h"], by["len4097_two_equal_peaks"]["h"], by["len4097_speechlike"]["h"]]
    orig, tgt = [0.6, 1.2, 0.9], [0.15, 0.3, 0.05]
    rir, win = fsn.reverberation_time_shortening(torch.from_numpy(np.stack(hs)).cuda(), orig, tgt, sr=16000)
    assert rir.shape == win.shape == (3, 4097)
    for b, h in enumerate(hs):
        q, after_max = T.host_descriptor(orig[b], tgt[b], 16000, 0.002)
        want_rir, want_win, want_idx = T.rts_window(h, q, after_max)
        T.check_shorten(dict(name=f"row {b}", h=h, rir=want_rir, win=want_win), rir[b].cpu().numpy(), win[b].cpu().numpy(),
                        want_idx)
    assert np.array_equal(T.rts_window(hs[0], *T.host_descriptor(0.6, 0.15, 16000, 0.002))[1], by["len4097_speechlike"]["win"])
    with pytest.raises(fsn._lib.FsnError):
        fsn.reverberation_time_shortening(torch.zeros(8), 0.6, 0.15)  # a host tensor: there is no CPU path


# ---- fsn_mix_pairs_target ---------------------------------------------------------------------------------------------------
def test_noisy_and_clean_keep_the_bits_of_mix_pairs(fsn, sweep, banks):
    items, lists, got, old = sweep
    for fmt in got:
        noisy, clean, target = (torch.from_numpy(a) for a in got[fmt])
        assert torch.equal(noisy, torch.from_numpy(old[fmt][0])) and torch.equal(clean, torch.from_numpy(old[fmt][1])), fmt
        assert torch.isfinite(noisy).all() and torch.isfinite(clean).all() and torch.isfinite(target).all()
        exact = [b for b, (_, it) in enumerate(items) if T.effective_mode(it) == 0]
        assert len(exact) == 2 and any(items[b][1].rir_index >= 0 for b in exact) and any(items[b][1].rir_index < 0 for b in exact)
        for b, (name, it) in enumerate(items):
            same = torch.equal(target[b], clean[b])
            assert same == (b in exact or name == "shortened_silence"), (fmt, name)
    for a, b in zip(got["f32"], got["i16"]):
        assert np.array_equal(a, b)  # the sources are 16-bit PCM values in both banks
    # clean = NULL: the other two outputs do not change
    by_fmt, _ = banks
    noisy, none, target = pairs_target(by_fmt["i16"], [it for _, it in items], want_clean=False)
    assert none is None and np.array_equal(noisy, got["i16"][0]) and np.array_equal(target, got["i16"][2])


def test_target_rows_against_the_fp64_port(fsn, sweep):
    """Worst error / allowance over the shortened and early rows is printed (profiles/mix_pairs.md states it)."""
    items, lists, got, _ = sweep
    noisy, clean, target = got["f32"]
    ratios = {}
    for b, (name, it) in enumerate(items):
        n64, c64, t64, allow, mode = T.target_rows(it, *lists, L)
        if mode == 0:
            continue
        if name == "shortened_silence":
            assert not target[b].any() and not noisy[b].any() and not clean[b].any()  # digital silence: exact zeros
            continue
        ratios[name] = T.check_target(name, target[b], t64, allow)
    assert len(ratios) == 5
    print("target rows, worst error / allowance: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def test_edge_rows(fsn):
    """An all-zero response gives exact zeros; a response longer than the workspace's transform gives NaN in all three
    outputs and leaves the other rows alone; the same descriptor gives the same bits in row 0 of a batch of 1 and in row
    5 of a batch of 8."""
    import dataclasses
    clean, noise, rir = R.mix_sources()
    rng = np.random.default_rng(5)
    long_rir = R.pcm(0.5 * rng.standard_normal(5000) * np.exp(-np.arange(5000) / 900.0))
    rir = rir + [np.zeros(100, np.float32), long_rir]
    bank = fsn.MixBank(clean, noise, rir, "cuda", fmt="i16")
    items = dict(T.sweep_items())
    probe = items["shortened_1d"]
    zero_h = dataclasses.replace(probe, rir_index=2)
    too_long = dataclasses.replace(probe, rir_index=3)
    batch = [items["early_2d"], zero_h, too_long, items["dry_asks_for_shortened"], items["shortened_2d_clipped"], probe,
             items["q_not_positive"], dataclasses.replace(too_long, target_mode=0)]
    # 4097 + 800 - 1 <= 8192 < 4097 + 4097 - 1: the transform of an 800-tap batch cannot carry the 5000-tap response
    noisy, cl, target = pairs_target(bank, batch, ws_rir_len=800)
    assert not noisy[1].any() and not cl[1].any() and not target[1].any()
    for b in (2, 7):
        assert np.isnan(noisy[b]).all() and np.isnan(cl[b]).all() and np.isnan(target[b]).all()
    rest = [b for b in range(8) if b not in (2, 7)]
    assert np.isfinite(noisy[rest]).all() and np.isfinite(cl[rest]).all() and np.isfinite(target[rest]).all()
    n1, c1, t1 = pairs_target(bank, [probe], ws_rir_len=800)
    assert np.array_equal(n1[0], noisy[5]) and np.array_equal(c1[0], cl[5]) and np.array_equal(t1[0], target[5])
    # with a transform for it the long response is carried: arg-max over the whole response, taps up to L
    n2, c2, t2 = pairs_target(bank, [too_long, probe])
    assert np.isfinite(t2).all() and not np.array_equal(t2[0], c2[0])
    lists = (clean, noise, rir)
    for b, it in enumerate([too_long, probe]):
        _, _, t64, allow, _ = T.target_rows(it, *lists, L)
        T.check_target(f"row {b}", t2[b], t64, allow)
    # a workspace without a transform: rows with a response are NaN, the dry one is copied and levelled
    n3, c3, t3 = pairs_target(bank, [probe, items["dry_asks_for_shortened"]], ws_rir_len=0)
    assert np.isnan(n3[0]).all() and np.isnan(t3[0]).all() and np.isfinite(n3[1]).all() and np.array_equal(t3[1], c3[1])


def test_mix_pairs_target_is_capturable_in_a_hip_graph(fsn, banks):
    """Captured once, a replay mixes whatever descriptors the static tables hold then, bit-identical to the eager call: a
    reverberant shortened row among dry ones, then other rows."""
    from fullsubnet_amd import _lib, mix
    by_fmt, _ = banks
    bank = by_fmt["i16"]
    items = dict(T.sweep_items())
    dry = items["dry_asks_for_shortened"]
    first = [dry, items["shortened_1d"], dry, dry]
    second = [items["early_2d"], dry, items["shortened_2d_clipped"], items["q_not_positive"]]
    eager = [pairs_target(bank, rows, ws_rir_len=800) for rows in (first, second)]
    (t1, seg_at, n1, tgt_at, _), (t2, _, n2, _, _) = tables(bank, first), tables(bank, second)
    desc = t1.cuda()
    noisy, clean, target = (torch.empty(4, L, device="cuda") for _ in range(3))
    ws = nan_bytes(_lib.lib().fsn_mix_target_workspace_bytes(4, L, 800))
    n_segs = max(n1, n2)
    call = lambda: mix.mix_pairs_target(bank, desc, seg_at, n_segs, tgt_at, noisy, clean, target, ws)  # noqa: E731
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for tab, want in ((t2, eager[1]), (t1, eager[0])):
        desc.copy_(tab)
        for t in (noisy, clean, target):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip((noisy, clean, target), want):
            assert np.array_equal(got.cpu().numpy(), ref)


# ---- the loader -------------------------------------------------------------------------------------------------------------
def test_loader_yields_targets(fsn):
    rng = np.random.default_rng(3)
    Ls = 2560
    clean = [R.pcm(0.2 * rng.standard_normal(n)) for n in (3000, 2560, 2000, 4000, 2700, 3100, 2900, 2561) * 2]
    noise = [R.pcm(0.05 * rng.standard_normal(n)) for n in (5000, 900, 1500)]
    r2 = rng.standard_normal((2, 200)) * np.exp(-np.arange(200) / 30.0)
    rir = [R.pcm(0.5 * np.exp(-np.arange(600) / 80.0) * rng.standard_normal(600)), R.pcm(0.8 * r2 / np.abs(r2).max())]
    t60 = [80 * np.log(1000) / 16000, [30 * np.log(1000) / 16000, 0.005]]  # the second row of the 2-D one: below the target
    with pytest.raises(ValueError):
        fsn.MixLoader(fsn.MixBank(clean, noise, rir, "cuda", fmt="i16"), fsn.MixConfig(target="shortened"), 4, seed=9)
    bank = fsn.MixBank(clean, noise, rir, "cuda", fmt="i16", rir_t60=t60)
    cfg = lambda target: fsn.MixConfig(sr=16000, sub_sample_length=0.16, silence_length=0.02, target=target,  # noqa: E731
                                       target_T60=0.01)
    assert cfg("shortened").samples == Ls
    new = lambda target: fsn.MixLoader(bank, cfg(target), batch_size=8, seed=9)  # noqa: E731
    assert len(new("shortened")) == 2
    plain = [(n.clone(), c.clone()) for n, c in new("reverberant")]
    modes_seen = set()
    for target in ("shortened", "early"):
        first = [(n.clone(), t.clone()) for n, t in new(target)]
        again = [(n.clone(), t.clone()) for n, t in new(target)]
        draws = list(new(target).draws())
        assert draws == list(new(target).draws()) and len(draws) == len(first) == 2
        for (n, t), (n2, t2), (pn, pc), items in zip(first, again, plain, draws):
            assert n.shape == t.shape == (8, Ls) and t.is_cuda and torch.isfinite(t).all()
            assert torch.equal(n, n2) and torch.equal(t, t2)      # the same seed: identical batches
            assert torch.equal(n, pn)                             # noisy does not depend on the target
            modes = fsn.mix.pack_targets(items)["mode"].tolist()
            assert [not torch.equal(t[b], pc[b]) for b in range(8)] == [m != 0 for m in modes], (target, modes)
            modes_seen |= {(target, m) for m in modes}
    assert {("shortened", 0), ("shortened", 1), ("early", 0), ("early", 2)} <= modes_seen
