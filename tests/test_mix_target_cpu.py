"""Dereverberation targets, the parts that need no device: the fp64 restatement of the window (tests/mix_target_reference.py)
against the reference's own outputs (tests/golden/rts_windows.npz), the target table of the loader, draw_item's unchanged
draws, struct layouts, header = exports = bindings, the refusals of the new entries, and every checker of
tests/test_gpu_mix_target.py against a wrong stand-in it must reject."""
import ctypes
import dataclasses
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_reference as R  # noqa: E402
import mix_target_reference as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsn_rir_shorten", "fsn_mix_target_workspace_bytes", "fsn_mix_pairs_target")


@pytest.fixture(scope="module")
def cases(golden_dir):
    return T.golden_cases(golden_dir)


def test_restatement_equals_the_reference_bit_for_bit(cases):
    names = {c["name"] for c in cases}
    assert {len(c["h"]) for c in cases} == {1, 2, 33, 513, 4097, 6000} and len(cases) >= 8
    for c in cases:
        out, win, idx = T.rts_window(c["h"], c["q"], c["after_max"])
        assert idx == int(np.argmax(np.abs(c["h"]))), c["name"]
        assert np.array_equal(win.view(np.uint32), c["win"].view(np.uint32)), c["name"]
        assert np.array_equal(out.view(np.uint32), c["rir"].view(np.uint32)), c["name"]
        assert T.check_shorten(c, out, win, idx) == 0
    # the cases are what they are named after
    by = {c["name"]: c for c in cases}
    assert by["len2_negative_peak"]["h"][1] < 0 and T.first_argmax_abs(by["len2_negative_peak"]["h"]) == 1
    assert T.first_argmax_abs(by["len33_peak_at_0"]["h"]) == 0 and T.first_argmax_abs(by["len513_peak_at_last"]["h"]) == 512
    two = by["len4097_two_equal_peaks"]["h"]
    assert abs(two[100]) == abs(two[2000]) == np.abs(two).max() and T.first_argmax_abs(two) == 100
    assert T.first_argmax_abs(by["len6000_peak_at_5000"]["h"]) == 5000 > R.MIX_L
    for name in ("len33_n1_past_the_end", "len513_peak_at_last"):
        assert (by[name]["win"] == 1).all() and np.array_equal(by[name]["rir"], by[name]["h"]), name
    w = by["len6000_huge_q"]["win"]
    assert ((w > 0) & (w < np.float32(2.0 ** -126))).sum() >= 10 and (w[300:] == 0).all(), "through the denormals to zero"
    assert {(c["kw"]["sr"], c["after_max"]) for c in cases} == {(16000, 32), (48000, 96)}
    assert "len1" in names


def test_early_window_is_the_shortened_one_cut_off(cases):
    for c in cases:
        out, win, idx = T.rts_window(c["h"], 0.0, c["after_max"], mode=2)
        n1 = idx + c["after_max"]
        assert (win[:n1] == 1).all() and not win[n1:].any() and np.array_equal(out[:n1], c["h"][:n1]) and not out[n1:].any()
        out0, win0, _ = T.rts_window(c["h"], c["q"], c["after_max"], mode=0)
        assert (win0 == 1).all() and np.array_equal(out0, c["h"])


# ---- wrong stand-ins ------------------------------------------------------------------------------------------------------
def test_shorten_checker_rejects_the_last_tie_and_a_window_from_the_peak(cases):
    by = {c["name"]: c for c in cases}
    c = by["len4097_two_equal_peaks"]

    def last_argmax_window(h, q, after_max):  # arg-max taking the LAST tie
        a = np.abs(h)
        idx = len(a) - 1 - int(np.argmax(a[::-1]))
        win = np.ones(len(h))
        win[idx + after_max:] = 10.0 ** (-q * np.arange(len(h) - idx - after_max))
        win = win.astype(np.float32)
        return h * win, win, idx

    out, win, idx = last_argmax_window(c["h"], c["q"], c["after_max"])
    assert idx == 2000
    with pytest.raises(AssertionError):
        T.check_shorten(c, out, win, idx)
    with pytest.raises(AssertionError):  # ... even when it reports the right index
        T.check_shorten(c, out, win, 100)
    # the window starting at idx rather than N1 = idx + after_max
    for name in ("len4097_speechlike", "len6000_peak_at_5000"):
        c = by[name]
        out, win, idx = T.rts_window(c["h"], c["q"], 0)
        with pytest.raises(AssertionError):
            T.check_shorten(c, out, win, idx)
    # one ulp of the window passes, two do not; a non-zero behind the response does not
    c = by["len4097_speechlike"]
    out, win, idx = T.rts_window(c["h"], c["q"], c["after_max"])
    up = np.nextafter(win, np.float32(2))
    assert T.check_shorten(c, c["h"] * up, up, idx) > 0
    up2 = np.nextafter(np.nextafter(up, np.float32(2)), np.float32(2))
    with pytest.raises(AssertionError):
        T.check_shorten(c, c["h"] * up2, up2, idx)
    with pytest.raises(AssertionError):
        T.check_shorten(c, np.append(out, np.float32(1e-30)), np.append(win, np.float32(0)), idx)


@pytest.fixture(scope="module")
def sweep():
    lists = R.mix_sources()
    items = T.sweep_items()
    return lists, items, {name: T.target_rows(it, *lists, R.MIX_L) for name, it in items}


def test_sweep_rows_cover_what_they_are_named_after(sweep):
    lists, items, refs = sweep
    assert 6 <= len(items) <= 8
    modes = {name: refs[name][4] for name, _ in items}
    assert modes == dict(shortened_1d=1, early_2d=2, dry_asks_for_shortened=0, shortened_2d_clipped=1, q_not_positive=0,
                         shortened_silence=1, huge_q_short_clean=1, early_clean_len_1=2)
    for name, it in items:
        noisy, clean, target, allow, mode = refs[name]
        if mode == 0:
            assert target is clean
        elif name == "shortened_silence":
            assert not target.any() and not clean.any()
        else:  # the target is a different signal, at the clean row's gain: it is the clean row's early part and a shorter tail
            assert np.abs(target - clean).max() > 1e-3 * np.abs(clean).max(), name
            assert np.dot(target, target) < np.dot(clean, clean), name
    clipped = {name: abs(np.abs(refs[name][0]).max() - (0.99 - R.EPS)) < 1e-6 for name, _ in items}
    assert clipped["shortened_2d_clipped"] and not clipped["shortened_1d"]


def test_target_checker_rejects_a_target_levelled_by_its_own_peak(sweep):
    lists, items, refs = sweep
    clean, noise, rir = lists
    for name, it in items:
        noisy, cl, target, allow, mode = refs[name]
        if mode == 0 or not target.any():
            continue
        assert T.check_target(name, target.astype(np.float32), target, allow) <= 1.0  # its own fp32 rounding passes
        c, n = R.rows_of(it, clean, noise, R.MIX_L)
        hs, _, _ = T.rts_window(R.rir_of(it, rir), it.target_q, it.target_after_max, mode)
        _, own, _ = R.snr_mix(c, n, it.snr, it.target_dB_FS, it.noisy_target_dB_FS, hs, R.EPS, np.float64)
        with pytest.raises(AssertionError):  # snr_mix on the shortened response: every scalar from the shortened row
            T.check_target(name, own, target, allow)
        with pytest.raises(AssertionError):  # the reverberant row itself is no target either
            T.check_target(name, cl, target, allow)
        # ... nor is a target from taps whose window starts at the peak
        h0, _, _ = T.rts_window(R.rir_of(it, rir), it.target_q, 0, mode)
        if not np.array_equal(h0, hs):
            wrong = target * 0 + R.fft_conv(c, h0) * (np.abs(target).max() / max(np.abs(R.fft_conv(c, hs)).max(), 1e-300))
            with pytest.raises(AssertionError):
                T.check_target(name, wrong, target, allow)


# ---- the loader's host side -------------------------------------------------------------------------------------------------
def test_target_table_and_the_mode_0_rule():
    from fullsubnet_amd import _lib, mix
    assert 0.002 * 16000 == 32 and 0.002 * 48000 == 96
    cfg = lambda **kw: mix.MixConfig(**kw)  # noqa: E731
    assert mix.target_of(cfg()) == (0, 0.0, 0) and mix.target_of(cfg(), 0.6) == (0, 0.0, 0)
    assert mix.target_of(cfg(target="shortened"), 0.6) == (1, 3 / (0.15 * 16000) - 3 / (0.6 * 16000), 32)
    assert mix.target_of(cfg(target="shortened", sr=48000, target_T60=0.3), 1.2) == (1, 3 / (0.3 * 48000) - 3 / (1.2 * 48000), 96)
    assert mix.target_of(cfg(target="shortened"), 0.6)[1] == T.host_descriptor(0.6, 0.15, 16000, 0.002)[0]
    for t60 in (0.15, 0.1):  # q <= 0 would lengthen the tail: the reverberant row stays
        assert mix.target_of(cfg(target="shortened"), t60) == (0, 0.0, 0)
    assert mix.target_of(cfg(target="early", time_after_max=0.001)) == (2, 0.0, 16)
    with pytest.raises(ValueError):
        mix.target_of(cfg(target="shortened"), None)
    with pytest.raises(ValueError):
        cfg(target="dry")
    base = R.mix_cases()[1][1]
    assert base.rir_index >= 0 and (base.target_mode, base.target_q, base.target_after_max) == (0, 0.0, 0)
    rows = [dataclasses.replace(base, target_mode=1, target_q=0.00075, target_after_max=32),
            dataclasses.replace(base, target_mode=1, target_q=0.0, target_after_max=32),       # q <= 0
            dataclasses.replace(base, target_mode=1, target_q=-0.001, target_after_max=32),
            dataclasses.replace(base, target_mode=2, target_q=0.5, target_after_max=96),       # early: q is not read
            dataclasses.replace(base, rir_index=-1, target_mode=1, target_q=0.00075, target_after_max=32),  # dry
            base]
    tab = mix.pack_targets(rows)
    assert tab.dtype.itemsize == 16 and tab["mode"].tolist() == [1, 0, 0, 2, 0, 0]
    assert tab["q"].tolist() == [0.00075, 0.0, 0.0, 0.0, 0.0, 0.0] and tab["after_max"].tolist() == [32, 0, 0, 96, 0, 0]
    assert [T.effective_mode(it) for it in rows] == tab["mode"].tolist()
    for bad in (dict(target_mode=3), dict(target_mode=-1), dict(target_mode=1, target_q=0.1, target_after_max=-1)):
        with pytest.raises(_lib.FsnError, match="outside 0 - 2|target_after_max"):
            mix.pack_targets([dataclasses.replace(base, **bad)])


def test_draws_do_not_depend_on_the_target(golden_dir):
    """draw_item issues the reference's random calls in the reference's order under every `target`: the logs recorded from
    Dataset.__getitem__ (tests/golden/mix_items.npz) hold, and only the target fields of the descriptors differ."""
    from fullsubnet_amd.mix import MixConfig, draw_item, rir_t60_rows
    (clean, noise, rir), _, meta = R.golden_sources(golden_dir)
    a = meta["args"]
    z = np.load(os.path.join(golden_dir, "mix_items.npz"))
    ref_logs = json.loads(str(z["logs"]))
    tables = R.HostTables(clean, noise, rir)
    t60 = [0.6, 0.1, 0.9, [0.6, 0.1, 0.6]]
    assert len(t60) == len(rir) and np.ndim(rir[3]) == 2
    tables.rir_t60 = rir_t60_rows(rir, t60)
    seen, plain = set(), None
    for target in ("reverberant", "shortened", "early"):
        cfg = MixConfig(sr=a["sr"], sub_sample_length=a["sub_sample_length"], silence_length=a["silence_length"],
                        snr_range=tuple(a["snr_range"]), reverb_proportion=a["reverb_proportion"],
                        target_dB_FS=a["target_dB_FS"], target_dB_FS_floating_value=a["target_dB_FS_floating_value"],
                        target=target)
        drawn = []
        for i, (ps, ns) in enumerate(z["seeds"]):
            log = []
            rnd = R.LoggedRandom(int(ps), int(ns), log)
            drawn.append(draw_item(i, tables, cfg, rnd, rnd))
            assert log == ref_logs[i], (target, i)
        strip = [dataclasses.replace(it, target_mode=0, target_q=0.0, target_after_max=0) for it in drawn]
        plain = strip if plain is None else plain
        assert strip == plain
        for it in drawn:
            if it.rir_index < 0 or target == "reverberant":
                assert (it.target_mode, it.target_q, it.target_after_max) == (0, 0.0, 0)
            elif target == "early":
                assert (it.target_mode, it.target_after_max) == (2, int(0.002 * a["sr"]))
            else:
                orig = float(tables.rir_t60[it.rir_index][it.rir_row])
                want = (1, 3 / (0.15 * a["sr"]) - 3 / (orig * a["sr"]), int(0.002 * a["sr"])) if orig > 0.15 else (0, 0.0, 0)
                assert (it.target_mode, it.target_q, it.target_after_max) == want
            seen.add((target, it.target_mode))
    assert {("shortened", 0), ("shortened", 1), ("early", 2), ("early", 0)} <= seen
    tables.rir_t60 = None
    with pytest.raises(ValueError, match="rir_t60"):
        for i in range(len(z["seeds"])):
            draw_item(i, tables, MixConfig(sr=a["sr"], sub_sample_length=a["sub_sample_length"], target="shortened",
                                           reverb_proportion=1.0), *(R.LoggedRandom(1, 1, []),) * 2)
    with pytest.raises(ValueError):
        rir_t60_rows(rir, t60[:3])
    with pytest.raises(ValueError):
        rir_t60_rows(rir, [0.6, 0.1, 0.9, [0.6, 0.1]])


def test_loader_refuses_shortened_without_t60():
    from fullsubnet_amd.mix import MixConfig, MixLoader
    bank = R.HostTables(*R.mix_sources())
    bank.__class__ = type("Tables", (R.HostTables,), {"__len__": lambda self: 23})
    bank.rir_len = np.asarray([800, 300])
    with pytest.raises(ValueError, match="rir_t60"):
        MixLoader(bank, MixConfig(sub_sample_length=0.25, target="shortened"), 4, seed=5)
    for target in ("reverberant", "early"):
        assert MixLoader(bank, MixConfig(sub_sample_length=0.25, target=target), 4, seed=5).max_rir_len == 800


# ---- the C side -----------------------------------------------------------------------------------------------------------
def test_struct_layouts():
    from fullsubnet_amd import mix

    class Target(ctypes.Structure):  # fsn_mix_target as a C compiler lays it out
        _fields_ = [("q", ctypes.c_double), ("after_max", ctypes.c_int), ("mode", ctypes.c_int)]

    assert ctypes.sizeof(Target) == 16 == mix.TARGET_DTYPE.itemsize and mix.ITEM_DTYPE.itemsize == 48
    assert {n: mix.TARGET_DTYPE.fields[n][1] for n in mix.TARGET_DTYPE.names} == {n: getattr(Target, n).offset for n, _ in Target._fields_}
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    body = re.search(r"typedef struct fsn_mix_target \{(.*?)\} fsn_mix_target;", src, flags=re.S).group(1)
    assert re.sub(r"/\*.*?\*/", "", body, flags=re.S).split() == "double q; int after_max; int mode;".split()


def test_header_exports_and_bindings_agree_on_the_target_entries():
    from fullsubnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert "fsn_*" in open(os.path.join(ROOT, "fullsubnet_amd", "csrc", "fsn_exports.map")).read()
    for name in ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.ADDED_IN_118
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118  # additive: no new revision
    old = re.search(r"\bfsn_mix_pairs\s*\(([^)]*)\)", src).group(1).split(",")
    new = re.search(r"\bfsn_mix_pairs_target\s*\(([^)]*)\)", src).group(1).split(",")
    norm = lambda a: [" ".join(x.split()) for x in a]  # noqa: E731
    extra = [x for x in norm(new) if x not in norm(old)]
    assert extra == ["const fsn_mix_target* targets", "float* target"]  # fsn_mix_pairs plus these two
    import fullsubnet_amd
    assert fullsubnet_amd.reverberation_time_shortening is fullsubnet_amd.acoustics.rvb.reverberation_time_shortening


def test_refusals_and_size_query_without_a_device():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    tq, mixq, conv = L.fsn_mix_target_workspace_bytes, L.fsn_mix_workspace_bytes, L.fsn_conv_rows_workspace_bytes
    # fsn_mix_pairs' workspace plus the second convolution's row, the shortened taps ([B][L rounded up to 4]) and their
    # offset / length tables
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for B, Ls, h in ((7, 4097, 800), (7, 4097, 0), (1, 1, 1), (48, 49152, 64000)):
        assert tq(B, Ls, h) == mixq(B, Ls, h) + r256(B * Ls * 4) + r256(B * ((Ls + 3) // 4 * 4) * 4) + r256(B * 8) + r256(B * 4)
    for bad in ((0, 100, 10), (1, 0, 10), (1, 131073, 10), (1, 100, -1)):
        assert tq(*bad) == 0 and b"1 <= L <= 131072" in L.fsn_last_error()
    p = ctypes.c_void_p
    ok = 1 << 12
    call = lambda **k: L.fsn_rir_shorten(*[k.get(n, d) for n, d in (  # noqa: E731
        ("h", p(ok)), ("fmt", 0), ("off", p(ok)), ("len", p(ok)), ("B", 2), ("max_h_len", 100), ("targets", p(ok)),
        ("out", p(2 * ok)), ("ld", 100), ("win", p(3 * ok)), ("idx", None), ("stream", None))])
    for kw, msg in ((dict(h=None), b"NULL"), (dict(off=None), b"NULL"), (dict(len=None), b"NULL"), (dict(targets=None), b"NULL"),
                    (dict(out=None), b"NULL"), (dict(B=0), b"B >= 1"), (dict(B=-3), b"B >= 1"), (dict(max_h_len=-1), b"length >= 0"),
                    (dict(ld=99), b"too small for the longest response of 100 taps"), (dict(ld=0, max_h_len=0), b"too small"),
                    (dict(fmt=2), b"slab_format"), (dict(win=p(2 * ok)), b"two arrays")):
        assert call(**kw) == -1, kw
        assert msg in L.fsn_last_error(), (kw, L.fsn_last_error())
    big = tq(2, 100, 10)
    mcall = lambda **k: L.fsn_mix_pairs_target(*[k.get(n, d) for n, d in (  # noqa: E731
        ("clean", p(ok)), ("noise", p(ok)), ("rir", p(ok)), ("fmt", 0), ("items", p(ok)), ("segs", p(ok)), ("n_segs", 1),
        ("B", 2), ("L", 100), ("eps", 1e-6), ("targets", p(ok)), ("noisy", p(ok)), ("out_clean", p(2 * ok)),
        ("target", p(3 * ok)), ("ws", p(ok)), ("ws_bytes", big), ("stream", None))])
    for kw, rc, msg in ((dict(L=0), -1, b"1 <= L"), (dict(B=0), -1, b"B >= 1"), (dict(fmt=2), -1, b"slab_format"),
                        (dict(n_segs=-1), -1, b"n_segs"), (dict(eps=-1.0), -1, b"eps"), (dict(targets=None), -1, b"NULL"),
                        (dict(target=None), -1, b"NULL"), (dict(items=None), -1, b"NULL"), (dict(ws=None), -1, b"NULL workspace"),
                        (dict(ws=p(ok + 64)), -1, b"aligned"), (dict(ws_bytes=tq(2, 100, 0) - 1), -2, b"at least"),
                        (dict(target=p(ok)), -1, b"three arrays"), (dict(target=p(2 * ok)), -1, b"three arrays")):
        assert mcall(**kw) == rc, kw
        assert msg in L.fsn_last_error(), (kw, L.fsn_last_error())
    # a mode outside 0 - 2 lives in a device table the library's host code cannot read: the packer refuses it
    from fullsubnet_amd import mix
    with pytest.raises(_lib.FsnError, match="mode 5 is outside 0 - 2"):
        mix.pack_targets([dataclasses.replace(R.mix_cases()[1][1], target_mode=5)])
