"""Mixing of training pairs, the parts that need no device: the numpy port (tests/mix_reference.py) against the
reference's own outputs (tests/golden/mix_*.npz), draw_item against the reference's recorded random calls, the
convolution references, the refusals and size queries of fsn_conv_rows / fsn_mix_pairs, and the sweep tables."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def goldens(golden_dir):
    items, logs, L = R.golden_items(golden_dir)
    (clean, noise, rir), _, _ = R.golden_sources(golden_dir)
    return items, logs, L, clean, noise, rir


def test_draw_item_reproduces_every_recorded_choice(goldens):
    """Under the recorded seeds draw_item makes the random calls Dataset.__getitem__ made - the same functions with the same
    arguments in the same order, hence the same results - for every golden item."""
    items, logs, L, clean, noise, rir = goldens
    assert len(logs) == 12
    for i, (ref, mine) in enumerate(logs):
        assert mine == ref, (i, ref, mine)
    kinds = [it for name, it, _, _ in items if name.startswith("getitem")]
    assert any(it.rir_index < 0 for it in kinds) and any(it.rir_index >= 0 for it in kinds)
    assert any(it.clean_len < L for it in kinds), "one clean file is shorter than the crop"
    assert any(len(it.segments) > 1 for it in kinds), "some noise rows are stitched from several files"


def test_fp64_port_reproduces_the_reference_outputs(goldens):
    """The port in fp64 against what the reference returned (fp32 arithmetic, scipy's fp32 fftconvolve).  Allowance 2^-19
    of the row's peak: the reference rounds to fp32 about ten times per sample (2^-24 each), its three rms scalars and
    two peaks carry fp32 sums, and its fp32 FFT convolution sits at ~2e-7 of peak; 32 roundings' worth covers them."""
    items, _, L, clean, noise, rir = goldens
    worst = 0.0
    names = [n for n, *_ in items]
    assert any("clipped" in n for n in names) and any(n.startswith("direct") and "clipped" not in n for n in names)
    for name, it, ref_noisy, ref_clean in items:
        noisy, cl, peak = R.mix_item(it, clean, noise, rir, L, np.float64, eps=1e-6)
        assert ("clipped" in name) == (peak > 0.999) or name.startswith("getitem"), (name, peak)
        e = max(R.mix_error(ref_noisy, noisy), R.mix_error(ref_clean, cl))
        print(f"{name}: {e:.3e}")
        worst = max(worst, e)
        assert e <= 2.0 ** -19, (name, e)
    print(f"worst: {worst:.3e}")


@pytest.mark.parametrize("L,h", [(1, 1), (2, 1), (2, 2), (3, 9), (5, 4), (16, 1), (17, 16), (33, 32), (64, 200), (100, 29)])
def test_convolution_references_equal_np_convolve(L, h):
    rng = np.random.default_rng(L * 1000 + h)
    x, hh = rng.standard_normal(L).astype(np.float32), rng.standard_normal(h).astype(np.float32)
    want = np.convolve(x.astype(np.float64), hh.astype(np.float64))[:L]
    scale = np.convolve(np.abs(x), np.abs(hh)).max()
    assert np.abs(R.fft_conv(x, hh) - want).max() <= 1e-13 * scale
    # the kernels' four-step plan, index for index (and with a longer transform than needed, as a batch's longest sets it)
    assert np.abs(R.four_step_conv(x, hh) - want).max() <= 1e-13 * scale
    assert np.abs(R.four_step_conv(x, hh, log_n=9) - want).max() <= 1e-12 * scale


def test_tables_match_the_c_structs():
    from fullsubnet_amd import mix
    off = {n: mix.ITEM_DTYPE.fields[n][1] for n in mix.ITEM_DTYPE.names}
    assert off == dict(clean_off=0, clean_len=8, seg_begin=12, seg_count=16, rir_off=24, rir_len=32, snr_db=36,
                       target_dbfs=40, noisy_target_dbfs=44) and mix.ITEM_DTYPE.itemsize == 48

    class Item(ctypes.Structure):  # fsn_mix_item as a C compiler lays it out
        _fields_ = [("clean_off", ctypes.c_long), ("clean_len", ctypes.c_int), ("seg_begin", ctypes.c_int),
                    ("seg_count", ctypes.c_int), ("rir_off", ctypes.c_long), ("rir_len", ctypes.c_int),
                    ("snr_db", ctypes.c_float), ("target_dbfs", ctypes.c_float), ("noisy_target_dbfs", ctypes.c_float)]

    assert ctypes.sizeof(Item) == 48 and {n: getattr(Item, n).offset for n, _ in Item._fields_} == off
    assert {n: mix.SEG_DTYPE.fields[n][1] for n in mix.SEG_DTYPE.names} == dict(src_off=0, dst_off=8, len=12)


def test_refusals_and_size_queries_without_a_device():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    conv, mixq = L.fsn_conv_rows_workspace_bytes, L.fsn_mix_workspace_bytes
    # the circular length is the power of two that holds L + min(h, L) - 1 samples, 16 bytes each, per row
    # (+ 256 bytes: one int per row, up to 64 rows, for the rows whose signal or response is all zeros)
    assert conv(1, 49152, 16000) == 256 + 16 * 65536 and conv(3, 49152, 64000) == 256 + 3 * 16 * 131072
    assert conv(1, 513, 512) == 256 + 16 * 1024 and conv(1, 513, 513) == 256 + 16 * 2048  # exactly 2^k, and 2^k + 1
    assert conv(2, 131072, 3 * 131072) == 256 + 2 * 16 * 262144 == conv(2, 131072, 131072)  # taps from L on are never read
    assert conv(4, 100, 0) == 256                                                    # no response at all: no transform
    rows = 3 * ((7 * 4097 * 4 + 255) // 256 * 256)
    assert mixq(7, 4097, 800) == rows + conv(7, 4097, 800) and mixq(7, 4097, 0) == rows + conv(7, 4097, 0)
    for bad in ((0, 100, 10), (1, 0, 10), (1, 131073, 10), (1, 100, -1), (-2, 100, 1)):
        assert conv(*bad) == 0 and b"1 <= L <= 131072" in L.fsn_last_error()
        assert mixq(*bad) == 0 and b"1 <= L <= 131072" in L.fsn_last_error()
    # the calls: refused before anything is launched (the pointers are never followed)
    p = ctypes.c_void_p
    ok = 1 << 12  # a 256-byte aligned "address"
    big = mixq(2, 100, 10)
    call = lambda **k: L.fsn_mix_pairs(*[k.get(n, d) for n, d in (  # noqa: E731
        ("clean", p(ok)), ("noise", p(ok)), ("rir", p(ok)), ("fmt", 0), ("items", p(ok)), ("segs", p(ok)), ("n_segs", 1),
        ("B", 2), ("L", 100), ("eps", 1e-6), ("noisy", p(ok)), ("out_clean", p(2 * ok)), ("ws", p(ok)), ("ws_bytes", big),
        ("stream", None))])
    for kw, rc, msg in ((dict(L=0), -1, b"1 <= L"), (dict(L=131073), -1, b"1 <= L"), (dict(B=0), -1, b"B >= 1"),
                        (dict(fmt=2), -1, b"slab_format"), (dict(n_segs=-1), -1, b"n_segs"), (dict(eps=-1.0), -1, b"eps"),
                        (dict(items=None), -1, b"NULL"), (dict(ws=None), -1, b"NULL workspace"),
                        (dict(ws=p(ok + 64)), -1, b"aligned"), (dict(ws_bytes=mixq(2, 100, 0) - 1), -2, b"at least"),
                        (dict(out_clean=p(ok)), -1, b"two arrays")):
        assert call(**kw) == rc, kw
        assert msg in L.fsn_last_error(), (kw, L.fsn_last_error())
    conv_call = lambda **k: L.fsn_conv_rows(*[k.get(n, d) for n, d in (  # noqa: E731
        ("x", p(ok)), ("B", 2), ("L", 100), ("h", p(ok)), ("fmt", 1), ("off", p(ok)), ("len", p(ok)), ("y", p(2 * ok)),
        ("ws", p(ok)), ("ws_bytes", conv(2, 100, 10)), ("stream", None))])
    for kw, rc, msg in ((dict(L=-5), -1, b"1 <= L"), (dict(fmt=-1), -1, b"slab_format"), (dict(y=p(ok)), -1, b"alias"),
                        (dict(len=None), -1, b"NULL"), (dict(ws=p(ok + 8)), -1, b"aligned"), (dict(ws_bytes=16), -2, b"at least")):
        assert conv_call(**kw) == rc, kw
        assert msg in L.fsn_last_error(), (kw, L.fsn_last_error())


def test_pack_items_refuses_what_the_device_cannot_check():
    from fullsubnet_amd import _lib
    from fullsubnet_amd.mix import MixItem, pack_items
    clean, noise, rir = R.mix_sources()
    bank = R.HostTables(clean, noise, rir)
    bank.clean_off = np.concatenate([[0], np.cumsum(bank.clean_len)[:-1]])
    bank.noise_off = np.concatenate([[0], np.cumsum(bank.noise_len)[:-1]])
    bank.rir_first_row, bank.rir_len = [0, 1], np.asarray([800, 300, 300, 300])
    bank.rir_off = np.concatenate([[0], np.cumsum(bank.rir_len)[:-1]])
    L = R.MIX_L
    good = MixItem(0, 450, L, [(1, 0, 0, 1200), (2, 10, 1900, 630)], 20, 1, 2, -30, -25)
    tab, segs, n_segs, longest = pack_items(bank, [good, good], L)
    assert n_segs == 4 and longest == 300 and tab["seg_begin"].tolist() == [0, 2] and tab["rir_off"][0] == 800 + 2 * 300
    assert segs["src_off"][1] == bank.noise_off[2] + 10 and tab["clean_off"][1] == 450
    import dataclasses
    for change in (dict(clean_start=-1), dict(clean_len=L + 1), dict(clean_start=901), dict(segments=[(1, 0, 0, 1201)]),
                   dict(segments=[(0, 0, 1, L)]), dict(segments=[(0, -1, 0, 5)]), dict(rir_row=3)):
        with pytest.raises(_lib.FsnError):
            pack_items(bank, [dataclasses.replace(good, **change)], L)
    with pytest.raises(_lib.FsnError):
        pack_items(bank, [good], 131073)


def test_every_mix_case_is_decisive_on_the_clip_branch():
    cases = R.mix_cases()  # asserts 0.999 (1 +- 1e-4) is clear of every case's fp64 peak as it builds the table
    assert len(cases) >= 12 and sum(c for _, _, c in cases) >= 2
    clean, noise, rir = R.mix_sources()
    for name, it, clipped in cases:  # ... so the fp32 yardstick takes the same branch
        assert (R.mix_item(it, clean, noise, rir, R.MIX_L, np.float32)[2] > np.float32(0.999)) == clipped, name


def test_loader_slices_are_disjoint_and_repeatable():
    from fullsubnet_amd.mix import MixConfig, MixLoader
    bank = R.HostTables(*R.mix_sources())
    bank.__class__ = type("Tables", (R.HostTables,), {"__len__": lambda self: 23})
    bank.rir_len = np.asarray([800, 300])
    cfg = MixConfig(sub_sample_length=0.25)
    a, b = (MixLoader(bank, cfg, 4, seed=5, rank=r, world_size=2) for r in (0, 1))
    assert len(a) == len(b) == 2 and a.max_rir_len == 800
    ia, ib = a.indices(), b.indices()
    assert len(ia) == len(ib) == 11 and not set(ia) & set(ib)
    assert MixLoader(bank, cfg, 4, seed=5, rank=0, world_size=2).indices() == ia
    a.set_epoch(1)
    assert a.indices() != ia and len(MixLoader(bank, cfg, 4, seed=5, drop_last=False)) == 6
