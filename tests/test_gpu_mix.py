"""fsn_conv_rows / fsn_mix_pairs and the loader on the device, held to the fp64 numpy port (tests/mix_reference.py).

Convolution: per-row error = max difference from the fp64 result over the peak of |h| * |x|; allowance 4 x the same
figure of a CPU fp32 FFT convolution (torch.fft) of that case, not below 4 * 2^-24.  Mix: per-row error against the fp64
port over the row's peak; allowance 4 x the fp32 port's own error on that row, not below 2^-23.  Outputs and workspaces
are NaN before every call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mix_reference as R  # noqa: E402
from oracle import fullsubnet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def nan_bytes(n):
    return torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")  # every fp32 / fp64 word a NaN


def conv_rows(x, hs, fmt, max_h_len=None):
    """fsn_conv_rows on x [B, L] with the responses `hs` (PCM-valued fp32) in a slab of format `fmt`."""
    from fullsubnet_amd import _lib, mix
    B, L = x.shape
    slab, off, lens = mix._to_slab(hs, fmt)
    d_slab = torch.from_numpy(slab).cuda()
    d_off, d_len = torch.from_numpy(off).cuda(), torch.from_numpy(lens.astype(np.int32)).cuda()
    d_x = torch.from_numpy(x).cuda()
    y = torch.full((B, L), float("nan"), device="cuda")
    lib = _lib.lib()
    nbytes = lib.fsn_conv_rows_workspace_bytes(B, L, int(max(lens)) if max_h_len is None else max_h_len)
    assert nbytes > 0
    ws = nan_bytes(nbytes)
    _lib.check(lib.fsn_conv_rows(d_x.data_ptr(), B, L, d_slab.data_ptr(), mix.SLAB_FORMATS[fmt], d_off.data_ptr(),
                                 d_len.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()))
    return y.cpu().numpy()


def mix_poisoned(bank, items, L, **kw):
    """mix_batch into NaN outputs with a NaN workspace."""
    from fullsubnet_amd import _lib, mix
    out = (torch.full((len(items), L), float("nan"), device="cuda"), torch.full((len(items), L), float("nan"), device="cuda"))
    real = _lib.workspace
    _lib.workspace = lambda nbytes, device: real(nbytes, device).fill_(0xFF)
    try:
        noisy, clean = mix.mix_batch(bank, items, L, out=out, **kw)
    finally:
        _lib.workspace = real
    return noisy.cpu().numpy(), clean.cpu().numpy()


def check(rows):
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f"worst error / allowance: {worst[1] / worst[2]:.3f} ({worst[0]}: {worst[1]:.3e} of {worst[2]:.3e}), {len(rows)} rows")
    for name, err, allow in rows:
        assert err <= allow, (name, err, allow)


@pytest.mark.parametrize("L", R.CONV_L)
def test_convolution_sweep(fsn, L):
    """Response lengths 1, 2, 255, 512, 513, L - 1, L, L + 7, 3 L where they mean something, in batches of 1, 3 and 16
    rows of mixed lengths (0 among them), both slab formats; L + min(h, L) - 1 lands on 2^k and on 2^k + 1."""
    check(R.run_conv_sweep(conv_rows, L))


def test_convolution_workspace_sets_the_transform(fsn):
    """The circular length follows from the workspace: a longer one than the batch needs gives the same convolution, one
    sized for shorter responses turns the rows it cannot carry into NaN (never an aliased result), rows without a response
    are copied either way."""
    L = 700
    x, hs = R.conv_inputs(L, [400, 0, 40], seed=5)
    want = np.stack([R.fft_conv(x[b], h) if len(h) else x[b].astype(np.float64) for b, h in enumerate(hs)])
    for max_h in (400, 700):
        y = conv_rows(x, hs, "f32", max_h_len=max_h)
        check([(f"max_h_len {max_h} row {b}", R.conv_error(y[b], want[b], x[b], hs[b]), R.CONV_FLOOR) for b in (0, 2)])
        assert np.array_equal(y[1], x[1])
    y = conv_rows(x, hs, "f32", max_h_len=40)   # 700 + 40 - 1 <= 1024 < 700 + 400 - 1
    assert np.isnan(y[0]).all() and np.array_equal(y[1], x[1]) and np.isfinite(y[2]).all()
    y = conv_rows(x, hs, "f32", max_h_len=0)    # no transform at all
    assert np.isnan(y[0]).all() and np.array_equal(y[1], x[1]) and np.isnan(y[2]).all()


@pytest.fixture(scope="module")
def sweep_bank(fsn):
    clean, noise, rir = R.mix_sources()
    return {fmt: fsn.MixBank(clean, noise, rir, "cuda", fmt=fmt) for fmt in ("f32", "i16")}, (clean, noise, rir)


def test_mix_sweep(fsn, sweep_bank):
    """Both clip branches, an all-zero clean row, a row whose noise is all silence, 1 / 2 / 5 segments (one ending at L),
    SNR -5 and 20, clean_len 1, L - 1 and L, 1-D and 2-D responses: one call, every row against the fp64 port."""
    banks, lists = sweep_bank
    cases = R.mix_cases()
    items = [it for _, it, _ in cases]
    got = {fmt: mix_poisoned(banks[fmt], items, R.MIX_L) for fmt in banks}
    for a, b in zip(got["f32"], got["i16"]):
        assert np.array_equal(a, b)  # the sources are 16-bit PCM values in both banks
    noisy, clean = got["f32"]
    for b, (name, it, clipped) in enumerate(cases):
        peak = float(np.abs(noisy[b]).max())
        assert (abs(peak - (0.99 - R.EPS)) < 1e-6) == clipped, (name, peak)
        if name.startswith("zero_clean"):
            assert not noisy[b].any() and not clean[b].any(), name  # the gain is clean_rms / .. = 0: as in the port
        if name == "silent_noise":
            assert np.array_equal(noisy[b], clean[b])
    rows = R.run_mix_rows((noisy, clean), items, *lists, R.MIX_L)
    check([(f"{cases[int(n.split()[1])][0]} {n}", e, a) for n, e, a in rows])


def test_mix_golden_items_against_the_reference(fsn, golden_dir):
    """The reference's own Dataset.__getitem__ / snr_mix outputs (tests/golden/mix_items.npz).  Allowance 2^-19 of the row's
    peak, the reference's fp32 rounding (tests/test_mix_cpu.py: test_fp64_port_reproduces_the_reference_outputs)."""
    items, _, L = R.golden_items(golden_dir)
    f32, pcm16, _ = R.golden_sources(golden_dir)
    descs = [it for _, it, _, _ in items]
    for fmt, lists in (("f32", f32), ("i16", pcm16)):
        bank = fsn.MixBank(*lists, "cuda", fmt=fmt)
        noisy, clean = mix_poisoned(bank, descs, L)
        check([(f"{fmt} {name} {what}", R.mix_error(ref, got[b]), 2.0 ** -19)
               for b, (name, _, ref_n, ref_c) in enumerate(items) for what, ref, got in (("noisy", ref_n, noisy), ("clean", ref_c, clean))])


def test_rows_are_independent_and_calls_repeat(fsn, sweep_bank):
    banks, _ = sweep_bank
    cases = {name: it for name, it, _ in R.mix_cases()}
    probe = cases["reverb_2d_five_segments"]
    others = [cases[n] for n in ("clipped_spikes_reverb", "plain_snr20", "zero_clean", "reverb_snr-5_two_segments")]
    batch = [probe] + others + [probe]
    n1, c1 = mix_poisoned(banks["f32"], batch, R.MIX_L)
    assert np.array_equal(n1[0], n1[-1]) and np.array_equal(c1[0], c1[-1])
    n2, c2 = mix_poisoned(banks["f32"], batch, R.MIX_L)
    assert np.array_equal(n1, n2) and np.array_equal(c1, c2)
    n3, c3 = mix_poisoned(banks["f32"], [probe], R.MIX_L, max_rir_len=800)  # alone, on the batch's transform
    assert np.array_equal(n3[0], n1[0]) and np.array_equal(c3[0], c1[0])


def test_mix_pairs_is_capturable_in_a_hip_graph(fsn, sweep_bank):
    """The call only enqueues on the caller's stream (no copy, no synchronise): captured once, a replay mixes whatever
    descriptors the static table holds then, bit-identical to the eager call."""
    from fullsubnet_amd import _lib, mix
    banks, _ = sweep_bank
    bank, L = banks["i16"], R.MIX_L
    cases = [it for _, it, _ in R.mix_cases()]
    first, second = cases[:4], cases[4:8]
    eager = [mix_poisoned(bank, items, L, max_rir_len=800) for items in (first, second)]

    def table(items):
        tab, seg_tab, n_segs, _ = mix.pack_items(bank, items, L)
        raw = np.zeros(256 + 16 * 32, np.uint8)  # the item table, then room for 32 segments
        raw[:tab.nbytes] = tab.view(np.uint8)
        raw[256:256 + seg_tab.nbytes] = seg_tab.view(np.uint8)
        return torch.from_numpy(raw), n_segs

    (t1, n1), (t2, n2) = table(first), table(second)
    desc = t1.cuda()
    noisy, clean = torch.empty(4, L, device="cuda"), torch.empty(4, L, device="cuda")
    ws = nan_bytes(_lib.lib().fsn_mix_workspace_bytes(4, L, 800))
    n_segs = max(n1, n2)  # the items' slices never reach past their own segments
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mix.mix_pairs(bank, desc, 256, n_segs, noisy, clean, ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mix.mix_pairs(bank, desc, 256, n_segs, noisy, clean, ws)
    for tab, want in ((t2, eager[1]), (t1, eager[0])):
        desc.copy_(tab)
        noisy.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(noisy.cpu().numpy(), want[0]) and np.array_equal(clean.cpu().numpy(), want[1])


def test_trainer_runs_from_a_mix_loader(fsn):
    """MixLoader -> Trainer for two steps: finite losses; batches differ between steps and between two ranks' slices; a
    second loader with the same seed yields bit-identical batches."""
    from fullsubnet_amd.trainer import Trainer
    rng = np.random.default_rng(3)
    L = 2560
    clean = [R.pcm(0.2 * rng.standard_normal(n)) for n in (3000, 2560, 2000, 4000, 2700, 3100, 2900, 2561) * 2]
    noise = [R.pcm(0.05 * rng.standard_normal(n)) for n in (5000, 900, 1500)]
    r2 = rng.standard_normal((2, 200)) * np.exp(-np.arange(200) / 30.0)
    rir = [R.pcm(0.5 * np.exp(-np.arange(600) / 80.0) * rng.standard_normal(600)), R.pcm(0.8 * r2 / np.abs(r2).max())]
    bank = fsn.MixBank(clean, noise, rir, "cuda", fmt="i16")
    cfg = fsn.MixConfig(sr=16000, sub_sample_length=0.16, silence_length=0.02)
    assert cfg.samples == L
    new = lambda rank: fsn.MixLoader(bank, cfg, batch_size=4, seed=9, rank=rank, world_size=2)  # noqa: E731
    loader = new(0)
    assert len(loader) == 2
    first = [(n.clone(), c.clone()) for n, c in loader]
    again = [(n.clone(), c.clone()) for n, c in new(0)]
    other = [(n.clone(), c.clone()) for n, c in new(1)]
    for (n, c), (n2, c2) in zip(first, again):
        assert n.shape == (4, L) and n.is_cuda and torch.isfinite(n).all() and torch.isfinite(c).all()
        assert torch.equal(n, n2) and torch.equal(c, c2)
    assert not torch.equal(first[0][0], first[1][0]) and not torch.equal(first[0][0], other[0][0])
    assert not set(new(0).indices()) & set(new(1).indices())

    params = O.make_params(seed=3)
    model = fsn.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                      fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                      sb_model_hidden_size=384, weight_init=False, norm_type="offline_laplace_norm", num_groups_in_drop_band=2)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    config = {"meta": {"use_amp": True}, "acoustics": {"n_fft": 512, "hop_length": 256, "win_length": 512, "sr": 16000},
              "trainer": {"train": {"epochs": 1, "clip_grad_norm_value": 10}}}
    opt = fsn.ClipAdam(model.parameters(), lr=1e-3, betas=(0.9, 0.999))
    t = Trainer(None, 0, config, False, False, model.cuda(), None, opt, loader)
    t.train()
    assert t.nonfinite_losses == 0 and t.persistent_timeouts == 0 and np.isfinite(t.last_loss)
