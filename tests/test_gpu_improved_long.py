"""Improved FullSubNet recordings of any length: ``improved_fullsubnet.Model.enhance_long`` (segments with carried state; three
passes over them for the reference's norms, libfsn_hip fsn_improved_segment_*) == the fp64 reference of
tests/improved_long_reference.py == ``model(y)``, on recordings short enough to compare.
Needs a real MI355X:  python -m pytest tests -m gpu

The bounds are the project's: the mask against fp64 at SHARP x the fp32 cell emulation's own error (whole tensor, per frame,
per 16-row tile), carried (h, c) the same way, the fp64 sums by the bound of an fp64 sum, the divisors to one fp32 ulp; the
waveform <= 2e-3 x peak against ``model(y)`` (tests/test_gpu_long.py) and <= 2e-5 x peak against StreamingEnhancer under the
causal norms (tests/test_gpu_streaming.py).  Two segmentations of one recording give the same mask bit for bit: a frame's sum
has a fixed shape and the fp64 carries advance frame by frame.  Hours of audio are left to tools/bench_long_improved.py."""
import ctypes

import numpy as np
import pytest
import torch

import improved_long_reference as LR
import improved_stream_reference as R
from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF
from test_gpu_improved_stream import model_of, read_state, run_calls, write_state

pytestmark = pytest.mark.gpu

L_SHORT, L_WHOLE = 1237, 1248  # at 64 / 32: 39 frames; 40 frames, a whole last hop
SEGMENTATIONS = (1, 7, 16, 19, 64)  # 19: two whole segments and a remainder of one or two frames; 64: one segment
CAUSAL = "cumulative_laplace_norm"


def peak(x):
    return float(x.abs().max())


def split_of(T, k):
    return tuple(min(k, T - s) for s in range(0, T, k))


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


def recording(fsn, model, cfg, B, samples, seed, norm="offline"):
    """The recording on the device, ``model(y)`` of it, and the reference of the three runs on the device's own magnitude -
    computed once, never written to."""
    xd = torch.from_numpy(O.make_noisy(B, samples, seed=seed)).cuda()
    with torch.no_grad():
        one = model(xd)[:, 0]
    n_fft = 2 * (cfg.F - 1)
    mag = fsn.stft(xd, n_fft, n_fft // 2, n_fft)[0].cpu().numpy()
    case = LR.Case(f"{samples}-samples", cfg, (mag.shape[-1],) * B, norm)
    return xd, one, case, LR.Ref(case, mag)


def hold(xd, one, case, ref, got, crm, what):
    assert got.shape == xd.shape and got.is_cuda and crm.shape == (case.B, 2, case.cfg.F, case.T)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(crm).all())  # poisoned buffers: all that was read was written
    worst = LR.check_mask(case, ref, crm.cpu().numpy())
    d_one = peak(got - one) / peak(one)
    print(f"[ilong] {what}: mask worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x the yardstick; "
          f"waveform vs model(y) {d_one:.2e} x peak")
    assert d_one <= 2e-3


# ---- 1. / 2. basic recordings ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basic(fsn):
    model = model_of(R.SMALL)
    out = {}
    for samples in (L_SHORT, L_WHOLE):
        rec = recording(fsn, model, R.SMALL, 2, samples, seed=17)
        assert rec[2].T == {L_SHORT: 39, L_WHOLE: 40}[samples]
        runs = {k: model.enhance_long(rec[0], segment_frames=k, return_crm=True, poison=True) for k in SEGMENTATIONS}
        out[samples] = (rec, runs)
    return out


@pytest.mark.parametrize("samples", [L_SHORT, L_WHOLE])
@pytest.mark.parametrize("k", SEGMENTATIONS)
def test_enhance_long_equals_the_reference_and_the_one_call(basic, samples, k):
    rec, runs = basic[samples]
    hold(*rec, *runs[k], what=f"{samples} samples, segment_frames {k}")


@pytest.mark.parametrize("samples", [L_SHORT, L_WHOLE])
def test_two_segmentations_give_the_same_bits(basic, samples):
    _, runs = basic[samples]
    assert torch.equal(runs[7][1], runs[16][1])


def test_both_forms_of_the_sections_blocks_give_the_same_bits(fsn, basic):
    """fsn_debug_improved_stream_form applies to pass 3 as it does to the stream step."""
    L = fsn._lib.lib()
    (xd, _, _, _), runs = basic[L_SHORT]
    default = L.fsn_debug_improved_stream_form(-1)
    try:
        assert L.fsn_debug_improved_stream_form(1 - default) == 1 - default
        other = model_of(R.SMALL).enhance_long(xd, segment_frames=7, return_crm=True, poison=True)
    finally:
        L.fsn_debug_improved_stream_form(default)
    assert torch.equal(other[1], runs[7][1]) and torch.equal(other[0], runs[7][0])


# ---- 3. unequal neighbour counts, two sections ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [R.OTHER_NEIGHBOURS, R.TWO_SECTIONS], ids=["other-neighbours", "two-sections"])
def test_other_configurations(fsn, cfg):
    model = model_of(cfg)
    rec = recording(fsn, model, cfg, 1, L_SHORT, seed=19)
    got = model.enhance_long(rec[0], segment_frames=7, return_crm=True, poison=True)
    hold(*rec, *got, what=f"{cfg}, segment_frames 7")


# ---- 4. a ragged batch ------------------------------------------------------------------------------------------------------------
def test_ragged_batch_rows_are_the_rows_alone(fsn):
    model = model_of(R.SMALL)
    lengths = [1237, 640, 40]  # 39, 21 and 2 frames
    noisy = O.make_noisy(3, lengths[0], seed=23)
    for b, n in enumerate(lengths):
        noisy[b, n:] = 1e3  # never read
    xd = torch.from_numpy(noisy).cuda()
    # 7: row 1's 21 frames end exactly on a segment edge, row 2's inside the first segment, row 0's inside the last
    got, crm = model.enhance_long(xd, lengths=lengths, segment_frames=7, return_crm=True, poison=True, slab_frames=16)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(crm).all())
    for b, n in enumerate(lengths):
        T = 1 + n // 32
        alone, alone_crm = model.enhance_long(xd[b:b + 1, :n], segment_frames=7, return_crm=True, poison=True, slab_frames=16)
        assert torch.equal(crm[b, :, :, :T], alone_crm[0]), f"row {b}: the mask differs from the row's alone"
        d = peak(got[b, :n] - alone[0]) / peak(alone[0])
        print(f"[ilong] ragged row {b} ({n} samples, {T} frames): waveform vs the row alone {d:.2e} x peak")
        assert d <= 2e-5
        assert bool((got[b, n:] == 0).all()) and bool((crm[b, :, :, T:] == 0).all())


# ---- 5. the entries directly --------------------------------------------------------------------------------------------------------
def run_entries(fsn, model, cfg, mag, total, segments, fb_norm=0):
    """The passes over `segments` on mag [B, F, T] (device) from a blob poisoned outside its fields -> (blob, den_fb, den_sb,
    fb_out [T, B, F - 1], mask [B, 2, F, T])."""
    lib, L = fsn._lib, fsn._lib.lib()
    B, F, T = mag.shape
    c = model.stream_cfg()
    ref, st, dev = ctypes.byref(c), lib.stream_ptr(mag.device), mag.device
    lay = lib.improved_stream_state_layout(c, B)
    state = write_state(lay, cfg, B, R.new_state(B, cfg), dev)
    sargs = (state.data_ptr(), state.numel())
    packed = model.stream_packed_weights().data_ptr()
    fb_out = torch.full((T, B, F - 1), float("nan"), device=dev)
    mask = torch.full((B, 2, F, T), float("nan"), device=dev)
    tot = torch.tensor(total, dtype=torch.int32, device=dev)

    def ws(k):
        w = lib.workspace(L.fsn_improved_stream_workspace_bytes(ref, B, k), dev)
        w.fill_(0xFF)  # nothing of the workspace may be read before the call wrote it
        return w

    seg = lambda s0, k: mag[:, :, s0:s0 + k].contiguous()  # noqa: E731  (held by the caller across the entry)
    if fb_norm == 0:
        for s0, k in segments:
            x = seg(s0, k)
            lib.check(L.fsn_improved_segment_stats(ref, *sargs, s0, tot.data_ptr(), lib.dev_ptr(x, "mag"), B, k, st))
    den_fb, den_sb = torch.empty(B, device=dev), torch.empty(c.num_sections, B, device=dev)
    for s0, k in segments:
        w, x = ws(k), seg(s0, k)
        lib.check(L.fsn_improved_segment_fullband(ref, packed, *sargs, fb_norm, s0, tot.data_ptr(), lib.dev_ptr(x, "mag"), B, k,
                                                  lib.dev_ptr(fb_out[s0:s0 + k]), w.data_ptr(), w.numel(), st))
    lib.check(L.fsn_improved_segment_divisors(ref, *sargs, tot.data_ptr(), B, lib.dev_ptr(den_fb), lib.dev_ptr(den_sb), st))
    for s0, k in segments:
        w, x, y = ws(k), seg(s0, k), torch.full((B, 2, F, k), float("nan"), device=dev)
        lib.check(L.fsn_improved_segment_sections(ref, packed, *sargs, s0, tot.data_ptr(), lib.dev_ptr(x, "mag"), lib.dev_ptr(fb_out[s0:s0 + k]),
                                                  B, k, lib.dev_ptr(y), w.data_ptr(), w.numel(), st))
        mask[..., s0:s0 + k] = y
    torch.cuda.synchronize()
    return state, den_fb, den_sb, fb_out, mask, lay


def test_sums_divisors_and_state_through_the_entries(fsn):
    cfg, total = R.SMALL, (39, 21, 2)
    model = model_of(cfg)
    case, ref = LR.reference_of("entries", cfg, total)
    mag = ref.mag.copy()
    for b, n in enumerate(total):
        mag[b, :, n:] = np.nan  # a frame past a row's end is never read
    md = torch.from_numpy(mag).cuda()
    state, den_fb, den_sb, fb_out, mask, lay = run_entries(fsn, model, cfg, md, total, [(0, 1), (1, 20), (21, 11), (32, 7)])
    assert bool(torch.isfinite(fb_out).all()) and bool(torch.isfinite(mask).all())
    got = read_state(lay, cfg, 3, state)  # also: every byte outside the fields is untouched, padded rows are finite
    worst = LR.check_state(case, ref, got)
    print(f"[ilong] entries: state worst {max(worst.values()):.2f} x ({max(worst, key=worst.get)})")
    LR.check_mask(case, ref, mask.cpu().numpy())
    LR.check_divisors(den_fb.cpu().numpy(), den_sb.cpu().numpy(), got, total, cfg)
    # the full-band output against the fp64 run, inside the rows
    fb = fb_out.permute(1, 2, 0).cpu().numpy()
    for b, n in enumerate(total):
        r64, c32 = ref.result["64"].fb[b, :, :n], ref.result["c32"].fb[b, :, :n].astype(np.float64)
        assert R.frob(fb[b, :, :n].astype(np.float64), r64) <= R.SHARP * R.frob(c32, r64), f"fb_out row {b}"
    # one segment: the same sums, divisors, planes, masks and state, bit for bit
    again = run_entries(fsn, model, cfg, md, total, [(0, 39)])
    for name, a, b in zip(("state", "den_fb", "den_sb", "fb_out", "mask"), (state, den_fb, den_sb, fb_out, mask), again):
        assert torch.equal(a, b), name


# ---- 6. the causal norms through the same driver --------------------------------------------------------------------------------------
def test_cumulative_model_is_the_stream_step_and_the_streaming_enhancer(fsn):
    from fullsubnet_amd.streaming import StreamingEnhancer
    model = model_of(R.SMALL, norm_type=CAUSAL, sb_norm_type=CAUSAL)
    xd = torch.from_numpy(O.make_noisy(2, L_SHORT, seed=5)).cuda()
    got, crm = model.enhance_long(xd, segment_frames=7, return_crm=True, poison=True)
    mag = fsn.stft(xd, 64, 32, 64)[0].cpu().numpy()
    lay = fsn._lib.improved_stream_state_layout(model.stream_cfg(), 2)
    calls, _ = run_calls(fsn, model, 2, split_of(39, 7), mag, torch.zeros(lay["bytes"], dtype=torch.uint8, device="cuda"))
    assert torch.equal(crm, torch.cat(calls, dim=-1))
    enh = StreamingEnhancer(model, batch_size=2)
    want = torch.cat([enh.process(xd[:, :500]), enh.process(xd[:, 500:]), enh.flush()], dim=1)
    d = peak(got - want) / peak(want)
    print(f"[ilong] cumulative / cumulative, segments of 7 vs StreamingEnhancer: {d:.2e} x peak")
    assert got.shape == want.shape and d <= 2e-5


def test_cumulative_fullband_norm_with_offline_sections(fsn):
    """norm_type = "cumulative_laplace_norm" alone, as the reference runs it: two passes, the mask against the fp64
    forward("cumulative", "offline")."""
    model = model_of(R.SMALL, norm_type=CAUSAL)
    xd, one, case, ref = recording(fsn, model, R.SMALL, 2, L_SHORT, seed=29, norm="cumulative")
    want = LR.rows_alone(ref.mag, case.total, ref.params, R.SMALL, "cumulative")
    assert max(np.abs(ref.mask["64"][0][b] - want[b]).max() for b in range(2)) <= 1e-12  # the truth is `forward` itself
    a = model.enhance_long(xd, segment_frames=7, return_crm=True, poison=True)
    hold(xd, one, case, ref, *a, what="cumulative / offline, segment_frames 7")
    b = model.enhance_long(xd, segment_frames=16, return_crm=True, poison=True)
    assert torch.equal(a[1], b[1])


# ---- 7. the shipped 48 kHz configuration ------------------------------------------------------------------------------------------------
def test_shipped_48k_configuration(fsn):
    model = model_of(R.K48)
    rec = recording(fsn, model, R.K48, 1, 19200, seed=31)
    assert rec[2].T == 41
    got = model.enhance_long(rec[0], segment_frames=16, return_crm=True, poison=True)
    hold(*rec, *got, what="48 kHz, 19 200 samples, segment_frames 16")


# ---- 8. refusals on the device ------------------------------------------------------------------------------------------------------------
def test_entries_refuse_short_buffers_before_anything_is_launched(fsn):
    L, lib = fsn._lib.lib(), fsn._lib
    model = model_of(R.SMALL)
    c = model.stream_cfg()
    ref, dev = ctypes.byref(c), torch.device("cuda")
    nbytes = L.fsn_improved_stream_state_bytes(ref, 1)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    mag, tot = torch.ones((1, 33, 4), device=dev), torch.tensor([4], dtype=torch.int32, device=dev)
    fb_out, mask = torch.zeros((4, 1, 32), device=dev), torch.zeros((1, 2, 33, 4), device=dev)
    ws = lib.workspace(L.fsn_improved_stream_workspace_bytes(ref, 1, 4), dev)
    packed, st = model.stream_packed_weights().data_ptr(), lib.stream_ptr(dev)
    p = lambda t: lib.dev_ptr(t)  # noqa: E731
    fullband = lambda sb, wb, fb_norm=0: L.fsn_improved_segment_fullband(  # noqa: E731
        ref, packed, blob.data_ptr(), sb, fb_norm, 0, tot.data_ptr(), p(mag), 1, 4, p(fb_out), ws.data_ptr(), wb, st)
    sections = lambda sb, wb: L.fsn_improved_segment_sections(  # noqa: E731
        ref, packed, blob.data_ptr(), sb, 0, tot.data_ptr(), p(mag), p(fb_out), 1, 4, p(mask), ws.data_ptr(), wb, st)
    assert L.fsn_improved_segment_stats(ref, blob.data_ptr(), nbytes - 1, 0, tot.data_ptr(), p(mag), 1, 4, st) == -2
    assert b"too small" in L.fsn_last_error()
    assert fullband(nbytes - 1, ws.numel()) == -2 and fullband(nbytes, ws.numel() - 1) == -2
    assert sections(nbytes - 1, ws.numel()) == -2 and sections(nbytes, ws.numel() - 1) == -2
    assert fullband(nbytes, ws.numel(), fb_norm=2) == -1 and b"fb_norm" in L.fsn_last_error()
    torch.cuda.synchronize()
    assert not blob.any() and not mask.any() and not fb_out.any()  # nothing was launched


def test_enhance_long_refusals_on_the_device(fsn):
    from fullsubnet_amd.improved_fullsubnet import Model
    xd = torch.from_numpy(O.make_noisy(1, L_SHORT, seed=3)).cuda()
    err = fsn._lib.FsnError
    for model, text in ((Model(**dict(R.as_dict(R.SMALL), sequence_model="GRU")), "LSTM"),
                        (Model(**MF.IMPROVED_16K), "hop = n_fft / 2"),
                        (Model(**dict(R.as_dict(R.SMALL), sb_norm_type=CAUSAL)), "norm_type / sb_norm_type"),
                        (Model(**dict(R.as_dict(R.SMALL), norm_type="offline_gaussian_norm")), "offline_gaussian_norm")):
        with pytest.raises(err, match=text) as e:
            model.cuda().eval().enhance_long(xd, segment_frames=16)
        assert "model(y)" in str(e.value)
    model = model_of(R.SMALL)
    with pytest.raises(err, match="segment_frames"):
        model.enhance_long(xd, segment_frames=4097)
    with pytest.raises(err, match="n_fft 64 / hop 32"):
        model.enhance_long(xd, segment_frames=16, n_fft=960, hop_length=480)
    with pytest.raises(ValueError):
        model.enhance_long(torch.cat([xd, xd]), lengths=[L_SHORT, 20], segment_frames=16)
    # a host input and the largest segment under a workspace limit
    from fullsubnet_amd.improved_long_form import ImprovedLongPlan
    limit = 1 << 20
    k = ImprovedLongPlan(model.stream_cfg(), 64, "offline", 1, L_SHORT, workspace_limit=limit).segment_frames
    assert 1 < k < 39
    got = model.enhance_long(xd.cpu(), workspace_limit=limit, slab_frames=5)  # several transform slabs too
    want = model.enhance_long(xd, segment_frames=7)
    assert got.is_cuda and peak(got - want) <= 2e-5 * peak(want)
