"""Recordings of any length without a device: the host book-keeping of ``Model.enhance_long`` (fullsubnet_amd.long_form.
LongPlan: segments, transform slabs, planned bytes) and the size queries of the segment entries (fsn_fullsubnet_segment_*)."""
import ctypes
import os
import re

import pytest

from fullsubnet_amd import _lib
from fullsubnet_amd.long_form import HOP, N_FFT, LongPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fsn_fullsubnet_segment_state_bytes", "fsn_fullsubnet_segment_workspace_bytes", "fsn_fullsubnet_segment_stats",
           "fsn_fullsubnet_segment_fullband", "fsn_fullsubnet_segment_subband", "fsn_fullsubnet_segment_divisors"]
LA, F = 2, 257
# samples of: 700 samples (3 frames), 38 frames, 100 001 frames (one past Model.enhance's limit), three hours (675 001 frames)
RECORDINGS = [700, 37 * HOP + 165, 100000 * HOP + 5, 675000 * HOP]


def cfg(norm=0, arith=0):
    return _lib.Cfg(num_freqs=F, look_ahead=LA, sb_num_neighbors=15, fb_hidden=512, sb_hidden=384, norm_type=norm, arith=arith)


def test_entries_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(L, name), name
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;()]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


@pytest.mark.parametrize("samples", RECORDINGS)
@pytest.mark.parametrize("k", [1, 7, 19, 4096, None])
def test_segments_cover_every_model_step_once_and_in_order(samples, k):
    T = 1 + samples // HOP
    if k == 1 and T > 1000:
        k = 3  # a segment per frame of the long recordings is the same arithmetic, 675 003 tuples of it
    plan = LongPlan(cfg(), 1, samples, segment_frames=k)
    assert plan.frames == T and plan.steps == T + LA
    pos = 0
    for s0, n in plan.segments:
        assert s0 == pos and 1 <= n <= 4096
        pos += n
    assert pos == T + LA
    if k is not None:
        assert all(n == min(k, T + LA) for _, n in plan.segments[:-1])
    else:  # the largest segment whose workspace stays under the limit
        L = _lib.lib()
        kk = plan.segment_frames
        assert L.fsn_fullsubnet_segment_workspace_bytes(ctypes.byref(cfg()), 1, kk) <= 4 << 30
        assert kk == min(4096, T + LA) or L.fsn_fullsubnet_segment_workspace_bytes(ctypes.byref(cfg()), 1, kk + 1) > 4 << 30


def test_segment_edge_cases():
    samples = 37 * HOP + 165  # T = 38
    # T a multiple of k: the last segment holds only the look-ahead zero frames
    plan = LongPlan(cfg(), 2, samples, segment_frames=19)
    assert plan.segments == [(0, 19), (19, 19), (38, 2)]
    # a segment per step
    plan = LongPlan(cfg(), 2, samples, segment_frames=1)
    assert plan.segments == [(s, 1) for s in range(40)]
    # k >= T + la: one segment of exactly the steps there are
    for k in (40, 64, 4096):
        assert LongPlan(cfg(), 2, samples, segment_frames=k).segments == [(0, 40)]
    for bad in (0, -1, 4097):
        with pytest.raises(_lib.FsnError):
            LongPlan(cfg(), 2, samples, segment_frames=bad)
    with pytest.raises(_lib.FsnError):
        LongPlan(cfg(), 1, N_FFT // 2)  # no reflect padding possible
    # a workspace limit picks k: monotone, and below one frame's worth it is refused
    ks = [LongPlan(cfg(), 1, RECORDINGS[2], workspace_limit=lim).segment_frames for lim in (64 << 20, 1 << 30, 4 << 30)]
    assert ks[0] < ks[1] < ks[2] <= 4096
    with pytest.raises(_lib.FsnError):
        LongPlan(cfg(), 1, RECORDINGS[2], workspace_limit=1 << 20)


@pytest.mark.parametrize("samples", RECORDINGS)
@pytest.mark.parametrize("slab_frames", [2, 5, 4096])
def test_slabs_tile_the_recording(samples, slab_frames):
    T = 1 + samples // HOP
    if slab_frames < 4096 and T > 1000:
        slab_frames *= 1000
    plan = LongPlan(cfg(), 1, samples, segment_frames=64, slab_frames=slab_frames)
    frame, sample = 0, 0
    for t0, t1, (a, b), (o0, o1) in plan.slabs:
        assert t0 == frame and t0 < t1 <= T and t1 - t0 <= slab_frames
        assert o0 == sample and o1 > o0
        # the samples read hold every frame of the slab whole (frame t covers [t hop - 256, t hop + 256)), clipped to the recording
        assert 0 <= a <= max(t0 * HOP - N_FFT // 2, 0) and min((t1 - 1) * HOP + N_FFT // 2, samples) <= b <= samples
        assert b - a > N_FFT // 2  # longer than its own reflect padding
        frame, sample = t1, o1
    assert frame == T and sample == samples


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [256, 1024])  # fixed k: both shorter than the minute's 3753 steps
def test_planned_memory_grows_by_planes_of_F_floats_only(B, k):
    minute, hours3 = 60 * 16000, 3 * 3600 * 16000
    a, b = LongPlan(cfg(), B, minute, segment_frames=k), LongPlan(cfg(), B, hours3, segment_frames=k)
    extra_frames = b.frames - a.frames
    assert b.total_bytes == sum(b.bytes.values())
    assert 0 < b.total_bytes - a.total_bytes <= 8 * 1024 * extra_frames * B
    # no term proportional to T x hidden size: everything outside the linear planes is the same at one minute and at
    # three hours once a slab / a segment is full ...
    for name in a.bytes:
        if name not in LongPlan.LINEAR:
            assert b.bytes[name] - a.bytes[name] <= 8 * 1024 * 4096 * B, name
    # ... the linear planes are exactly F floats (a hop of samples for the result) per frame and row ...
    per_frame = {"mag": 4 * F, "spec_re": 4 * F, "spec_im": 4 * F, "fb_out": 4 * F, "mask": 8 * F}
    for name, n in per_frame.items():
        assert b.bytes[name] - a.bytes[name] == n * extra_frames * B, name
    assert b.bytes["enhanced"] == 4 * B * hours3
    # ... and state and workspace come from the library's queries and do not depend on the recording at all
    L = _lib.lib()
    assert a.bytes["state"] == b.bytes["state"] == L.fsn_fullsubnet_segment_state_bytes(ctypes.byref(cfg()), B)
    assert a.bytes["workspace"] == b.bytes["workspace"] == L.fsn_fullsubnet_segment_workspace_bytes(ctypes.byref(cfg()), B, k)
    # one sub-band hidden sequence of the three hours would be 272 rows x 384 units x 4 B per frame and row
    assert b.total_bytes < 0.03 * (272 * 384 * 4) * b.frames * B + b.bytes["workspace"] + b.bytes["state"]


@pytest.mark.parametrize("norm", [0, 1])
def test_size_queries(norm):
    L = _lib.lib()
    c = cfg(norm)
    state = lambda B: L.fsn_fullsubnet_segment_state_bytes(ctypes.byref(c), B)  # noqa: E731
    ws = lambda B, k: L.fsn_fullsubnet_segment_workspace_bytes(ctypes.byref(c), B, k)  # noqa: E731
    # (h, c) of the four layers, the cumulative norm's sums, per-bin fp64 sums [B][FP] and the fp64 full-band sum [B]
    for B in (1, 3, 17):
        rows_fb, rows_sb = (B + 15) // 16 * 16, (B * F + 15) // 16 * 16
        floor = 4 * 4 * (rows_fb * 512 + rows_sb * 384) + 8 * (B + B * F) + 8 * (B * 272 + B)
        assert floor <= state(B) <= floor + 16 * 256
    assert all(ws(1, k1) > ws(1, k0) > 0 for k0, k1 in ((1, 2), (2, 64), (64, 4096)))
    assert ws(2, 16) > ws(1, 16)
    # one sub-band hidden sequence of the segment alone: k x 272 rows x 384 floats
    assert ws(1, 64) >= 64 * 272 * 384 * 4
    for bad in ((0, 1), (-3, 1), (4097, 1), (1, 0), (1, -1), (1, 4097)):
        assert ws(*bad) == 0
        assert "out of range" in L.fsn_last_error().decode()
    for B in (0, 4097):
        assert state(B) == 0
        assert "out of range" in L.fsn_last_error().decode()
    assert L.fsn_fullsubnet_segment_state_bytes(None, 1) == 0 and "NULL" in L.fsn_last_error().decode()
    f16x3 = cfg(norm, arith=1)
    assert L.fsn_fullsubnet_segment_workspace_bytes(ctypes.byref(f16x3), 1, 1) == 0
    assert "fp32" in L.fsn_last_error().decode()


def test_streaming_enhancer_and_enhance_long_share_the_slab_helpers():
    import inspect

    from fullsubnet_amd import long_form, slabs, streaming
    for mod in (long_form, streaming):
        assert mod.analysis_slab is slabs.analysis_slab and mod.synthesis_slab is slabs.synthesis_slab
        src = inspect.getsource(mod)
        assert "istft(" not in src and " stft(" not in src  # the transforms themselves are called in slabs.py only


def test_the_three_plans_share_one_base_and_its_segments_and_slabs():
    import improved_stream_reference as R
    from fullsubnet_amd.fast_long_form import FastLongPlan
    from fullsubnet_amd.improved_fullsubnet import Model as ImprovedModel
    from fullsubnet_amd.improved_long_form import ImprovedLongPlan
    from fullsubnet_amd.long_form import SegmentPlan
    for cls in (LongPlan, FastLongPlan, ImprovedLongPlan):
        assert issubclass(cls, SegmentPlan) and cls is not SegmentPlan
        assert "slabs_of" not in vars(cls) and cls.slabs_of is SegmentPlan.slabs_of
    fast_cfg = _lib.FastCfg(F=F, num_mels=64, shrink=2, mel_neighbors=5, enc_neighbors=0, bn_hidden=384, bn_layers=2, norm=0)
    samples = 37 * HOP + 165  # T = 38 at 512 / 256
    a = LongPlan(cfg(), 2, samples, segment_frames=19, slab_frames=5)
    b = FastLongPlan(fast_cfg, LA, 2, samples, segment_frames=19, slab_frames=5)
    assert (a.frames, a.steps) == (b.frames, b.steps) == (38, 40)
    assert a.segments == b.segments == [(0, 19), (19, 19), (38, 2)]
    assert len(a.slabs) == 8 and a.slabs == b.slabs
    # Improved FullSubNet has no look-ahead and its own transform (960 / 480): 40 frames are the same 40 steps
    k48 = ImprovedModel(**R.as_dict(R.K48)).stream_cfg()
    c = ImprovedLongPlan(k48, 960, "offline", 2, 39 * 480 + 100, segment_frames=19)
    assert (c.frames, c.steps) == (40, 40) and c.segments == a.segments
    # ... and without a look-ahead the 38 frames are 38 steps on every plan
    d = FastLongPlan(fast_cfg, 0, 2, samples, segment_frames=19)
    e = ImprovedLongPlan(k48, 960, "offline", 2, 37 * 480 + 165, segment_frames=19)
    assert d.steps == e.steps == 38 and d.segments == e.segments == [(0, 19), (19, 19)]
