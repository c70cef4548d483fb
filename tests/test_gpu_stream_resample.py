"""fsn_resample_stream_* on the device (fullsubnet_amd.StreamResampler): a session fed chunk by chunk gives,
bit for bit, fsn_resample of its whole input - whatever the chunking, whoever shares the launch.
Needs an MI355X:  python -m pytest tests -m gpu"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(a, b, "scipy") for a, b in R.RATIOS] + [(a, b, "sharp") for a, b in R.SHARP_RATIOS]
IDS = [f"{a}to{b}-{design}" for a, b, design in CASES]
N = 4099


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def geometry(sr_in, sr_out, design):
    u, d = R.ratio(sr_in, sr_out)
    if u == d == 1:
        return 1, 1, 0, 1
    H = R.DESIGNS[design][0] * max(u, d)
    return u, d, H, -(-(2 * H + 1) // u)


def fill(sizes, n, rng, high):
    sizes = list(sizes)
    while sum(sizes) < n:
        sizes.append(int(min(rng.integers(0, high), n - sum(sizes))))
    return sizes


def edge_sizes(n, u, d, H, rng):
    """Chunks that end one sample before, exactly where and one sample after n_in u - H - 1 is a multiple of d - the
    counts at which one more output becomes due -, at three places of the row."""
    ends = []
    for start in (n // 7, n // 2, n - 300):
        at = next(m for m in range(start, n) if m * u > H and (m * u - H - 1) % d == 0)
        ends += [at - 1, at, at + 1]
    ends = sorted(set(e for e in ends if 0 < e < n)) + [n]
    return [b - a for a, b in zip([0] + ends[:-1], ends)]


def stream(rs, row, sizes, poison=False):
    """One session: the row in chunks of ``sizes``, then close."""
    sid, parts, pos = rs.open(), [], 0
    for c in sizes:
        parts.append(rs.push({sid: row[pos:pos + c]}, poison=poison)[sid])
        pos += c
    assert pos == row.numel()
    parts.append(rs.close(sid))
    return torch.cat(parts)


@pytest.mark.parametrize("sr_in,sr_out,design", CASES, ids=IDS)
def test_chunked_equals_whole_bit_for_bit(fsn, sr_in, sr_out, design):
    u, d, H, J = geometry(sr_in, sr_out, design)
    rng = np.random.default_rng(1000 * sr_in + sr_out)
    row = torch.from_numpy(R.signal(N, seed=77 + sr_in + 3 * sr_out)).cuda()
    whole = fsn.resample.resample(row, sr_in, sr_out, design=design)[0]
    assert whole.numel() == R.out_length(N, sr_in, sr_out)
    rs = fsn.StreamResampler(sr_in, sr_out, capacity=2, design=design)
    schedules = {"ones": fill([1] * (J + 3), N, rng, 900), "random": fill([0, 5, 0], N, rng, 900),
                 "edges": edge_sizes(N, u, d, H, rng)}
    assert 0 in schedules["random"] and all(sum(s) == N for s in schedules.values())
    for name, sizes in schedules.items():
        got = stream(rs, row, sizes, poison=True)
        assert got.shape == whole.shape, name
        assert torch.equal(got, whole), (name, (got - whole).abs().max().item())
    # rows shorter than the filter, and the whole row, pushed once with the end of the input
    for n in sorted({1, 2, max(1, H // max(u, 1)), N}):
        sid = rs.open()
        got = rs.push({sid: row[:n]}, final=(sid,), poison=True)[sid]
        assert rs.close(sid).numel() == 0
        assert torch.equal(got, fsn.resample.resample(row[:n], sr_in, sr_out, design=design)[0]), n


def test_sessions_are_independent(fsn):
    sr_in, sr_out = 441, 160  # 160 phases: the five sessions stand at different ones
    rows = [torch.from_numpy(R.signal(3000, seed=500 + i)).cuda() for i in range(5)]
    before = [0, 37, 500, 1001, 64]      # where each session stands when the shared push comes
    chunk = [300, 0, 123, 1, 700]        # one empty chunk; session 2 ends with its chunk
    rs = fsn.StreamResampler(sr_in, sr_out, capacity=5)
    sids = [rs.open() for _ in range(5)]
    assert [rs.slot(s) for s in sids] == list(range(5))
    head = rs.push({s: rows[i][:before[i]] for i, s in enumerate(sids)})
    state0 = rs.state.clone()
    calls = rs.calls
    got = rs.push({s: rows[i][before[i]:before[i] + chunk[i]] for i, s in enumerate(sids)}, final=(sids[2],), poison=True)
    assert rs.calls == calls + 1  # one library call for the five
    full = rs.last_rows
    assert torch.isfinite(full).all()
    for i, s in enumerate(sids):
        assert not full[i, got[s].numel():].any(), i  # zeros behind the row's count
    for i, s in enumerate(sids):
        alone = fsn.StreamResampler(sr_in, sr_out, capacity=1)
        a = alone.open()
        h = alone.push({a: rows[i][:before[i]]})[a]
        g = alone.push({a: rows[i][before[i]:before[i] + chunk[i]]}, final=(a,) if i == 2 else ())[a]
        assert torch.equal(h, head[s]) and torch.equal(g, got[s]), i
        assert g.numel() > 0 or chunk[i] <= 1
    # the slots: sessions that received samples (and go on) left a new history, the others were not written
    for i in range(5):
        changed = not torch.equal(rs.slot_bytes(i), state0[rs.slot_bytes(i).storage_offset():][:rs.slot_bytes(i).numel()])
        assert changed == (chunk[i] > 0 and i != 2), i
    # two of five listed: the other three slots keep their bytes
    state1 = rs.state.clone()
    rs.push({sids[0]: rows[0][300:900], sids[4]: rows[4][764:765]})
    off = rs.slot_bytes(0).storage_offset()
    assert torch.equal(rs.state[:off], state1[:off])  # the header with the table
    for i in range(5):
        view = rs.slot_bytes(i)
        same = torch.equal(view, state1[view.storage_offset():][:view.numel()])
        assert same == (i not in (0, 4)), i


def test_reset_and_reuse(fsn):
    row = torch.from_numpy(R.signal(2500, seed=9)).cuda()
    other = torch.from_numpy(R.signal(1800, seed=10)).cuda()
    sizes = [700, 1, 0, 999, 800]
    fresh = stream(fsn.StreamResampler(48000, 16000, capacity=2), row, sizes)
    assert torch.equal(fresh, fsn.resample.resample(row, 48000, 16000)[0])
    rs = fsn.StreamResampler(48000, 16000, capacity=2)
    keep = rs.open()
    stream(rs, other, [1000, 800])  # slot 1, used and closed
    assert rs.slot(keep) == 0 and not rs.slot_bytes(1).any()
    assert torch.equal(stream(rs, row, sizes), fresh)  # the same slot again
    # reset() in mid-stream: the session starts over
    rs.push({keep: other[:777]})
    assert rs.slot_bytes(0).any()
    rs.reset(keep)
    assert not rs.slot_bytes(0).any()
    parts, pos = [], 0
    for c in sizes:
        parts.append(rs.push({keep: row[pos:pos + c]})[keep])
        pos += c
    assert torch.equal(torch.cat(parts + [rs.close(keep)]), fresh)


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (16000, 44100), (16000, 16000)])
def test_exact_zeros_and_fully_written_outputs(fsn, sr_in, sr_out):
    rs = fsn.StreamResampler(sr_in, sr_out, capacity=3)
    a, b = rs.open(), rs.open()
    zeros = torch.zeros(2000, device="cuda")
    noise = torch.from_numpy(R.signal(2000, seed=4)).cuda()
    outs = []
    for lo, hi in ((0, 700), (700, 701), (701, 2000)):
        got = rs.push({a: zeros[lo:hi], b: noise[lo // 2:hi // 2]}, poison=True)  # b: half as many samples, fewer outputs
        assert torch.isfinite(rs.last_rows).all()
        assert not rs.last_rows[1, got[b].numel():].any() and not rs.last_rows[0, got[a].numel():].any()
        outs.append(got[a])
    outs.append(rs.close(a))
    z = torch.cat(outs)
    assert z.numel() == R.out_length(2000, sr_in, sr_out)
    assert not z.any() and not torch.signbit(z).any()  # exact zeros, and +0.0 like the offline call's
    if sr_in == sr_out:  # the identity passes chunks through with no delay
        c = rs.open()
        assert torch.equal(rs.push({c: noise[:33]})[c], noise[:33])


def test_past_two_to_the_31(fsn):
    """44.1 -> 16 kHz: k d passes 2^31 at output 4 869 576 of 4 897 960; chunks of a million samples tile over 1418
    workgroups each."""
    n = 13_500_000
    g = torch.Generator(device="cuda").manual_seed(5)
    row = torch.randn(n, generator=g, device="cuda")
    whole = fsn.resample.resample(row, 44100, 16000)[0]
    assert (whole.numel() - 1) * 441 > 2 ** 31
    rs = fsn.StreamResampler(44100, 16000, capacity=1)
    got = stream(rs, row, [1_000_000] * 13 + [500_000])
    assert got.shape == whole.shape
    assert torch.equal(got, whole)


def test_refusals_leave_the_state_alone(fsn):
    _lib = fsn._lib
    L = _lib.lib()
    rs = fsn.StreamResampler(48000, 16000, capacity=4)
    sid = rs.open()
    rs.push({sid: torch.from_numpy(R.signal(500, seed=1)).cuda()})
    state0 = rs.state.clone()
    st, nb = rs.state.data_ptr(), rs.state.numel()
    items = torch.tensor([[0, 8, 0, 1, 500, 157, 3, 0]], dtype=torch.int64, device="cuda")
    x = torch.ones((4, 8), device="cuda")
    y = torch.full((4, 8), float("nan"), device="cuda")
    s = _lib.stream_ptr()
    push = lambda state, nbytes, cap, a, b, z, n, it=items, xx=x, yy=y, C=8, Om=8: L.fsn_resample_stream_push(
        state, nbytes, cap, a, b, z, it.data_ptr() if it is not None else None, n, xx.data_ptr() if xx is not None else None, C,
        yy.data_ptr() if yy is not None else None, Om, s)
    bad = [push(st, nb, 4, 0, 16000, 10, 1), push(st, nb, 4, 48000, 16000, 0, 1), push(st, nb, 4, 48000, 48001, 10, 1),
           push(st, nb, 0, 48000, 16000, 10, 1), push(st, nb, 4, 48000, 16000, 10, 0), push(st, nb, 4, 48000, 16000, 10, 5),
           push(st, nb - 256, 4, 48000, 16000, 10, 1), push(st, nb, 3, 48000, 16000, 10, 1), push(st, nb, 4, 44100, 16000, 10, 1),
           push(st + 4, nb, 4, 48000, 16000, 10, 1), push(None, nb, 4, 48000, 16000, 10, 1),
           push(st, nb, 4, 48000, 16000, 10, 1, it=None), push(st, nb, 4, 48000, 16000, 10, 1, xx=None),
           push(st, nb, 4, 48000, 16000, 10, 1, yy=None), push(st, nb, 4, 48000, 16000, 10, 1, C=0),
           push(st, nb, 4, 48000, 16000, 10, 1, Om=0), push(st, nb, 4, 48000, 16000, 10, 1, yy=x)]
    assert bad == [-1] * len(bad), bad
    ids = torch.tensor([0], dtype=torch.int32, device="cuda")
    assert L.fsn_resample_stream_reset(st, nb, 4, 48000, 16000, 10, ids.data_ptr(), 0, s) == -1
    assert L.fsn_resample_stream_reset(st, nb, 4, 48000, 16000, 10, ids.data_ptr(), 5, s) == -1
    assert L.fsn_resample_stream_reset(st, nb + 256, 4, 48000, 16000, 10, ids.data_ptr(), 1, s) == -1
    assert L.fsn_resample_stream_reset(st, nb, 4, 48000, 16000, 10, None, 1, s) == -1
    assert L.fsn_resample_stream_init(st, nb, 5, 48000, 16000, 10, 5.0, 1.0, s) == -1
    assert L.fsn_resample_stream_init(st, nb, 4, 48000, 16000, 10, 5.0, 1.5, s) == -1
    assert L.fsn_resample_stream_state_bytes(48000, 16000, 10, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(rs.state, state0)
    assert torch.isnan(y).all()  # and nothing was launched
    # Python: no host fallback
    with pytest.raises(_lib.FsnError, match="ROCm"):
        rs.push({sid: torch.zeros(10)})
    with pytest.raises(_lib.FsnError):
        rs.push({sid: [0.0, 1.0]})
    with pytest.raises(_lib.FsnError, match="ROCm"):
        fsn.StreamResampler(48000, 16000, device="cpu")
    with pytest.raises(ValueError):
        rs.push({sid: torch.zeros((2, 3), device="cuda")})
    with pytest.raises(KeyError):
        rs.push({sid + 7: torch.zeros(3, device="cuda")})
    with pytest.raises(RuntimeError, match="full"):
        for _ in range(4):
            rs.open()
    assert torch.equal(rs.state, state0)
    # an item that points outside the blob or its rows is clamped on the device: zeros, nothing written elsewhere
    wild = torch.tensor([[9, 8, 0, 0, 0, 0, 8, 0], [-1, 1 << 40, 0, 1, 0, 0, 1 << 40, 0]], dtype=torch.int64, device="cuda")
    assert push(st, nb, 4, 48000, 16000, 10, 2, it=wild) == 0
    torch.cuda.synchronize()
    assert torch.equal(rs.state, state0) and not y[:2].any() and torch.isnan(y[2:]).all()
