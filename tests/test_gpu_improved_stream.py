"""fsn_improved_stream_step and StreamingEnhancer(improved_model) against the fp64 step of tests/improved_stream_reference.py,
call by call, over its table: reduced configurations (row padding inside and between sections, both fdrc modes, differing
neighbour counts, two sections, a state written at 100 000 steps), the shipped 48 kHz configuration and the 16 kHz bins; every
row on a state blob poisoned outside its fields and in two chunkings, bit for bit; the enhancer end to end against the
whole-utterance model.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import improved_stream_reference as R
from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu
CAUSAL = dict(norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm")


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


_MODELS = {}


def model_of(cfg, **norms):
    from fullsubnet_amd.improved_fullsubnet import Model
    key = (cfg, tuple(sorted(norms.items())))
    if key not in _MODELS:
        m = Model(**R.as_dict(cfg), **norms)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_params(cfg).items()}, strict=True)
        _MODELS[key] = m.cuda().eval()
    return _MODELS[key]


# ---- the state blob through the layout query ----------------------------------------------------------------------------------

def _fields(lay, cfg, B):
    """(byte offset, dtype, shape in the blob, getter / setter path into a reference state, valid extent)."""
    out = []
    for a in range(4):
        out.append((lay["fb"][a], np.float32, (lay["rows"], cfg.fb_hidden), ("fb", a // 2, a % 2), (B, cfg.fb_hidden)))
    for i, n in enumerate(R.num_units(cfg)):
        for a in range(4):
            out.append((lay["sb"][i][a], np.float32, (lay["sb_rows"][i], cfg.sb_hidden), ("sb", i, a // 2, a % 2), (B * n, cfg.sb_hidden)))
    S = len(cfg.centers)
    out += [(lay["fb_sum"], np.float64, (B,), ("fb_sum",), (B,)), (lay["sb_sum"], np.float64, (S, B), ("sb_sum",), (S, B)),
            (lay["steps"], np.int64, (B,), ("steps",), (B,))]
    return out


def _view(host, off, dtype, shape):
    return host[off:off + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)


def _get(st, path):
    for p in path:
        st = st[p]
    return st


def write_state(lay, cfg, B, st, dev):
    """The blob of the reference state `st`: every field the layout names zero outside its valid extent, every byte outside
    the fields 0xFF (a NaN pattern in either float width: a kernel that reads one shows it)."""
    host = np.full(lay["bytes"], 0xFF, dtype=np.uint8)
    for off, dtype, shape, path, valid in _fields(lay, cfg, B):
        view = _view(host, off, dtype, shape)
        view[...] = 0
        view[tuple(slice(0, n) for n in valid)] = np.asarray(_get(st, path)).reshape(valid) if path != ("steps",) else st["steps"]
    return torch.from_numpy(host).to(dev)


def read_state(lay, cfg, B, blob):
    """The blob as a state dict of the reference; every byte outside the fields is still the 0xFF it was written with."""
    host = blob.cpu().numpy()
    st = R.new_state(B, cfg)
    covered = np.zeros(lay["bytes"], dtype=bool)
    for off, dtype, shape, path, valid in _fields(lay, cfg, B):
        view = _view(host, off, dtype, shape)
        covered[off:off + view.nbytes] = True
        a = view[tuple(slice(0, n) for n in valid)].copy()
        if path == ("steps",):
            assert (a == a[0]).all()
            st["steps"] = int(a[0])
        elif len(path) == 1:
            st[path[0]] = a
        else:
            _get(st, path[:-1])[path[-1]] = a
            assert np.isfinite(view).all(), f"{path}: a padded row is not finite"
    assert (host[~covered] == 0xFF).all(), "a byte outside the fields of the layout was written"
    return st


def run_calls(fsn, model, B, split, mag, state0, steps0=0, form=None):
    """The calls `split` of fsn_improved_stream_step on mag [B, F, T] -> ([mask per call], final blob).  form: 0 / 1 runs
    the sections' blocks as per-section chains / with the multi-set step launch (None: the library's default)."""
    L, _lib = fsn._lib.lib(), fsn._lib
    default = L.fsn_debug_improved_stream_form(-1)
    if form is not None:
        assert L.fsn_debug_improved_stream_form(form) == form
    try:
        return _run_calls(L, _lib, model, B, split, mag, state0, steps0)
    finally:
        L.fsn_debug_improved_stream_form(default)


def _run_calls(L, _lib, model, B, split, mag, state0, steps0):
    cfg = model.stream_cfg()
    dev = torch.device("cuda")
    blob = state0.clone()
    assert blob.numel() == L.fsn_improved_stream_state_bytes(ctypes.byref(cfg), B)
    packed = model.stream_packed_weights()
    x = torch.from_numpy(mag).to(dev)
    out, t0 = [], steps0
    for k in split:
        chunk = x[..., t0 - steps0:t0 - steps0 + k].contiguous()
        mask = torch.full((B, 2, x.shape[1], k), float("nan"), dtype=torch.float32, device=dev)
        ws = _lib.workspace(L.fsn_improved_stream_workspace_bytes(ctypes.byref(cfg), B, k), dev)
        ws.fill_(0xFF)  # nothing of the workspace may be read before the call wrote it
        _lib.check(L.fsn_improved_stream_step(ctypes.byref(cfg), packed.data_ptr(), blob.data_ptr(), blob.numel(), t0,
                                              _lib.dev_ptr(chunk, "mag"), B, k, _lib.dev_ptr(mask), ws.data_ptr(), ws.numel(),
                                              _lib.stream_ptr(dev)))
        out.append(mask)
        t0 += k
    torch.cuda.synchronize()
    return out, blob


def other_split(split):
    """Another chunking of the same frames: frame by frame, or in one call where the row already runs frame by frame."""
    T = sum(split)
    return (T,) if set(split) == {1} else (1,) * T


@pytest.mark.parametrize("row", R.TABLE, ids=lambda r: r.id)
def test_improved_stream_sweep(fsn, row):
    """Every call's masks and the final state against the fp64 step (SHARP x the fp32 cell emulation: whole tensor, per frame,
    per 16-row tile; the sums by their bounds), from a blob whose bytes outside the layout's fields are poisoned and stay so.
    A second chunking of the same frames gives the same masks and the same blob, bit for bit, and so do the per-section
    chains in place of the multi-set step launch, in both chunkings.  The resumed row starts from a
    state written through the layout query at 100 000 steps and is called with that steps_done."""
    ref = R.reference_of(row)
    model = model_of(row.cfg, **CAUSAL)
    lay = fsn._lib.improved_stream_state_layout(model.stream_cfg(), row.B)
    steps0 = row.resumed or 0
    state0 = write_state(lay, row.cfg, row.B, ref.state0, torch.device("cuda"))
    got, blob = run_calls(fsn, model, row.B, row.split, ref.mag, state0, steps0)
    worst = R.check_calls(row, ref, [g.cpu().numpy() for g in got])
    state = R.check_state(row, ref, read_state(lay, row.cfg, row.B, blob))
    print(f"[isweep] {row.id}: mask worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x; state worst "
          f"{max(state.values()):.2f} x ({max(state, key=state.get)})")
    again, blob_b = run_calls(fsn, model, row.B, other_split(row.split), ref.mag, state0, steps0)
    assert torch.equal(torch.cat(got, dim=-1), torch.cat(again, dim=-1))
    assert torch.equal(blob, blob_b)
    # the two forms of the sections' blocks: the multi-set step launch and a chain of launches per section
    other = 1 - fsn._lib.lib().fsn_debug_improved_stream_form(-1)  # the runs above took the library's default
    for split in (row.split, other_split(row.split)):
        others, blob_c = run_calls(fsn, model, row.B, split, ref.mag, state0, steps0, form=other)
        assert torch.equal(torch.cat(got, dim=-1), torch.cat(others, dim=-1))
        assert torch.equal(blob, blob_c)


def test_a_zero_filled_blob_is_a_new_stream(fsn):
    """All zeros (what StreamingEnhancer.reset allocates) is the state the table's rows write through the layout."""
    row = next(r for r in R.TABLE if r.why == "mixed")
    ref = R.reference_of(row)
    model = model_of(row.cfg, **CAUSAL)
    lay = fsn._lib.improved_stream_state_layout(model.stream_cfg(), row.B)
    dev = torch.device("cuda")
    a, _ = run_calls(fsn, model, row.B, row.split, ref.mag, torch.zeros(lay["bytes"], dtype=torch.uint8, device=dev))
    b, _ = run_calls(fsn, model, row.B, row.split, ref.mag, write_state(lay, row.cfg, row.B, ref.state0, dev))
    assert torch.equal(torch.cat(a, dim=-1), torch.cat(b, dim=-1))


def test_step_refuses_short_buffers_before_anything_is_launched(fsn):
    L, _lib = fsn._lib.lib(), fsn._lib
    model = model_of(R.SMALL, **CAUSAL)
    cfg = model.stream_cfg()
    dev = torch.device("cuda")
    nbytes = L.fsn_improved_stream_state_bytes(ctypes.byref(cfg), 1)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    mag = torch.ones((1, R.SMALL.F, 1), device=dev)
    mask = torch.zeros((1, 2, R.SMALL.F, 1), device=dev)
    ws = _lib.workspace(L.fsn_improved_stream_workspace_bytes(ctypes.byref(cfg), 1, 1), dev)
    args = lambda sb, wb: (ctypes.byref(cfg), model.stream_packed_weights().data_ptr(), blob.data_ptr(), sb, 0, _lib.dev_ptr(mag), 1, 1,  # noqa: E731
                           _lib.dev_ptr(mask), ws.data_ptr(), wb, _lib.stream_ptr(dev))
    assert L.fsn_improved_stream_step(*args(nbytes - 1, ws.numel())) == -2 and b"too small" in L.fsn_last_error()
    assert L.fsn_improved_stream_step(*args(nbytes, ws.numel() - 1)) == -2
    torch.cuda.synchronize()
    assert not blob.any() and not mask.any()  # nothing was launched


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def run_stream(model, noisy, sizes):
    from fullsubnet_amd.streaming import StreamingEnhancer
    enh = StreamingEnhancer(model, batch_size=noisy.shape[0])
    out, pos, lat = [], 0, []
    for n in sizes:
        out.append(enh.process(noisy[:, pos:pos + n]))
        pos += n
        lat.append(pos - sum(o.shape[1] for o in out))
    assert pos == noisy.shape[1]
    out.append(enh.flush())
    return torch.cat(out, dim=1), lat, enh


def uneven_sizes(L, seed, top):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < L:
        sizes.append(int(min(2 * rng.integers(0, top) + 1, L - sum(sizes))))
    return sizes


def test_streaming_enhancer_equals_the_whole_utterance_at_48k(fsn):
    """StreamingEnhancer(improved_model) on half a second at 48 kHz in uneven chunks + flush = model(y) of the whole utterance
    to 1e-4 of its peak (the bound tests/test_gpu_fast_stream.py holds the same comparison to); 480-sample chunks give the
    same bits; no sample leaves later than two hops after it came in; the transform is the model's own 960 / 480."""
    model = model_of(R.K48, **CAUSAL)
    L = 24011
    noisy = torch.from_numpy(O.make_noisy(1, L, seed=17)).cuda()
    a, lat_a, enh = run_stream(model, noisy, uneven_sizes(L, 3, 900))
    assert (enh.n_fft, enh.hop) == (960, 480)
    b, lat_b, _ = run_stream(model, noisy, [480] * (L // 480) + [L % 480])
    assert a.shape == noisy.shape and torch.isfinite(a).all()
    with torch.no_grad():
        offline = model(noisy)[:, 0]
    scale = offline.abs().max().item()
    err = (a - offline).abs().max().item()
    print(f"[isweep] 48 kHz: stream against the whole utterance {err:.3e}, peak {scale:.3e} ({err / scale:.2e} of it)")
    assert scale > 0 and err <= 1e-4 * scale
    assert torch.equal(a, b)
    assert max(lat_a + lat_b) <= 2 * 480
    enh.reset()
    assert torch.equal(torch.cat([enh.process(noisy), enh.flush()], dim=1), a)


def test_streaming_enhancer_refusals_on_the_device(fsn):
    """Norms that are not causal (the key to set is named), a hop that is not n_fft / 2, and a flushed enhancer."""
    from fullsubnet_amd.improved_fullsubnet import Model
    from fullsubnet_amd.streaming import StreamingEnhancer
    from oracle import model_family_oracle as MF
    with pytest.raises(ValueError, match="norm_type = 'cumulative_laplace_norm'"):
        StreamingEnhancer(model_of(R.SMALL))
    with pytest.raises(ValueError, match="sb_norm_type = 'cumulative_laplace_norm'"):
        StreamingEnhancer(model_of(R.SMALL, norm_type="cumulative_laplace_norm"))
    with pytest.raises(NotImplementedError, match="512 / 128"):
        StreamingEnhancer(Model(**dict(MF.IMPROVED_16K, **CAUSAL)).cuda())
    with pytest.raises(NotImplementedError, match="LSTM"):
        StreamingEnhancer(Model(**dict(R.as_dict(R.SMALL), sequence_model="GRU", **CAUSAL)).cuda())
    enh = StreamingEnhancer(model_of(R.SMALL, **CAUSAL))
    assert (enh.n_fft, enh.hop) == (64, 32)
    noisy = torch.from_numpy(O.make_noisy(1, 500, seed=2)).cuda()
    out = torch.cat([enh.process(noisy), enh.flush()], dim=1)
    assert out.shape == noisy.shape and torch.isfinite(out).all()
    with pytest.raises(RuntimeError, match="flush"):
        enh.process(noisy)
    with pytest.raises(RuntimeError, match="flushed"):
        enh.flush()
