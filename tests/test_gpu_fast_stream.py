"""fsn_fast_stream_step and StreamingEnhancer(fast_model) against the fp64 step of tests/fast_stream_reference.py, call by
call, over its table: row padding and a second row tile, every (shrink, look-ahead) pair, both neighbour settings and
bottlenecks, frame-by-frame / mixed / one-call chunkings, states written at 100 000 and 100 001 steps; two chunkings of the
same frames bit for bit; the enhancer end to end against the whole-utterance model.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import fast_stream_reference as R
from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


_MODELS = {}


def model_of(cfg, norm="cumulative_laplace_norm"):
    from fullsubnet_amd.fast_fullsubnet import Model
    if (cfg, norm) not in _MODELS:
        m = Model(look_ahead=cfg.la, shrink_size=cfg.shrink, sequence_model="LSTM", num_mels=R.M, encoder_input_size=R.F,
                  bottleneck_hidden_size=cfg.bn_hidden, bottleneck_num_layers=cfg.bn_layers, noisy_input_num_neighbors=cfg.n_mel,
                  encoder_output_num_neighbors=cfg.n_enc, norm_type=norm)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_params(cfg).items()}, strict=True)
        _MODELS[(cfg, norm)] = m.cuda().eval()
    return _MODELS[(cfg, norm)]


# ---- the state blob through the layout query ----------------------------------------------------------------------------------

def _fields(lay, cfg, B):
    """(name of the layout, dtype, shape in the blob, (key, layer, index) or key of the reference state, valid extent)."""
    rows, H = lay["rows"], cfg.bn_hidden
    out = []
    for key, width, real in (("enc0", 384, 384), ("enc1", lay["enc1_hidden"], 257), ("dec0", 512, 512), ("dec1", 512, 512)):
        for i, hc in enumerate("hc"):
            out.append((f"{key}_{hc}", np.float32, (rows, width), (key, 0, i), (B, real)))
    for l in range(cfg.bn_layers):
        for i, hc in enumerate("hc"):
            out.append((f"bn_{hc}{l}", np.float32, (B * R.M, H), ("bn", l, i), (B * R.M, H)))
    W = lay["unit_width"]
    out += [("mel_sum", np.float64, (B,), "mel_sum", (B,)), ("unit_sum", np.float64, (B, R.M), "unit_sum", (B, R.M)),
            ("partial", np.float32, (B, R.M, W), "partial", (B, R.M, W)), ("held", np.float32, (B, R.M), "held", (B, R.M))]
    return out


def write_state(lay, cfg, B, st, dev):
    host = np.zeros(lay["bytes"], dtype=np.uint8)
    for name, dtype, shape, src, valid in _fields(lay, cfg, B):
        view = host[lay[name]:lay[name] + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
        a = st[src[0]][src[1]][src[2]] if isinstance(src, tuple) else st[src]
        view[tuple(slice(0, n) for n in valid)] = np.asarray(a).reshape(valid)
    return torch.from_numpy(host).to(dev)


def read_state(lay, cfg, B, blob):
    """The blob as a state dict of the reference; "steps" is None: the count is an argument of the entry, not a field."""
    host = blob.cpu().numpy()
    st = R.new_state(B, cfg)
    for name, dtype, shape, src, valid in _fields(lay, cfg, B):
        view = host[lay[name]:lay[name] + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)
        a = view[tuple(slice(0, n) for n in valid)].copy()
        if isinstance(src, tuple):
            st[src[0]][src[1]][src[2]] = a
            if name.startswith("enc1"):  # the padding of 257 -> 320 units: zero weights keep h = c = 0
                assert not view[:, 257:].any(), f"{name}: a padded unit left zero"
        else:
            st[src] = a
    st["steps"] = None
    return st


def run_calls(fsn, model, B, split, mag, state0=None, steps0=0):
    """The calls `split` of fsn_fast_stream_step on mag [B, 1, F, T] -> ([crm per call] as numpy, final blob, layout)."""
    L, _lib = fsn._lib.lib(), fsn._lib
    cfg = model.stream_cfg()
    lay = _lib.fast_stream_state_layout(cfg, B)
    dev = torch.device("cuda")
    blob = torch.zeros(lay["bytes"], dtype=torch.uint8, device=dev) if state0 is None else state0
    assert blob.numel() == L.fsn_fast_stream_state_bytes(ctypes.byref(cfg), B)
    packed = model.stream_packed_weights()
    x = torch.from_numpy(mag).to(dev)
    out, t0 = [], steps0
    for k in split:
        chunk = x[..., t0 - steps0:t0 - steps0 + k].contiguous()
        crm = torch.full((B, 2, R.F, k), float("nan"), dtype=torch.float32, device=dev)
        ws = _lib.workspace(L.fsn_fast_stream_workspace_bytes(ctypes.byref(cfg), B, k), dev)
        _lib.check(L.fsn_fast_stream_step(ctypes.byref(cfg), packed.data_ptr(), blob.data_ptr(), blob.numel(), t0, _lib.dev_ptr(chunk, "mag"),
                                          B, k, _lib.dev_ptr(crm), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        out.append(crm)
        t0 += k
    torch.cuda.synchronize()
    return out, blob, lay


@pytest.mark.parametrize("row", R.TABLE, ids=lambda r: r.id)
def test_fast_stream_sweep(fsn, row):
    """Every call's masks and the final state against the fp64 step (SHARP x the fp32 cell emulation: whole tensor, per frame,
    per 16-row tile; the sums by their bounds).  A resumed row starts from a state written through the layout query at
    100 000 / 100 001 steps and called with that steps_done: both phases of a block of 2, the running sums and the divisors'
    counts at that length."""
    ref = R.reference_of(row)
    model = model_of(row.cfg)
    cfg = model.stream_cfg()
    lay = fsn._lib.fast_stream_state_layout(cfg, row.B)
    state0, steps0 = None, 0
    if row.resumed is not None:
        state0, steps0 = write_state(lay, row.cfg, row.B, ref.state0, torch.device("cuda")), row.resumed
        assert (R.open_frames(steps0, row.cfg.shrink) > 0) == bool(ref.state0["partial"].any())
    got, blob, _ = run_calls(fsn, model, row.B, row.split, ref.mag, state0, steps0)
    worst = R.check_calls(row, ref, [g.cpu().numpy() for g in got])
    state = R.check_state(row, ref, read_state(lay, row.cfg, row.B, blob))
    print(f"[fsweep] {row.id}: crm worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x; state worst "
          f"{max(state.values()):.2f} x ({max(state, key=state.get)})")


@pytest.mark.parametrize("cfg,B", [(R.SHIPPED, 3), (R.Cfg(shrink=3, la=1, n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1), 17),
                                   (R.Cfg(shrink=4, la=2), 1), (R.Cfg(shrink=1, la=0), 16)], ids=str)
def test_chunking_is_invisible(fsn, cfg, B):
    """Two chunkings of the same frames: every mask and the final state blob bit for bit (a third: the whole stream in one
    call)."""
    model = model_of(cfg)
    T = sum(R.MIXED)
    mag = R.make_mag(B, T, seed=77)
    a, blob_a, _ = run_calls(fsn, model, B, R.MIXED, mag)
    b, blob_b, _ = run_calls(fsn, model, B, (1,) * T, mag)
    c, blob_c, _ = run_calls(fsn, model, B, (T,), mag)
    a, b = torch.cat(a, dim=-1), torch.cat(b, dim=-1)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and torch.equal(a, c[0])
    assert torch.equal(blob_a, blob_b) and torch.equal(blob_a, blob_c)


@pytest.mark.parametrize("cfg,B,steps0", [(R.SHIPPED, 3, 5), (R.Cfg(shrink=3, la=1, n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1), 17, 8),
                                          (R.Cfg(shrink=4, la=2), 1, R.LONG + 3)], ids=str)
def test_call_without_a_completed_frame_leaves_the_bottleneck_alone(fsn, cfg, B, steps0):
    """A k = 1 call at a step t % shrink != 0 (n_low = 0): the bottleneck's (h, c), the unit norm's sums and the held output
    are bit for bit what they were, the masks take the held output (finite, not the NaN they were filled with), and the open
    block's sum, the mel norm's sum and the other blocks' states moved.  The next call, at a multiple of shrink, moves them."""
    assert steps0 % cfg.shrink and (steps0 + 1) % cfg.shrink == 0
    model = model_of(cfg)
    lay = fsn._lib.fast_stream_state_layout(model.stream_cfg(), B)
    state0 = R.random_state(B, cfg, steps0, R.LEVEL, seed=23)
    blob = write_state(lay, cfg, B, state0, torch.device("cuda"))
    before = read_state(lay, cfg, B, blob)
    mag = R.make_mag(B, 2, seed=9)
    got, blob, _ = run_calls(fsn, model, B, (1,), mag[..., :1], blob, steps0)
    after = read_state(lay, cfg, B, blob)
    assert torch.isfinite(got[0]).all()
    for l in range(cfg.bn_layers):
        for i in range(2):
            assert np.array_equal(after["bn"][l][i], before["bn"][l][i]), f"bottleneck layer {l} {'hc'[i]} changed"
    assert np.array_equal(after["unit_sum"], before["unit_sum"]) and np.array_equal(after["held"], before["held"])
    w_mel = 2 * cfg.n_mel + 1  # the mel columns of a window are positive, the encoder's (after its ReLU) may be zero
    assert (after["partial"] >= before["partial"]).all() and (after["partial"][..., :w_mel] > before["partial"][..., :w_mel]).all()
    assert (after["mel_sum"] > before["mel_sum"]).all()
    for key in ("enc0", "enc1", "dec0", "dec1"):
        assert not np.array_equal(after[key][0][0], before[key][0][0])
    got, blob, _ = run_calls(fsn, model, B, (1,), mag[..., 1:], blob, steps0 + 1)
    last = read_state(lay, cfg, B, blob)
    assert not np.array_equal(last["bn"][0][0], after["bn"][0][0]) and (last["unit_sum"] > after["unit_sum"]).all()
    assert not last["partial"].any() and not np.array_equal(last["held"], after["held"])


def test_step_refuses_short_buffers_and_the_offline_norm(fsn):
    L, _lib = fsn._lib.lib(), fsn._lib
    model = model_of(R.SHIPPED)
    cfg = model.stream_cfg()
    dev = torch.device("cuda")
    nbytes = L.fsn_fast_stream_state_bytes(ctypes.byref(cfg), 1)
    blob = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    mag = torch.ones((1, 1, R.F, 1), device=dev)
    crm = torch.zeros((1, 2, R.F, 1), device=dev)
    ws = _lib.workspace(L.fsn_fast_stream_workspace_bytes(ctypes.byref(cfg), 1, 1), dev)
    args = lambda sb, wb: (ctypes.byref(cfg), model.stream_packed_weights().data_ptr(), blob.data_ptr(), sb, 0, _lib.dev_ptr(mag), 1, 1,  # noqa: E731
                           _lib.dev_ptr(crm), ws.data_ptr(), wb, _lib.stream_ptr(dev))
    assert L.fsn_fast_stream_step(*args(nbytes - 1, ws.numel())) == -2 and b"too small" in L.fsn_last_error()
    assert L.fsn_fast_stream_step(*args(nbytes, ws.numel() - 1)) == -2
    torch.cuda.synchronize()
    assert not blob.any() and not crm.any()  # nothing was launched
    offline = model_of(R.SHIPPED, "offline_laplace_norm")
    assert L.fsn_fast_stream_state_bytes(ctypes.byref(offline.stream_cfg()), 1) == 0 and b"causal norm" in L.fsn_last_error()
    from fullsubnet_amd.streaming import StreamingEnhancer
    with pytest.raises(ValueError, match="streaming needs a causal norm"):
        StreamingEnhancer(offline)


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
    return torch.cat(out, dim=1), lat


def odd_sizes(L, seed):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < L:
        sizes.append(int(min(2 * rng.integers(0, 450) + 1, L - sum(sizes))))
    return sizes


@pytest.mark.parametrize("cfg", [R.SHIPPED, R.Cfg(shrink=3, la=1, n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1), R.Cfg(shrink=1, la=0)], ids=str)
def test_streaming_enhancer_equals_the_whole_utterance(fsn, cfg):
    """StreamingEnhancer(fast_model) over odd chunk lengths + flush = model.enhance(noisy) of the whole utterance to 1e-4 of its
    peak (the bound tests/test_gpu_streaming.py holds FullSubNet's composed stream to); two chunkings bit for bit; no sample
    leaves later than (look_ahead + 2) hops after it came in."""
    model = model_of(cfg)
    L = 5003
    noisy = torch.from_numpy(O.make_noisy(2, L, seed=17)).cuda()
    a, lat_a = run_stream(model, noisy, odd_sizes(L, 3))
    b, lat_b = run_stream(model, noisy, [256] * (L // 256) + [L % 256])
    assert a.shape == noisy.shape and torch.isfinite(a).all()
    offline = model.enhance(noisy)
    scale = offline.abs().max().item()
    err = (a - offline).abs().max().item()
    print(f"[fsweep] {cfg}: stream against the whole utterance {err:.3e}, peak {scale:.3e} ({err / scale:.2e} of it)")
    assert scale > 0 and err <= 1e-4 * scale
    assert torch.equal(a, b)
    assert max(lat_a + lat_b) <= (cfg.la + 2) * 256
    from fullsubnet_amd.streaming import StreamingEnhancer
    enh = StreamingEnhancer(model, batch_size=2)
    enh.process(noisy[:, :3000])
    enh.reset()
    assert torch.equal(torch.cat([enh.process(noisy), enh.flush()], dim=1), a)
