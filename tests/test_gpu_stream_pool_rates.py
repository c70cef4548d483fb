"""The streaming pool at other sample rates (StreamPool(input_sr=, output_sr=)): what reaches the model is, bit
for bit, the offline resampling of the session's input, what leaves is the offline resampling of the model's output, and
the model in between keeps the pool's existing bound.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu

MODEL_KW = dict(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                sb_model_hidden_size=384, weight_init=False)
LEN48 = {"A": 15009, "B": 9000, "C": 2100}  # 5003, 3000 and 700 samples at the model's rate
SR = 16000


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd as fsn
    fsn._lib.lib()
    params = O.make_params(seed=0, gain=2.0, mask_gain=24.0)
    m = fsn.Model(norm_type="cumulative_laplace_norm", num_groups_in_drop_band=1, **MODEL_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.cuda().eval()
    inf = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}),
                              acoustics=dict(n_fft=512, hop_length=256, win_length=512, sr=SR)), model=m)
    return fsn, m, inf


def utterance(n, seed):
    return torch.from_numpy(O.make_noisy(1, n, seed=seed)[0]).cuda()


def chunks_of(name):
    L = LEN48[name]
    if name == "A":
        return [768] * (L // 768) + [L % 768]  # a tick's worth each
    if name == "B":
        rng = np.random.default_rng(3)
        sizes = []
        while sum(sizes) < L:
            sizes.append(int(min(rng.integers(1, 2700), L - sum(sizes))))
        return sizes
    return [300, 3, 465, 3, 1329]


class Feeder:
    def __init__(self, pool, y, sizes):
        self.pool, self.y, self.sizes, self.pos = pool, y, list(sizes), 0
        self.sid = pool.open()
        self.out = []

    def push(self):
        n = self.sizes.pop(0)
        self.pool.push(self.sid, self.y[self.pos:self.pos + n])
        self.pos += n

    def close(self):
        assert not self.sizes and self.pos == self.y.numel()
        self.out.append(self.pool.close(self.sid))
        return torch.cat(self.out)


def drain(pool, feeders):
    got = pool.drain()
    for f in feeders:
        if f.sid in got:
            f.out.append(got[f.sid])


@pytest.fixture(scope="module")
def schedule(setup):
    """A opens; B opens after A has pushed 4500 samples and pushes every third round; A closes while B is mid-stream; C
    opens afterwards, into A's freed slot, and runs beside the rest of B.  48 kHz in and out."""
    fsn, model, _ = setup
    utts = {name: utterance(L, 40 + i) for i, (name, L) in enumerate(LEN48.items())}
    pool = fsn.StreamPool(model, capacity=4, input_sr=48000, output_sr="input", record_model_rate=True)
    res, rec = {}, {}
    a = Feeder(pool, utts["A"], chunks_of("A"))
    while a.pos < 4500:
        a.push()
        drain(pool, [a])
    b = Feeder(pool, utts["B"], chunks_of("B"))
    assert (pool.slot(a.sid), pool.slot(b.sid)) == (0, 1)
    r = 0
    while a.sizes:
        a.push()
        if r % 3 == 0:
            b.push()
        d0, u0 = pool._down.calls, pool._up.calls
        out = pool.step()  # both sessions' input in one conversion, both outputs in one
        assert pool._down.calls - d0 == 1 and pool._up.calls - u0 == (1 if out else 0)
        for f in (a, b):
            if f.sid in out:
                f.out.append(out[f.sid])
        drain(pool, [a, b])
        r += 1
    assert 0 < b.pos < LEN48["B"] and b.sizes
    res["A"] = a.close()
    c = Feeder(pool, utts["C"], chunks_of("C"))
    assert pool.slot(c.sid) == 0
    while c.sizes or b.sizes:
        if c.sizes:
            c.push()
        if b.sizes:
            b.push()
        drain(pool, [b, c])
    res["C"] = c.close()
    res["B"] = b.close()
    assert not pool.book.sids() and not pool._down.book.sids() and not pool._up.book.sids()
    for name, f in (("A", a), ("B", b), ("C", c)):
        rec[name] = pool.recorded(f.sid)
    return utts, res, rec


def up_gain(fsn, sr_out, design="scipy"):
    """G = max over phases of sum_j |poly[p][j]|: the up filter's worst-case gain on a difference at the model's rate."""
    h = fsn.resample.taps(SR, sr_out, design).abs().cpu().numpy()
    u = fsn.resample.ratio(SR, sr_out)[0]
    return max(h[p::u].sum() for p in range(u))


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_48k_in_and_out(setup, schedule, name):
    fsn, model, inf = setup
    utts, res, rec = schedule
    x, got = utts[name], res[name]
    model_in, model_out = rec[name]
    rs = fsn.resample
    # (a) what the model received is the offline conversion of the whole utterance
    want_in = rs.resample(x, 48000, SR)[0]
    assert want_in.numel() == rs.out_length(x.numel(), 48000, SR)
    assert torch.equal(model_in, want_in)
    # (b) what came back is the offline conversion of what the model gave, cut to the input's length
    assert model_out.numel() == model_in.numel()
    assert got.numel() == x.numel()
    assert torch.equal(got, rs.resample(model_out, SR, 48000)[0][:x.numel()])
    # (c) in between, the pool's existing bound at the rate where it was established
    offline16 = model.enhance(model_in[None])[0]
    scale = offline16.abs().max().item()
    d = (model_out - offline16).abs().max().item()
    print(f"{name}: max|pool - offline| at 16 kHz = {d:.3e} of {scale:.3e}")
    assert d <= 2e-3 * scale
    # (d) end to end
    G = up_gain(fsn, 48000)
    offline48 = inf.enhance_utterances([x], sr=48000, output_sr="input")[0]
    assert offline48.shape == got.shape
    e = (got - offline48).abs().max().item()
    print(f"{name}: max|pool - Inferencer| at 48 kHz = {e:.3e}, bound G 2e-3 max|offline| = {G:.3f} * {2e-3 * scale:.3e}")
    assert 2.0 < G < 2.2
    assert e <= G * 2e-3 * scale


def test_44k1_in_and_out(setup):
    fsn, model, _ = setup
    rs = fsn.resample
    x = utterance(13807, 50)
    rng = np.random.default_rng(8)
    pool = fsn.StreamPool(model, capacity=2, input_sr=44100, output_sr="input", record_model_rate=True)
    f = Feeder(pool, x, [])
    while sum(f.sizes) < x.numel():
        f.sizes.append(int(min(rng.integers(0, 2000), x.numel() - sum(f.sizes))))
    while f.sizes:
        f.push()
        drain(pool, [f])
    got = f.close()
    model_in, model_out = pool.recorded(f.sid)
    assert torch.equal(model_in, rs.resample(x, 44100, SR)[0])
    assert got.numel() == x.numel() == 13807
    assert torch.equal(got, rs.resample(model_out, SR, 44100)[0][:x.numel()])
    assert 2.1 < up_gain(fsn, 44100) < 2.4


def test_model_rate_out_equals_the_plain_pool(setup):
    """48 kHz in, the model's rate out: the samples are those of a pool without resamplers that is fed the converted
    input under the same push and drain schedule (a session alone runs every tick with n = 1, so a repeat has the same
    bits - shown first)."""
    fsn, model, _ = setup
    x = utterance(7000, 60)
    sizes = [768] * 5 + [1, 0, 2000] + [7000 - 768 * 5 - 2001]

    def rated():
        pool = fsn.StreamPool(model, capacity=2, input_sr=48000, record_model_rate=True)
        assert pool._up is None and pool._down is not None
        sid, pos, outs, fed = pool.open(), 0, [], []
        for c in sizes:
            pool.push(sid, x[pos:pos + c])
            pos += c
            got = pool.drain()
            outs.append(got.get(sid, x[:0]))
            fed.append(pool.recorded(sid)[0].numel())
        outs.append(pool.close(sid))
        return outs, fed, pool.recorded(sid)

    outs, fed, (model_in, model_out) = rated()
    again = rated()[0]
    assert all(torch.equal(p, q) for p, q in zip(outs, again))
    assert torch.equal(torch.cat(outs), model_out) and model_out.numel() == model_in.numel() == 2334
    plain = fsn.StreamPool(model, capacity=2)
    sid, pos = plain.open(), 0
    for n, want in zip(fed, outs):
        plain.push(sid, model_in[pos:n])
        pos = n
        got = plain.drain().get(sid, x[:0])
        assert torch.equal(got, want)
    plain.push(sid, model_in[pos:])  # what the end of the input released
    assert torch.equal(plain.close(sid), outs[-1])


def test_default_pool_has_no_resampler(setup):
    fsn, model, _ = setup
    for pool in (fsn.StreamPool(model, capacity=2), fsn.StreamPool(model, capacity=2, input_sr=SR, output_sr="model"),
                 fsn.StreamPool(model, capacity=2, input_sr=SR, output_sr="input"), fsn.StreamPool(model, capacity=2, output_sr=SR)):
        assert pool._down is None and pool._up is None and not pool._rate and not pool.record_model_rate
        sid = pool.open()
        pool.push(sid, utterance(1000, 1))
        pool.drain()
        pool.close(sid)
        assert not pool._rate and not pool._recorded
    up_only = fsn.StreamPool(model, capacity=2, output_sr=48000)
    assert up_only._down is None and up_only._up is not None
    sid = up_only.open()
    up_only.push(sid, utterance(1000, 1))
    parts = [up_only.drain().get(sid)]
    parts.append(up_only.close(sid))
    assert sum(p.numel() for p in parts if p is not None) == 3000
    # a session too short after conversion: the existing refusal, and the session is still there
    pool = fsn.StreamPool(model, capacity=2, input_sr=48000, output_sr="input")
    sid = pool.open()
    pool.push(sid, torch.zeros(768))  # 256 samples at the model's rate
    assert pool.step() == {}
    with pytest.raises(fsn._lib.FsnError, match="shorter"):
        pool.close(sid)
    pool.push(sid, torch.zeros(3))    # 257
    assert pool.close(sid).numel() == 771
    for bad in (dict(input_sr=0), dict(input_sr=16000.0), dict(output_sr="source"), dict(output_sr=-1)):
        with pytest.raises(ValueError):
            fsn.StreamPool(model, capacity=2, **bad)
