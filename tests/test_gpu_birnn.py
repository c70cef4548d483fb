"""The bidirectional layer entries (fsn_lstm_bilayer_* / fsn_gru_bilayer_*) and SequenceModel(bidirectional=True) on an MI355X:
python -m pytest tests/test_gpu_birnn.py -m gpu -s

Entry level, through fullsubnet_amd._lib directly, every row of ROWS:
1. forward (inference and with saves) and backward against the fp64 reference of tests/birnn_reference.py by the rule of
   tests/test_gpu_recurrent_sweep.py, unchanged: both statistics, for the whole tensor, per step, per 16-row tile and per gate
   block, at most SHARP = 4 x those of the CPU fp32 run yardstick_of chooses;
2. slot symmetry as equality: (wr, wf) on x.flip(0) gives the halves swapped and frame-reversed, bit for bit, and the swapped
   weight gradients;
3. memory discipline: NaN-sentinel outputs with a 1024-element guard, ldh = 2H and 2H + 16 the same bits with the extra columns
   untouched, workspaces exactly the queries' sizes and 0xFF-filled, two calls bit-identical, dx == NULL the same weight
   gradients, zero-padded units exactly 0.0 in both halves and in their gradient rows;
4. launch counts: fsn_debug_bilayer_last_step_launches() == T after a forward call, <= T after a backward call.

Module level: SequenceModel(257, 2, H, layers, True, cell) on [3, 257, 9] - inference output and every parameter's gradient by the
same rule, the yardstick being torch's own CPU fp32 nn.LSTM / nn.GRU(bidirectional=True) + Linear; pooled over DRAWS inputs (the
output has 54 elements, the fc bias 2: one draw is no statistic).  A unidirectional block beside it gives the bits of the
untouched layer entries.

Seen on an MI355X: 27 tests, 5.8 s.  Worst ratio to the yardstick over all rows and outputs: relative Frobenius error 2.26 x (y of
bilstm-T1-N16-I20-H64, held to the cell emulation), max error 2.55 x (dx of bilstm-T9-N32-I768-H384); every slot-symmetry
equality held.  With dX formed as ONE product over the concatenated gate gradients (K = 2 g H) the max error of dx stood at 4.58 x
on bigru-T9-N80-I257-H512 (3.12 x on bilstm-T9-N80-I257-H384): it is formed per direction and added, 1.66 x / 1.59 x.
"""
import pytest
import torch
import torch.nn as nn

import birnn_reference as R
import test_gpu_recurrent_sweep as S

pytestmark = pytest.mark.gpu

ROWS = [R.BiRow(c, T, 16, 20, 64) for c in ("lstm", "gru") for T in (1, 2, 9)] + \
       [R.BiRow(c, 8, 48, 33, 128) for c in ("lstm", "gru")] + \
       [R.BiRow("lstm", 9, 80, 257, 384), R.BiRow("gru", 9, 80, 257, 512)] + \
       [R.BiRow(c, 9, 32, 768, 384) for c in ("lstm", "gru")] + \
       [R.BiRow(c, 9, 16, 20, 64, gain=6.0) for c in ("lstm", "gru")] + \
       [R.BiRow(c, 9, 32, 33, 384, Hreal=320) for c in ("lstm", "gru")]


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return fullsubnet_amd


class Device:
    """A row's entries on device operands: outputs behind sentinels, workspaces and save buffers exact and poisoned."""

    def __init__(self, fsn, row, ops):
        self.lib, self.L, self.row = fsn._lib, fsn._lib.lib(), row
        self.dev = torch.device("cuda:0")
        self.st = self.lib.stream_ptr(self.dev)
        c = row.cell
        self.q = {n: getattr(self.L, f"fsn_{c}_bilayer_{n}") for n in ("save_bytes", "fwd_workspace_bytes", "forward",
                                                                        "bwd_workspace_bytes", "backward")}
        self.set(ops["x"], ops["dy"], ops["wf"], ops["wr"])

    def set(self, x, dy, wf, wr):
        self.x, self.dy = x.to(self.dev), dy.to(self.dev)
        self.w = [torch.stack((a, b)).to(self.dev).contiguous() for a, b in zip(wf, wr)]  # [2][gH][.] each

    def ws(self, nbytes):
        return self.lib.workspace(nbytes, self.dev).fill_(0xFF)

    def run(self, ldx, ldh, lddx, want_dx=True):
        r, p, ck, q = self.row, self.lib.dev_ptr, self.lib.check, self.q
        T, N, I, H, G = r.T, r.n, r.I, r.H, r.G * r.H
        x = S._padded(self.x, ldx)
        wp = [p(t) for t in self.w]
        out = {}
        # inference
        ws, y0 = self.ws(q["fwd_workspace_bytes"](T, N, I, H)), S.Out(self.dev, (T, N, 2 * H), ldh)
        ck(q["forward"](p(x), ldx, *wp, T, N, I, H, p(y0.f), ldh, None, 0, ws.data_ptr(), ws.numel(), self.st))
        assert self.L.fsn_debug_bilayer_last_step_launches() == T
        out["y_infer"] = y0.take("hseq (inference)")
        # forward with saves + BPTT
        save = self.ws(q["save_bytes"](T, N, H))
        ws, y = self.ws(q["fwd_workspace_bytes"](T, N, I, H)), S.Out(self.dev, (T, N, 2 * H), ldh)
        ck(q["forward"](p(x), ldx, *wp, T, N, I, H, p(y.f), ldh, save.data_ptr(), save.numel(), ws.data_ptr(), ws.numel(), self.st))
        assert self.L.fsn_debug_bilayer_last_step_launches() == T
        out["y"] = y.take("hseq")
        dh = S._padded(self.dy, ldh)
        ws = self.ws(q["bwd_workspace_bytes"](T, N, I, H))
        dx = S.Out(self.dev, (T, N, I), lddx) if want_dx else None
        dwi, dwh = S.Out(self.dev, (2, G, I)), S.Out(self.dev, (2, G, H))
        dbs = [S.Out(self.dev, (2, G)) for _ in range(1 if r.cell == "lstm" else 2)]
        ck(q["backward"](p(dh), ldh, p(x), ldx, wp[0], wp[1], T, N, I, H, p(y.f[:T * N * ldh]), ldh, save.data_ptr(),
                         p(dx.f) if want_dx else None, lddx, p(dwi.f), p(dwh.f), *[p(b.f) for b in dbs], ws.data_ptr(), ws.numel(),
                         self.st))
        assert 1 <= self.L.fsn_debug_bilayer_last_step_launches() <= T
        if want_dx:
            out["dx"] = dx.take("dx")
        got = dict(dw_ih=dwi.take("dw_ih"), dw_hh=dwh.take("dw_hh"))
        for n, b in zip(R.grad_names(r.cell)[2:], dbs):
            got[n] = b.take(n)
        for n, v in got.items():
            out[n + "_f"], out[n + "_r"] = v[0].contiguous(), v[1].contiguous()
        self.lib.check_canaries()
        return out


def _same(a, b, what, skip=()):
    for k in a:
        if k in b and k not in skip:
            assert torch.equal(a[k], b[k]), f"{k}: {what}: not bit-identical"


def run_draw(fsn, row, draw, stats, first):
    ops = R.make_operands(row, draw)
    d = Device(fsn, row, ops)
    H, ldx, lddx = row.H, S.ru16(row.I), S.ru16(row.I) + 4
    got = d.run(ldx, 2 * H, lddx)
    assert torch.equal(got["y_infer"], got["y"]), "inference and the forward with saves give different hidden sequences"
    if first:
        _same(d.run(ldx, 2 * H, lddx), got, "two calls in a row")
        _same(d.run(ldx + 16, 2 * H + 16, row.I), got, "another ldx / ldh / lddx")
        _same(d.run(ldx, 2 * H, lddx, want_dx=False), got, "dx == NULL")
        # slot symmetry: the directions swapped on the frame-reversed problem
        d.set(ops["x"].flip(0), torch.cat((ops["dy"][..., H:], ops["dy"][..., :H]), -1).flip(0), ops["wr"], ops["wf"])
        sw = d.run(ldx, 2 * H, lddx)
        for k in ("y", "y_infer"):
            assert torch.equal(sw[k][..., :H], got[k][..., H:].flip(0)), f"{k}: the reverse direction in the forward slot differs"
            assert torch.equal(sw[k][..., H:], got[k][..., :H].flip(0)), f"{k}: the forward direction in the reverse slot differs"
        for n in R.grad_names(row.cell):
            assert torch.equal(sw[n + "_f"], got[n + "_r"]), f"{n}: the reverse direction's gradient depends on its slot"
            assert torch.equal(sw[n + "_r"], got[n + "_f"]), f"{n}: the forward direction's gradient depends on its slot"
    assert fsn._lib.stream_status(d.dev) == (0, 0), "the stream carries a timeout record"
    host = {k: v.cpu() for k, v in got.items() if k != "y_infer"}
    if row.Hreal < H:  # zero-padded units: exactly zero in both halves and in their gradient rows / columns
        y = host["y"].view(row.T, row.n, 2, H)
        assert bool((y[..., row.Hreal:] == 0).all()), "y: zero-padded units are not exactly 0.0"
        for k, v in host.items():
            if k[0] == "d" and k != "dx":
                assert bool((v.view(row.G, H, -1)[:, row.Hreal:] == 0).all()), f"{k}: gradient rows of zero-padded units are not exactly 0.0"
            if k.startswith("dw_hh"):
                assert bool((v[:, row.Hreal:] == 0).all()), f"{k}: gradient columns of zero-padded units are not exactly 0.0"
    if row.cell == "gru":
        for sfx in ("_f", "_r"):
            assert torch.equal(host["db_ih" + sfx][:2 * H], host["db_hh" + sfx][:2 * H]), "db_ih / db_hh differ outside the n block"
    del d
    R.check(row, stats, ops, host)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_bilayer_entries(fsn, row):
    stats = {}
    for draw in range(row.draws()):
        run_draw(fsn, row, draw, stats, draw == 0)
    R.assert_stats(row, stats)


def test_bilayer_refuses_bad_strides_on_the_device(fsn):
    """ldh < 2H is refused with nothing written."""
    row = ROWS[0]
    d = Device(fsn, row, R.make_operands(row, 0))
    T, N, I, H = row.T, row.n, row.I, row.H
    y = S.Out(d.dev, (T, N, 2 * H))
    ws = d.ws(d.q["fwd_workspace_bytes"](T, N, I, H))
    p = d.lib.dev_ptr
    rc = d.q["forward"](p(S._padded(d.x, 32)), 32, *[p(t) for t in d.w], T, N, I, H, p(y.f), 2 * H - 4, None, 0, ws.data_ptr(), ws.numel(), d.st)
    assert rc == -1 and b"row stride" in d.L.fsn_last_error()
    assert bool((y.buf == S.SENTINEL).all())


# ---- module level -----------------------------------------------------------------------------------------------------------
DRAWS = 6
B, F, T = 3, 257, 9


class _TorchBlock(nn.Module):
    def __init__(self, cell, H, layers, bidirectional=True):
        super().__init__()
        self.sequence_model = (nn.LSTM if cell == "LSTM" else nn.GRU)(input_size=F, hidden_size=H, num_layers=layers, batch_first=True,
                                                                    bidirectional=bidirectional)
        self.fc_output_layer = nn.Linear(2 * H if bidirectional else H, 2)

    def forward(self, x):  # [B, F, T] -> [B, O, T], as the reference's block with its default Tanh
        return torch.tanh(self.fc_output_layer(self.sequence_model(x.permute(0, 2, 1))[0])).permute(0, 2, 1)


@pytest.mark.parametrize("layers", (1, 2))
@pytest.mark.parametrize("H", (64, 320))
@pytest.mark.parametrize("cell", ("LSTM", "GRU"))
def test_bidirectional_sequence_model(fsn, cell, H, layers):
    from fullsubnet_amd.sequence_model import SequenceModel
    dev = torch.device("cuda:0")
    row = R.ModuleRow(cell.lower(), T, F)
    infer, train = {}, {}
    for draw in range(DRAWS):
        torch.manual_seed(100 * draw + layers)
        ref = _TorchBlock(cell, H, layers)
        sd = ref.state_dict()
        m = SequenceModel(F, 2, H, layers, True, cell)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev)
        x, dy = torch.randn(B, F, T), torch.randn(B, 2, T)
        want, want_g = R.module_reference(cell.lower(), sd, x, layers, dy)
        # inference
        with torch.no_grad():
            got = m.eval()(x.to(dev)).cpu()
            cpu = ref(x)
        assert got.shape == (B, 2, T)
        infer.setdefault("y", S.Stat("y")).add(row, got, cpu, want)
        # one training step's gradients, every parameter
        m.train()
        out = m(x.to(dev))
        (out * dy.to(dev)).sum().backward()
        (ref(x) * dy).sum().backward()
        train.setdefault("y", S.Stat("y")).add(row, out.detach().cpu(), cpu, want)
        cpu_g = dict(ref.named_parameters())
        names = [n for n, _ in m.named_parameters()]
        assert names == list(cpu_g) and any(n.endswith("_reverse") for n in names)
        for n, prm in m.named_parameters():
            assert prm.grad is not None and prm.grad.shape == want_g[n].shape, n
            k = R.grad_key(n)
            train.setdefault(k, S.Stat(k)).add(row, prm.grad.cpu(), cpu_g[n].grad, want_g[n])
    R.assert_stats(_Named(row, f"bi{cell}-H{H}-L{layers} inference"), infer)
    R.assert_stats(_Named(row, f"bi{cell}-H{H}-L{layers} training"), train)


class _Named:
    def __init__(self, row, name):
        self.cell, self.T, self.I, self.id = row.cell, row.T, row.I, name


@pytest.mark.parametrize("cell", ("LSTM", "GRU"))
def test_unidirectional_block_beside_it_keeps_its_bits(fsn, cell):
    """The unidirectional block's inference output is, bit for bit, the untouched layer entries composed by hand: one layer
    through lstm_layer_infer / gru_layer_infer, two LSTM layers through lstm2_infer (the module's few-row plan)."""
    from fullsubnet_amd import sequence_model as M
    dev = torch.device("cuda:0")
    for H, layers in ((64, 1), (320, 1), (64, 2)):
        torch.manual_seed(7 + layers)
        m = M.SequenceModel(F, 2, H, layers, False, cell).to(dev).eval()
        x = torch.randn(B, F, T, device=dev)
        Hp = (H + 63) // 64 * 64
        with torch.no_grad():
            got = m(x)
            h = M.to_rows(x)
            ws = [tuple(t.contiguous() for t in M.pad_lstm_weights(*m._layer_tensors(k), F if k == 0 else Hp)) for k in range(layers)]
            if cell == "LSTM" and layers == 2:
                h = M.lstm2_infer(h, ws[0], ws[1])
            else:
                for w in ws:
                    h = (M.lstm_layer_infer if cell == "LSTM" else M.gru_layer_infer)(h, *w)
            fw = torch.zeros((2, Hp), device=dev)
            fw[:, :H] = m.fc_output_layer.weight
            o = M.linear_infer(h.reshape(-1, Hp), fw, m.fc_output_layer.bias.contiguous(), False).reshape(T, -1, 2)
            want = M.from_rows(torch.tanh(o), B)
        assert torch.equal(got, want), f"{cell} H {H} layers {layers}: the unidirectional block changed its bits"
