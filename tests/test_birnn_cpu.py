"""CPU-side checks of the bidirectional SequenceModel: the reference of tests/birnn_reference.py against torch's own bidirectional
rnn, the module's parameter surface, the bilayer entries' size queries and refusals, the padding re-layout, and the checker of
tests/test_gpu_birnn.py tried on torch's fp32 and on deliberately wrong stand-ins."""
import ctypes

import pytest
import torch
import torch.nn as nn

import birnn_reference as R
from fullsubnet_amd import _lib
from fullsubnet_amd.sequence_model import (SequenceModel, multi_forward, multi_plan, pad_lstm_weights, pair_forward_rows,
                                           pair_fusable)

CELLS = ("LSTM", "GRU")


def _torch_layers(rnn, num_layers, dtype=None):
    cast = (lambda t: t.detach()) if dtype is None else (lambda t: t.detach().to(dtype))
    return [tuple([cast(getattr(rnn, f"{n}_l{k}{sfx}")) for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                  for sfx in ("", "_reverse")) for k in range(num_layers)]


@pytest.mark.parametrize("cell", CELLS)
def test_reference_is_torchs_bidirectional_rnn_in_fp64(cell):
    """T 9, N 5, I 20, H 64, two layers: the flipped-and-concatenated recurrences against nn.LSTM / nn.GRU(bidirectional=True)."""
    torch.manual_seed(3)
    rnn = (nn.LSTM if cell == "LSTM" else nn.GRU)(20, 64, num_layers=2, bidirectional=True).double()
    x = torch.randn(9, 5, 20, dtype=torch.float64)
    with torch.no_grad():
        want = rnn(x)[0]
        got = R.stack(cell.lower(), x, _torch_layers(rnn, 2))
    assert got.shape == want.shape == (9, 5, 128)
    assert float((got - want).abs().max()) <= 1e-12


class _TorchBlock(nn.Module):
    """What the reference's block holds for bidirectional=True: torch's bidirectional rnn and Linear(2H, O)."""

    def __init__(self, cell, I, O, H, layers):
        super().__init__()
        self.sequence_model = (nn.LSTM if cell == "LSTM" else nn.GRU)(input_size=I, hidden_size=H, num_layers=layers, batch_first=True,
                                                                    bidirectional=True)
        self.fc_output_layer = nn.Linear(2 * H, O)


@pytest.mark.parametrize("cell", CELLS)
def test_bidirectional_block_constructs_with_torchs_parameter_surface(cell):
    m = SequenceModel(257, 2, 64, 2, True, cell)
    ref = _TorchBlock(cell, 257, 2, 64, 2)
    have, want = m.state_dict(), ref.state_dict()
    assert list(have) == list(want)  # names AND order
    assert [tuple(v.shape) for v in have.values()] == [tuple(v.shape) for v in want.values()]
    assert any(k.endswith("_reverse") for k in have) and have["fc_output_layer.weight"].shape == (2, 128)
    m.load_state_dict(want, strict=True)
    for k, v in want.items():
        assert torch.equal(m.state_dict()[k], v)
    uni = SequenceModel(64, 2, 64, 1, False, "LSTM")
    assert pair_fusable(SequenceModel(257, 0, 64, 1, False, "LSTM", None), uni, 3)  # the unidirectional pair still fuses
    one = SequenceModel(257, 0, 64, 1, True, cell, None)
    assert not pair_fusable(one, uni, 3) and not pair_fusable(m, m, 3)
    assert multi_plan([m], [(3, 257, 9)]) is False
    with pytest.raises(_lib.FsnError):
        pair_forward_rows(one, uni, torch.zeros(9, 16, 272))
    with pytest.raises(_lib.FsnError):
        multi_forward([m], prepared=[(torch.zeros(9, 16, 272), 3)])


def test_unidirectional_block_is_what_it_was():
    m = SequenceModel(257, 2, 64, 2, False, "LSTM")
    assert not m.bidirectional and not any(k.endswith("_reverse") for k in m.state_dict())
    assert m.fc_output_layer.weight.shape == (2, 64)


ENTRIES = ("save_bytes", "fwd_workspace_bytes", "forward", "bwd_workspace_bytes", "backward")


def test_bilayer_size_queries_and_refusals_without_a_gpu():
    L = _lib.lib()
    T, N, I, H = 9, 32, 20, 64
    for cell, g in (("lstm", 4), ("gru", 3)):
        q = {n: getattr(L, f"fsn_{cell}_bilayer_{n}") for n in ENTRIES}
        per_dir = T * N * (5 if g == 4 else 4) * H * 4
        assert q["save_bytes"](T, N, H) >= 2 * per_dir
        assert q["fwd_workspace_bytes"](T, N, I, H) >= T * N * 2 * g * H * 4       # the projection of both directions at least
        assert q["bwd_workspace_bytes"](T, N, I, H) >= T * N * 2 * g * H * 4       # ... and their gate gradients
        assert q["fwd_workspace_bytes"](T, N, 2 * H, H) > q["fwd_workspace_bytes"](T, N, I, H)
        for bad in ((T, 24, H), (T, N, 96), (0, N, H), (T, 0, H)):
            assert q["save_bytes"](*bad) == 0
            assert q["fwd_workspace_bytes"](bad[0], bad[1], I, bad[2]) == 0
            assert q["bwd_workspace_bytes"](bad[0], bad[1], I, bad[2]) == 0
        # the entries refuse before they touch anything: dummy (never dereferenced) pointers
        p = ctypes.c_void_p(4096)
        fwd = lambda T_, N_, H_, ldh: q["forward"](p, 32, p, p, p, p, T_, N_, I, H_, p, ldh, None, 0, p, 1 << 40, None)
        nb = 1 if g == 4 else 2
        bwd = lambda T_, N_, H_, ldh, lddh: q["backward"](p, lddh, p, 32, p, p, T_, N_, I, H_, p, ldh, p, None, 32, p, p, *([p] * nb), p,
                                                          1 << 40, None)
        for call, word in ((lambda: fwd(T, 24, H, 2 * H), b"multiple of 16"), (lambda: fwd(T, N, 96, 192), b"multiple of 64"),
                           (lambda: fwd(T, N, H, 2 * H - 4), b"row stride"), (lambda: fwd(0, N, H, 2 * H), b"T >= 1"),
                           (lambda: bwd(T, 24, H, 2 * H, 2 * H), b"multiple of 16"), (lambda: bwd(T, N, 96, 192, 192), b"multiple of 64"),
                           (lambda: bwd(T, N, H, 2 * H - 4, 2 * H), b"row stride"), (lambda: bwd(T, N, H, 2 * H, H), b"row stride"),
                           (lambda: bwd(0, N, H, 2 * H, 2 * H), b"T >= 1")):
            assert call() == -1, "FSN_ERR_ARG expected"
            assert word in L.fsn_last_error(), L.fsn_last_error()
    assert L.fsn_debug_bilayer_last_step_launches() == 0  # a refused call launched nothing


@pytest.mark.parametrize("cell,g", (("LSTM", 4), ("GRU", 3)))
def test_padding_relayout_of_a_layer_above_a_bidirectional_one(cell, g):
    """H = 20 -> Hp = 64: the second layer's W_ih [g 20][40] becomes [g 64][128] with input columns [0, 20) at [0, 20) and
    [20, 40) at [64, 84); nothing else is filled.  The padded and the unpadded CPU recurrences give the same fp32 values, and
    the padded units are exactly zero."""
    torch.manual_seed(5)
    H, Hp = 20, 64
    rnn = (nn.LSTM if cell == "LSTM" else nn.GRU)(33, H, num_layers=2, bidirectional=True)
    layers = _torch_layers(rnn, 2)
    w_ih = layers[1][0][0]
    wi, wh, bi, bh = pad_lstm_weights(*layers[1][0], 2 * Hp, in_halves=H)
    assert wi.shape == (g * Hp, 2 * Hp) and wh.shape == (g * Hp, Hp) and bi.shape == bh.shape == (g * Hp,)
    w3 = wi.view(g, Hp, 2 * Hp)
    assert torch.equal(w3[:, :H, :H], w_ih.view(g, H, 2 * H)[:, :, :H])
    assert torch.equal(w3[:, :H, Hp:Hp + H], w_ih.view(g, H, 2 * H)[:, :, H:])
    filled = torch.zeros_like(w3, dtype=torch.bool)
    filled[:, :H, :H] = True
    filled[:, :H, Hp:Hp + H] = True
    assert bool((w3[~filled] == 0).all())
    assert int((w3 != 0).sum()) == int((w_ih != 0).sum())
    with pytest.raises(_lib.FsnError):
        pad_lstm_weights(*layers[1][0], 2 * Hp, in_halves=H + 1)
    # gradients reach the unpadded parameter through the re-layout
    w = w_ih.clone().requires_grad_(True)
    pad_lstm_weights(w, *layers[1][0][1:], 2 * Hp, in_halves=H)[0].sum().backward()
    assert torch.equal(w.grad, torch.ones_like(w))
    # the whole block: padded against unpadded, exactly (zero units keep h = c = 0; zero products add nothing)
    m = SequenceModel(33, 0, H, 2, True, cell, None)
    m.sequence_model.load_state_dict(rnn.state_dict())
    # (both recurrences in fp64 and compared as fp32 values: the CPU's matrix product groups a K = 40 sum and the same terms
    # inside a K = 128 sum differently, which moves an fp64 result by ~1e-16 and an fp32 one by a whole ULP)
    x = torch.randn(7, 5, 33, dtype=torch.float64)
    dbl = lambda ws: tuple(t.double() for t in ws)
    with torch.no_grad():
        plain = R.stack(cell.lower(), x, [tuple(dbl(w) for w in lp) for lp in layers]).float()
        padded = R.stack(cell.lower(), x, [tuple(dbl(t[d] for t in m._bi_layer_tensors(k)) for d in (0, 1)) for k in (0, 1)]).float()
    assert padded.shape == (7, 5, 2 * Hp)
    assert torch.equal(padded[..., :H], plain[..., :H]) and torch.equal(padded[..., Hp:Hp + H], plain[..., H:])
    assert bool((padded[..., H:Hp] == 0).all()) and bool((padded[..., Hp + H:] == 0).all())


# ---- the checker on stand-ins ---------------------------------------------------------------------------------------------
ROWS = [R.BiRow("lstm", 9, 16, 257, 64), R.BiRow("gru", 9, 16, 257, 64), R.BiRow("lstm", 9, 16, 20, 64), R.BiRow("gru", 2, 16, 20, 64)]


def _verdict(row, ops, outs):
    stats = {}
    R.check(row, stats, ops, outs)
    R.assert_stats(row, stats, log=lambda s: None)


def _flagged(row, ops, outs, what):
    with pytest.raises(AssertionError):
        _verdict(row, ops, outs)
        pytest.fail(f"{row.id}: '{what}' passed the checker", pytrace=False)


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_checker_passes_torch_fp32_and_flags_wrong_stand_ins(row):
    ops = R.make_operands(row, 0)
    H, cell = row.H, row.cell
    # torch's own CPU fp32 bidirectional rnn as the "device"
    rnn = (nn.LSTM if cell == "lstm" else nn.GRU)(row.I, H, bidirectional=True)
    with torch.no_grad():
        for sfx, w in (("", ops["wf"]), ("_reverse", ops["wr"])):
            for n, t in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), w):
                getattr(rnn, f"{n}_l0{sfx}").copy_(t)
    x = ops["x"].clone().requires_grad_(True)
    y = rnn(x)[0]
    names = [f"{n}_l0{sfx}" for sfx in ("", "_reverse") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    grads = torch.autograd.grad((y * ops["dy"]).sum(), [x] + [getattr(rnn, n) for n in names])
    good = {"y": y.detach(), "dx": grads[0]}
    for d, sfx in enumerate(("_f", "_r")):
        gw = grads[1 + 4 * d:5 + 4 * d]
        good["dw_ih" + sfx], good["dw_hh" + sfx] = gw[0], gw[1]
        if cell == "lstm":
            good["db" + sfx] = gw[2]  # torch keeps two equal bias gradients
        else:
            good["db_ih" + sfx], good["db_hh" + sfx] = gw[2], gw[3]
    _verdict(row, ops, good)

    def with_y(y2):
        return dict(good, y=y2)
    yf, yr = good["y"][..., :H], good["y"][..., H:]
    _flagged(row, ops, with_y(torch.cat((yr, yf), -1)), "halves swapped")
    _flagged(row, ops, with_y(torch.cat((yf, yr.flip(0)), -1)), "reverse half not flipped back")
    with torch.no_grad():
        wrong = R.bilayer(cell, ops["x"], ops["wf"], ops["wf"])
    _flagged(row, ops, with_y(wrong), "reverse direction run with the forward weights")
    z = good["y"].clone()
    z[-1, :, H:] = 0
    _flagged(row, ops, with_y(z), "last frame of the reverse half zeroed")
    _flagged(row, ops, dict(good, dw_ih_f=good["dw_ih_r"], dw_ih_r=good["dw_ih_f"]), "weight gradients of the two directions swapped")
