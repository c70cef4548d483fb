"""``SequenceModel`` of audio_zen/model/module/sequence_model.py:26-125 on libfsn_hip.so.

Same constructor, same parameter names (``sequence_model.weight_ih_l{k}`` ..., ``fc_output_layer.*``),
same ``forward(x [B, F, T]) -> [B, O, T]``.  The ``nn.LSTM`` / ``nn.Linear`` members only hold the
parameters; every layer runs through the C ABI:

* inference (no autograd): ``fsn_lstm_layer_forward`` / ``fsn_gru_layer_forward`` (``save = NULL``) per
  layer + ``fsn_linear_forward``;
* training: ``LstmLayerFunction`` / ``GruLayerFunction`` / ``LinearFunction`` (fullsubnet_amd/train.py:
  forward with saved activations + back-propagation through time).

``bidirectional=True`` holds torch's bidirectional rnn (``*_reverse`` parameters, ``nn.Linear(2 * hidden_size, ..)``) and runs
layer by layer through ``fsn_lstm_bilayer_forward`` / ``fsn_gru_bilayer_forward`` (``BiLstmLayerFunction`` /
``BiGruLayerFunction`` in training): both directions of a layer advance in one launch per step.

Hidden sizes that are not a multiple of 64 (Fast FullSubNet's 257) are run zero-padded: a unit whose
weights and biases are all zero keeps h = c = 0 at every step, so the padding is exact.
"""
import torch
import torch.nn as nn

from . import _lib


def _round_up(x, m):
    return (x + m - 1) // m * m


def pad_lstm_weights(w_ih, w_hh, b_ih, b_hh, in_pad, hidden_pad=None, in_halves=None):
    """nn.LSTM / nn.GRU layer tensors ([gH, I], [gH, H], [gH], [gH], g = 4 / 3 gates) -> the same layer
    with H padded to a multiple of 64 (or to ``hidden_pad``) and I padded to ``in_pad`` columns (gate blocks stay
    contiguous).  Plain torch ops, so gradients flow back to the unpadded parameters when autograd is recording.
    ``in_halves`` = the width Hb of each direction of a bidirectional layer below (I = 2 Hb): its padded output is
    ``in_pad`` = 2 Hbp columns wide, so input columns [0, Hb) stay at [0, Hb) and columns [Hb, 2 Hb) go to
    [Hbp, Hbp + Hb)."""
    H, I = w_hh.shape[1], w_ih.shape[1]
    g = w_hh.shape[0] // H
    Hp = _round_up(H, 64) if hidden_pad is None else hidden_pad
    if in_halves is not None and (I != 2 * in_halves or in_pad % 2 or in_pad // 2 < in_halves):
        raise _lib.FsnError(f"pad_lstm_weights: {I} input columns are not two halves of {in_halves} within {in_pad}")
    if Hp == H and in_pad == I:
        return w_ih, w_hh, b_ih, b_hh
    dev = w_ih.device
    wi = torch.zeros((g, Hp, in_pad), dtype=torch.float32, device=dev)
    if in_halves is None:
        wi[:, :H, :I] = w_ih.reshape(g, H, I)
    else:
        Hb, Hbp = in_halves, in_pad // 2
        wi[:, :H, :Hb] = w_ih.reshape(g, H, I)[:, :, :Hb]
        wi[:, :H, Hbp:Hbp + Hb] = w_ih.reshape(g, H, I)[:, :, Hb:]
    wh = torch.zeros((g, Hp, Hp), dtype=torch.float32, device=dev)
    wh[:, :H, :H] = w_hh.reshape(g, H, H)
    bi = torch.zeros((g, Hp), dtype=torch.float32, device=dev)
    bi[:, :H] = b_ih.reshape(g, H)
    bh = torch.zeros((g, Hp), dtype=torch.float32, device=dev)
    bh[:, :H] = b_hh.reshape(g, H)
    return wi.reshape(g * Hp, in_pad), wh.reshape(g * Hp, Hp), bi.reshape(-1), bh.reshape(-1)


def lstm_layer_infer(x, w_ih, w_hh, b_ih, b_hh):
    """One LSTM layer, inference mode.  x [T, N, ldx] time-major, contiguous, N % 16 == 0, columns
    beyond I = w_ih.shape[1] zero; H = w_hh.shape[1] a multiple of 64.  Returns hseq [T, N, H]."""
    L = _lib.lib()
    T, N, ldx = x.shape
    I, H = w_ih.shape[1], w_hh.shape[1]
    hseq = torch.empty((T, N, H), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(L.fsn_lstm_layer_fwd_workspace_bytes(T, N, I, H), x.device)
    _lib.check(L.fsn_lstm_layer_forward(
        _lib.dev_ptr(x, "x"), ldx, _lib.dev_ptr(w_ih, "w_ih"), _lib.dev_ptr(w_hh, "w_hh"), _lib.dev_ptr(b_ih, "b_ih"),
        _lib.dev_ptr(b_hh, "b_hh"), T, N, I, H, _lib.dev_ptr(hseq), None, 0, ws.data_ptr(), ws.numel(),
        _lib.stream_ptr(x.device)))
    return hseq


WAVEFRONT_BELOW_ROWS = 96 * 16  # fewer rows than this: two equal-width LSTM layers run as one wavefront


def lstm2_infer(x, layer0, layer1):
    """Two stacked LSTM layers (equal or different hidden sizes), inference mode, as one wavefront of per-step
    launches (fsn_lstm2_forward).  x [T, N, ldx]; layer0 / layer1 = (w_ih, w_hh, b_ih, b_hh), padded.  Returns the
    hidden sequence of layer 1."""
    L = _lib.lib()
    T, N, ldx = x.shape
    I, H0, H1 = layer0[0].shape[1], layer0[1].shape[1], layer1[1].shape[1]
    if layer1[0].shape[1] != H0:
        raise _lib.FsnError("lstm2_infer: the second layer must take the first layer's (padded) hidden size as input")
    hseq = torch.empty((T, N, H1), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(L.fsn_lstm2_fwd_workspace_bytes(T, N, I, H0, H1), x.device)
    ptrs = [_lib.dev_ptr(t, "weight") for t in (*layer0, *layer1)]
    _lib.check(L.fsn_lstm2_forward(_lib.dev_ptr(x, "x"), ldx, *ptrs, T, N, I, H0, H1, _lib.dev_ptr(hseq),
                                   ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)))
    return hseq


def gru2_infer(x, layer0, layer1):
    """Two stacked GRU layers of equal (padded) width with few rows as ONE persistent launch (fsn_gru2_forward: the chain kernel
    with the GRU as a four-gate cell); the caller asked fsn_gru2_forward_supported.  x [T, N, ldx] -> layer 1's hidden sequence."""
    L = _lib.lib()
    T, N, ldx = x.shape
    I, H = layer0[0].shape[1], layer0[1].shape[1]
    hseq = torch.empty((T, N, H), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(L.fsn_gru2_fwd_workspace_bytes(T, N, I, H), x.device)
    ptrs = [_lib.dev_ptr(t, "weight") for t in (*layer0, *layer1)]
    _lib.check(L.fsn_gru2_forward(_lib.dev_ptr(x, "x"), ldx, *ptrs, T, N, I, H, _lib.dev_ptr(hseq), ws.data_ptr(), ws.numel(),
                                  _lib.stream_ptr(x.device)))
    return hseq


def gru_layer_infer(x, w_ih, w_hh, b_ih, b_hh):
    """One GRU layer, inference mode (same conventions as lstm_layer_infer, 3H gate rows r, z, n)."""
    L = _lib.lib()
    T, N, ldx = x.shape
    I, H = w_ih.shape[1], w_hh.shape[1]
    hseq = torch.empty((T, N, H), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(L.fsn_gru_layer_fwd_workspace_bytes(T, N, I, H), x.device)
    _lib.check(L.fsn_gru_layer_forward(
        _lib.dev_ptr(x, "x"), ldx, _lib.dev_ptr(w_ih, "w_ih"), _lib.dev_ptr(w_hh, "w_hh"), _lib.dev_ptr(b_ih, "b_ih"),
        _lib.dev_ptr(b_hh, "b_hh"), T, N, I, H, _lib.dev_ptr(hseq), None, 0, ws.data_ptr(), ws.numel(),
        _lib.stream_ptr(x.device)))
    return hseq


def bilayer_infer(cell, x, w_ih, w_hh, b_ih, b_hh):
    """One bidirectional LSTM / GRU layer, inference mode (fsn_lstm_bilayer_forward / fsn_gru_bilayer_forward: both directions
    per step launch).  x [T, N, ldx] as lstm_layer_infer takes it; the tensors carry a leading direction axis (0 forward,
    1 ``*_reverse``): w_ih [2, gH, I], w_hh [2, gH, H], b_* [2, gH].  Returns hseq [T, N, 2H], forward | reverse."""
    L = _lib.lib()
    T, N, ldx = x.shape
    I, H = w_ih.shape[2], w_hh.shape[2]
    query, entry = (L.fsn_lstm_bilayer_fwd_workspace_bytes, L.fsn_lstm_bilayer_forward) if cell == "LSTM" else \
        (L.fsn_gru_bilayer_fwd_workspace_bytes, L.fsn_gru_bilayer_forward)
    hseq = torch.empty((T, N, 2 * H), dtype=torch.float32, device=x.device)
    ws = _lib.workspace(query(T, N, I, H), x.device)
    _lib.check(entry(_lib.dev_ptr(x, "x"), ldx, _lib.dev_ptr(w_ih, "w_ih"), _lib.dev_ptr(w_hh, "w_hh"),
                     _lib.dev_ptr(b_ih, "b_ih"), _lib.dev_ptr(b_hh, "b_hh"), T, N, I, H, _lib.dev_ptr(hseq), 2 * H, None, 0,
                     ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)))
    return hseq


def linear_infer(x2, w, b, relu):
    """x2 [R, ldx] (columns beyond I = w.shape[1] zero, ldx % 16 == 0) -> [R, O] (+ ReLU)."""
    L = _lib.lib()
    R, ldx = x2.shape
    O, I = w.shape
    y = torch.empty((R, O), dtype=torch.float32, device=x2.device)
    ws = _lib.workspace(L.fsn_linear_workspace_bytes(R, I, O), x2.device)
    _lib.check(L.fsn_linear_forward(_lib.dev_ptr(x2, "x"), ldx, _lib.dev_ptr(w, "w"), _lib.dev_ptr(b, "b"), R, I, O,
                                    1 if relu else 0, _lib.dev_ptr(y), ws.data_ptr(), ws.numel(),
                                    _lib.stream_ptr(x2.device)))
    return y


def to_rows(x):
    """x [B, F, T] (inference, fp32, on the GPU) -> h [T, Np, Ip] time-major, zero beyond (B, F): the layout every LSTM /
    Linear entry takes (fsn_bft_to_rows: one transposing kernel instead of a fill and a strided copy of the host framework)."""
    B, F, T = x.shape
    Np, Ip = _round_up(B, 16), _round_up(F, 16)
    x = x.float()  # (the strided copy this replaced cast on the way; fp32 stays as it is)
    x = x if x.is_contiguous() else x.contiguous()
    h = torch.empty((T, Np, Ip), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().fsn_bft_to_rows(_lib.dev_ptr(x, "x"), B, F, T, _lib.dev_ptr(h), Np, Ip, _lib.stream_ptr(x.device)))
    return h


def from_rows(o, B):
    """o [T, Np, O] time-major as an entry wrote it (or a column slice of it: row stride o.stride(1)) -> [B, O, T] contiguous
    (fsn_rows_to_bft)."""
    T, Np, O = o.shape
    ld = o.stride(1)
    if o.stride(2) != 1 or o.stride(0) != Np * ld:
        o = o.contiguous()
        ld = O
    if not o.is_cuda or o.dtype != torch.float32:
        raise _lib.FsnError("from_rows: fp32 rows on a ROCm device")
    y = torch.empty((B, O, T), dtype=torch.float32, device=o.device)
    # (a column slice is not contiguous: its base address and row stride are what the entry takes)
    _lib.check(_lib.lib().fsn_rows_to_bft(o.data_ptr(), T, Np, ld, B, O, _lib.dev_ptr(y), _lib.stream_ptr(o.device)))
    return y


class SequenceModel(nn.Module):
    def __init__(self, input_size, output_size, hidden_size, num_layers, bidirectional, sequence_model="GRU",
                 output_activate_function="Tanh"):
        super().__init__()
        if sequence_model not in ("LSTM", "GRU"):
            raise NotImplementedError(f"Not implemented {sequence_model}")
        rnn = nn.LSTM if sequence_model == "LSTM" else nn.GRU
        self.bidirectional = bool(bidirectional)
        self.sequence_model = rnn(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers,
                                  batch_first=True, bidirectional=self.bidirectional)
        self.cell = sequence_model
        if int(output_size):
            self.fc_output_layer = nn.Linear(hidden_size * 2 if self.bidirectional else hidden_size, output_size)
        if output_activate_function:
            acts = {"Tanh": nn.Tanh, "ReLU": nn.ReLU, "ReLU6": nn.ReLU6, "LeakyReLU": nn.LeakyReLU, "PReLU": nn.PReLU}
            if output_activate_function not in acts:
                raise NotImplementedError(f"Not implemented activation function {output_activate_function}")
            self.activate_function = acts[output_activate_function]()
        self.output_activate_function = output_activate_function
        self.output_size = output_size
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self._padded = None
        self._padded_key = None

    # ---- inference weights, padded once per parameter version --------------------------------
    def _layer_tensors(self, k):
        m = self.sequence_model
        return (getattr(m, f"weight_ih_l{k}"), getattr(m, f"weight_hh_l{k}"), getattr(m, f"bias_ih_l{k}"),
                getattr(m, f"bias_hh_l{k}"))

    def _bi_layer_tensors(self, k):
        """Layer k of a bidirectional block, padded, each tensor with a leading direction axis (0 forward, 1 ``*_reverse``):
        what the bilayer entries take.  Each direction is padded to Hp units, so the layer's output is 2 Hp wide and the layer
        above reads its two halves at columns [0, H) and [Hp, Hp + H).  Plain torch ops (gradients reach the parameters)."""
        m, H, Hp = self.sequence_model, self.hidden_size, _round_up(self.hidden_size, 64)
        dirs = []
        for sfx in ("", "_reverse"):
            t = tuple(getattr(m, f"{n}_l{k}{sfx}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
            dirs.append(pad_lstm_weights(*t, self.input_size) if k == 0 else pad_lstm_weights(*t, 2 * Hp, in_halves=H))
        return tuple(torch.stack(pair) for pair in zip(*dirs))

    def _inference_weights(self):
        ps = list(self.parameters())
        key = tuple((p.data_ptr(), p._version, str(p.device)) for p in ps)
        if self._padded is None or key != self._padded_key:
            H, Hp = self.hidden_size, _round_up(self.hidden_size, 64)
            layers = []
            with torch.no_grad():
                for k in range(self.num_layers):
                    if self.bidirectional:
                        layers.append(tuple(t.detach().contiguous() for t in self._bi_layer_tensors(k)))
                        continue
                    in_pad = self.input_size if k == 0 else Hp
                    layers.append(tuple(t.detach().contiguous()
                                        for t in pad_lstm_weights(*self._layer_tensors(k), in_pad)))
                fc = None
                if self.output_size and self.bidirectional:  # the two halves of the [.., 2 Hp] sequence
                    w = torch.zeros((self.output_size, 2 * Hp), dtype=torch.float32, device=ps[0].device)
                    w[:, :H] = self.fc_output_layer.weight.detach()[:, :H]
                    w[:, Hp:Hp + H] = self.fc_output_layer.weight.detach()[:, H:]
                    fc = (w, self.fc_output_layer.bias.detach().contiguous())
                elif self.output_size:
                    w = torch.zeros((self.output_size, Hp), dtype=torch.float32, device=ps[0].device)
                    w[:, :self.hidden_size] = self.fc_output_layer.weight.detach()
                    fc = (w, self.fc_output_layer.bias.detach().contiguous())
            self._padded, self._padded_key = (layers, fc), key
        return self._padded

    def forward(self, x):
        """x [B, F, T] -> [B, O, T] (O = hidden_size when there is no output layer)."""
        assert x.dim() == 3, f"The shape of input is {x.shape}."
        if not x.is_cuda:
            raise _lib.FsnError("SequenceModel: input must live on a ROCm device; this path has no CPU implementation")
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return self._forward_train(x)
        return self.forward_time_major(to_rows(x), x.shape[0])

    def forward_time_major(self, h, B, rows_out=False):
        """Inference on an input that is already laid out as the LSTM entries take it: h [T, Np, Ip] time-major, rows
        beyond B and columns beyond input_size zero (Np, Ip multiples of 16) -> [B, O, T]; ``rows_out``: the output as it
        lies, [T, Np, O] (rows beyond B are not meaningful) - what the next block's time-major entry takes."""
        T, Np, _ = h.shape
        H, Hp = self.hidden_size, _round_up(self.hidden_size, 64)
        layers, fc = self._inference_weights()
        if self.bidirectional:
            # layer by layer through the bilayer entry (both directions per step launch); none of the wavefront, chain and
            # persistent shortcuts below applies.  The sequence is [T, Np, 2 Hp]: forward | reverse, each padded to Hp
            for w_ih, w_hh, b_ih, b_hh in layers:
                h = bilayer_infer(self.cell, h, w_ih, w_hh, b_ih, b_hh)
            relu = self.output_activate_function == "ReLU"
            if fc is not None:
                o = linear_infer(h.reshape(T * Np, 2 * Hp), fc[0], fc[1], relu).reshape(T, Np, self.output_size)
            else:
                o = h if Hp == H else torch.cat((h[:, :, :H], h[:, :, Hp:Hp + H]), dim=2)
                relu = False
            if self.output_activate_function and not relu:
                o = self.activate_function(o)
            return o if rows_out else from_rows(o, B)
        layer_infer = lstm_layer_infer if self.cell == "LSTM" else gru_layer_infer
        k = 0
        if self.cell == "LSTM":
            # consecutive layers two by two (fsn_lstm2_forward) where that pays: few rows - latency-bound, half the
            # dependent launches, or ONE launch of the chain kernel up to 64 rows - or a shape with a persistent
            # two-layer kernel; a left-over layer (the full-band baseline has three) runs on its own below
            while k + 1 < len(layers):
                width = h.shape[2]
                if not (Np < WAVEFRONT_BELOW_ROWS or _lib.lib().fsn_lstm2_forward_is_persistent(T, Np, width, width, Hp, Hp)):
                    break
                h = lstm2_infer(h, layers[k], layers[k + 1])
                k += 2
        elif self.cell == "GRU":
            # two GRU layers with few rows (a GRU FullSubNet's full-band model): one persistent launch where the chain kernel applies
            while k + 1 < len(layers) and layers[k][1].shape[1] == layers[k + 1][1].shape[1] and \
                    _lib.lib().fsn_gru2_forward_supported(T, Np, layers[k][1].shape[1]):
                h = gru2_infer(h, layers[k], layers[k + 1])
                k += 2
        for w_ih, w_hh, b_ih, b_hh in layers[k:]:
            h = layer_infer(h, w_ih, w_hh, b_ih, b_hh)
        relu = self.output_activate_function == "ReLU"
        if fc is not None:
            o = linear_infer(h.reshape(T * Np, Hp), fc[0], fc[1], relu).reshape(T, Np, self.output_size)
        else:
            o = h[:, :, :H]
            relu = False
        if self.output_activate_function and not relu:
            o = self.activate_function(o)
        return o if rows_out else from_rows(o, B)

    def _forward_train(self, x):
        from .train import GruLayerFunction, LinearFunction, LstmLayerFunction, lstm2_rows_chunked, lstm2_train_chunks
        H, Hp = self.hidden_size, _round_up(self.hidden_size, 64)
        layer = LstmLayerFunction if self.cell == "LSTM" else GruLayerFunction
        h = x.permute(2, 0, 1)  # [T, B, F]
        # ``train_arithmetic`` (set by the owning model from Model.train_arithmetic = the trainer's use_amp): under the 16-bit
        # autocast arithmetic a two-layer stack of the group kernels' width runs on the persistent training kernels, in
        # pieces of whole clusters when it has more rows than one launch holds (Fast FullSubNet's bottleneck: 3 x 1536 rows
        # at the shipped batch of 72); fp32 and every other shape layer by layer as before
        if self.bidirectional:
            # fp32 whatever train_arithmetic says (BiLstmLayerFunction / BiGruLayerFunction)
            from .train import BiGruLayerFunction, BiLstmLayerFunction
            bilayer = BiLstmLayerFunction if self.cell == "LSTM" else BiGruLayerFunction
            for k in range(self.num_layers):
                h = bilayer.apply(h, *self._bi_layer_tensors(k))
            if Hp != H:
                h = torch.cat((h[..., :H], h[..., Hp:Hp + H]), dim=-1)
            relu = self.output_activate_function == "ReLU"
            if self.output_size:
                o = LinearFunction.apply(h, self.fc_output_layer.weight, self.fc_output_layer.bias, relu)
            else:
                o, relu = h, False
            if self.output_activate_function and not relu:
                o = self.activate_function(o)
            return o.permute(1, 2, 0)
        arith = getattr(self, "train_arithmetic", "f32")
        chunks = None
        if self.cell == "LSTM" and self.num_layers == 2 and arith != "f32" and Hp == H:
            chunks = lstm2_train_chunks(h.shape[0], h.shape[1], h.shape[2], H, pad_small=h.shape[1] >= 256)
        if chunks is not None:
            params = [t for k in (0, 1) for t in self._layer_tensors(k)]
            h = lstm2_rows_chunked(h, params, arith, *chunks)
        else:
            for k in range(self.num_layers):
                in_pad = self.input_size if k == 0 else Hp
                h = layer.apply(h, *pad_lstm_weights(*self._layer_tensors(k), in_pad))
        h = h[..., :H]
        relu = self.output_activate_function == "ReLU"
        if self.output_size:
            o = LinearFunction.apply(h, self.fc_output_layer.weight, self.fc_output_layer.bias, relu)
        else:
            o, relu = h, False
        if self.output_activate_function and not relu:
            o = self.activate_function(o)
        return o.permute(1, 2, 0)


def multi_plan(models, shapes):
    """Whether ``multi_forward`` would run these two-layer LSTM SequenceModels on inputs of ``shapes`` [(B_i, F_i, T)] as
    ONE persistent launch (fsn_lstm2_multi_is_persistent); callers keep small stacks on one stream each otherwise."""
    import ctypes
    n = len(models)
    if n < 1 or n > 8 or any(m.cell != "LSTM" or m.num_layers != 2 or m.bidirectional for m in models):
        return False
    stacks = (_lib.Lstm2Stack * n)()
    for q, m, (B, F, T) in zip(stacks, models, shapes):
        Hp = _round_up(m.hidden_size, 64)
        q.N, q.I, q.H0, q.H1 = _round_up(B, 16), F, Hp, Hp
    return bool(_lib.lib().fsn_lstm2_multi_is_persistent(n, ctypes.byref(stacks), shapes[0][2]))


def multi_forward(models, xs=None, prepared=None, rows_out=False):
    """Several independent two-layer LSTM SequenceModels over the SAME frames (the band sections of Improved FullSubNet,
    improved_fullsubnet/model.py:402-449) through fsn_lstm2_forward_multi: one persistent launch of the group kernel with
    one weight set per model when ``multi_plan`` says so.  models[i](xs[i]) for xs[i] [B_i, F_i, T] -> list of
    [B_i, O_i, T] (``rows_out``: of [T, Np_i, O_i] time-major, as the output layers wrote them); or ``prepared[i] = (h_i [T, Np_i, Ip_i], B_i)``, inputs already in the entries' time-major zero-padded
    layout.  Inference only."""
    import ctypes
    L = _lib.lib()
    n = len(models)
    given = prepared if prepared is not None else xs
    if n < 1 or n > 8 or given is None or len(given) != n:
        raise _lib.FsnError("multi_forward: 1 .. 8 models with one input each")
    if prepared is None:
        prepared = []
        for x in xs:
            if x.dim() != 3 or not x.is_cuda:
                raise _lib.FsnError("multi_forward: GPU inputs [B, F, T]")
            prepared.append((to_rows(x), x.shape[0]))
    T = prepared[0][0].shape[0]
    dev = prepared[0][0].device
    stacks = (_lib.Lstm2Stack * n)()
    keep, hseqs, meta = [], [], []
    for i, (m, (h, B)) in enumerate(zip(models, prepared)):
        if m.cell != "LSTM" or m.num_layers != 2 or m.bidirectional or h.dim() != 3 or h.shape[0] != T or not h.is_cuda:
            raise _lib.FsnError("multi_forward: unidirectional two-layer LSTM SequenceModels on GPU inputs with a common T")
        Hp = _round_up(m.hidden_size, 64)
        Np, Ip = h.shape[1], h.shape[2]
        layers, fc = m._inference_weights()
        hseq = torch.empty((T, Np, Hp), dtype=torch.float32, device=dev)
        q = stacks[i]
        q.x, q.ldx = h.data_ptr(), Ip
        for name, t in zip(("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1"), (*layers[0], *layers[1])):
            setattr(q, name, _lib.dev_ptr(t, name).value)
        q.N, q.I, q.H0, q.H1, q.hseq1 = Np, layers[0][0].shape[1], Hp, Hp, hseq.data_ptr()
        keep.append((h, layers))
        hseqs.append(hseq)
        meta.append((B, Np, Hp, fc))
    nbytes = L.fsn_lstm2_multi_workspace_bytes(n, ctypes.byref(stacks), T)
    ws = _lib.workspace(nbytes, dev)
    _lib.check(L.fsn_lstm2_forward_multi(n, ctypes.byref(stacks), T, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    outs = []
    for m, hseq, (B, Np, Hp, fc) in zip(models, hseqs, meta):
        relu = m.output_activate_function == "ReLU"
        if fc is not None:
            o = linear_infer(hseq.reshape(T * Np, Hp), fc[0], fc[1], relu).reshape(T, Np, m.output_size)
        else:
            o, relu = hseq[:, :, :m.hidden_size], False
        if m.output_activate_function and not relu:
            o = m.activate_function(o)
        outs.append(o if rows_out else from_rows(o, B))  # rows_out: [T, Np, O] as it lies (rows beyond B are not meaningful)
    return outs


def pair_fusable(block0, block1, rows):
    """Whether two consecutive SequenceModel blocks run as ONE two-layer recurrence in inference (``pair_forward``): both
    single-layer unidirectional LSTM blocks, block0 without output layer / activation, few rows."""
    return (block0.cell == block1.cell == "LSTM" and block0.num_layers == block1.num_layers == 1
            and not block0.bidirectional and not block1.bidirectional
            and not block0.output_size and not block0.output_activate_function
            and block1.input_size == block0.hidden_size and _round_up(rows, 16) < WAVEFRONT_BELOW_ROWS)


def pair_forward_rows(block0, block1, h):
    """``block1(block0(.))`` of a fusable pair on time-major rows: h [T, Np, Ip] (zero beyond the block's input width) ->
    [T, Np, O] as the output layer writes it (rows beyond the batch are not meaningful)."""
    if block0.bidirectional or block1.bidirectional:
        raise _lib.FsnError("pair_forward_rows: a bidirectional block does not run as a wavefront pair")
    T, Np, _ = h.shape
    (layer0,), _ = block0._inference_weights()
    _, fc = block1._inference_weights()
    Hp0, Hp1 = layer0[1].shape[1], _round_up(block1.hidden_size, 64)
    # Up to 64 rows two EQUAL-width layers of 384 or 512 units are one launch of the chain kernel (fb_chain_kernels.hip)
    # instead of T + 1 dependent ones: blocks of different widths (Fast FullSubNet's encoder, 384 -> 320) are padded to
    # the wider one for that - units with zero weights and biases keep h = c = 0, so the padding is exact
    width = max(Hp0, Hp1)
    chain = Np <= 64 and width in (384, 512)
    H0t, H1t = (width, width) if chain else (Hp0, Hp1)
    key = (block0._padded_key, block1._padded_key, H0t, H1t)
    cached = getattr(block1, "_pair_cache", None)
    if cached is None or cached[0] != key:
        with torch.no_grad():
            if H0t != Hp0:
                layer0 = tuple(t.detach().contiguous() for t in
                               pad_lstm_weights(*block0._layer_tensors(0), block0.input_size, hidden_pad=H0t))
            # block1's weights take block0.hidden_size inputs: widened to block0's (padded) width
            layer1 = tuple(t.detach().contiguous() for t in pad_lstm_weights(*block1._layer_tensors(0), H0t, hidden_pad=H1t))
        cached = (key, layer0, layer1)
        block1._pair_cache = cached
    _, layer0, layer1 = cached
    h = lstm2_infer(h, layer0, layer1)
    if h.shape[2] != Hp1:
        h = h[:, :, :Hp1].contiguous()
    relu = block1.output_activate_function == "ReLU"
    if fc is not None:
        o = linear_infer(h.reshape(T * Np, Hp1), fc[0], fc[1], relu).reshape(T, Np, block1.output_size)
    else:
        o, relu = h[:, :, :block1.hidden_size], False
    if block1.output_activate_function and not relu:
        o = block1.activate_function(o)
    return o


def pair_forward(block0, block1, x):
    """``block1(block0(x))`` for two consecutive SequenceModel blocks (an ``nn.Sequential`` pair of the sibling
    models).  In inference, when both are single-layer LSTM blocks, block0 has no output layer / activation and
    there are few rows, the two recurrences advance as one wavefront (fsn_lstm2_forward); otherwise block by
    block."""
    if torch.is_grad_enabled() or not x.is_cuda or not pair_fusable(block0, block1, x.shape[0]):
        return block1(block0(x))
    return from_rows(pair_forward_rows(block0, block1, to_rows(x)), x.shape[0])
