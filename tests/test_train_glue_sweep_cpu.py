"""The table, the oracles and the checkers of tests/test_gpu_train_glue_sweep.py, tried without a GPU.

* The oracle itself: the torch transcription's forward equals the numpy oracle to 1e-12 relative on every glue row; the
  float64 Adam transcription agrees with torch.optim.Adam + clip_grad_norm_ run in float64, and with the fp32 one at the
  tolerances of test_clip_adam_vs_torch; the MSE one with torch.nn.functional.mse_loss.
* The checkers accept the oracle at float32 (its fp32 mode forms the statistics in fp64 and casts once, like the kernels)
  and torch's own fp32 Adam / MSE / target, and reject each of eleven wrong stand-ins made from the oracle.
* The size queries (host code, no device needed): fsn_train_rows against the oracle's row order, fsn_train_den_elems and
  fsn_train_glue_workspace_bytes against the regions the host code carves (this pins the size formula; overruns are
  FSN_WS_CANARY's to catch), over all rows of the table.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_train_glue_sweep as S

GLUE = [(r, n) for r in S.GLUE_ROWS for n in r.norms]
GLUE_IDS = [f"{r.id}-{n}" for r, n in GLUE]
ROW = {r.id: r for r in S.TABLE}


def _fp32_oracle_outs(d, ops):
    outs = {k: v.astype(np.float32) for k, v in S.oracle_forward(d, ops["mag"].numpy(), ops["fb"].numpy(), dtype=np.float32).items()}
    cpu = S.glue_standin(d, ops)
    outs.update(d_fb=cpu["d_fb"], mask=cpu["mask"], dy=cpu["dy"])
    return outs


def _judge(row, d, make_outs):
    """Pooled over the row's draws like the GPU test; make_outs(ops) -> the outputs to judge."""
    stats = {}
    for draw in range(S.glue_draws(row, d)):
        ops = S.make_glue_ops(row, d, draw)
        arith, exact = S.glue_reference(d, ops)
        S.check_glue(stats, arith, exact, make_outs(ops))
    for s in stats.values():
        s.check()
    return stats


@pytest.mark.parametrize("row,norm", GLUE, ids=GLUE_IDS)
def test_torch_transcription_equals_the_numpy_oracle(row, norm):
    d = S.glue_dims(row, norm)
    ops = S.make_glue_ops(row, d, 0)
    want = S.oracle_forward(d, ops["mag"].numpy(), ops["fb"].numpy())
    got = S.torch_sequence(d, ops["mag"].double(), ops["fb"].double())
    for k, w in want.items():
        assert got[k].shape == w.shape
        assert float(np.abs(got[k].numpy() - w).max()) <= 1e-12 * float(np.abs(w).max()), k


@pytest.mark.parametrize("row,norm", GLUE, ids=GLUE_IDS)
def test_checkers_accept_the_oracle_at_float32(row, norm):
    d = S.glue_dims(row, norm)
    stats = _judge(row, d, lambda ops: _fp32_oracle_outs(d, ops))
    assert all(s.scalar or s.n >= S.POOL_ELEMS for s in stats.values())


WRONG = [  # (stand-in, row, norm, the output that must give it away)
    ("edge_repeat", "bins-F33-nb7", S.OFF, "sb_in"),
    ("edge_repeat", "bins-F33-nb7", S.CUM, "sb_in"),
    ("mean_kept_rows", "dropband-g2-B5", S.OFF, "sb_in"),
    ("count_off_by_one", "frames-Tp9-la2", S.CUM, "x_tm"),
    ("no_lookahead_count", "frames-Tp9-la2", S.CUM, "sb_in"),
    ("stop_at_frame", "frames-Tp9-la2", S.CUM, "d_fb"),
    ("no_dmu_dropped", "dropband-g2-B5", S.OFF, "d_fb"),
    ("no_gate", "frames-Tp9-la2", S.OFF, "d_fb"),
    ("no_gate", "frames-Tp9-la2", S.CUM, "d_fb"),
    ("interleave", "dropband-g2-B5", S.OFF, "sb_in"),
    ("interleave", "dropband-g3-B7", S.CUM, "sb_in"),
]


@pytest.mark.parametrize("variant,row_id,norm,name", WRONG, ids=[f"{v}-{r}-{n}" for v, r, n, _ in WRONG])
def test_wrong_standins_are_rejected(variant, row_id, norm, name):
    """Evaluated at float64 and rounded once, so that nothing but the defect separates the stand-in from the reference;
    the named output alone must be enough."""
    row = ROW[row_id]
    d = S.glue_dims(row, norm)
    ops = S.make_glue_ops(row, d, 0)
    good = S.glue_standin(d, ops, dtype=torch.float64)
    bad = S.glue_standin(d, ops, variant, dtype=torch.float64)
    _judge(row, d, lambda o: dict(S.glue_standin(d, o, dtype=torch.float64), mag_tm=S.glue_exact(d, o)["mag_tm"]))
    assert not np.array_equal(bad[name], good[name]), "the stand-in is not wrong at this row"
    with pytest.raises(AssertionError):
        _judge(row, d, lambda o: {name: S.glue_standin(d, o, variant, dtype=torch.float64)[name]})


@pytest.mark.parametrize("name", ["x_tm", "sb_in"])
@pytest.mark.parametrize("norm", [S.OFF, S.CUM])
def test_two_ulp_at_tensor_max_scale_is_rejected(name, norm):
    row = ROW["frames-Tp33-la0"]
    d = S.glue_dims(row, norm)
    def off_by_two_ulp(ops):
        t = _fp32_oracle_outs(d, ops)[name].copy()
        i = np.unravel_index(int(np.argmin(np.abs(t) + (t == 0) * 1e30)), t.shape)  # the smallest element, the largest scale
        t[i] += 2 * np.spacing(np.abs(t).max())
        return {name: t}

    with pytest.raises(AssertionError):
        _judge(row, d, off_by_two_ulp)


def test_exact_checker_tells_minus_zero_and_a_moved_element():
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    S.check_exact("same", a.copy(), a)
    for bad in (np.where(a == 0, np.float32(-0.0), a), np.roll(a, 1, axis=1)):
        with pytest.raises(AssertionError):
            S.check_exact("bad", bad, a)


@pytest.mark.parametrize("row", S.GLUE_ROWS, ids=[r.id for r in S.GLUE_ROWS])
def test_size_queries(row):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    for norm in (S.OFF, S.CUM):
        d = S.glue_dims(row, norm)
        dims = _lib.TrainDims(d.B, d.F, d.T, d.la, d.nb, d.groups, S.NORM_ID[norm])
        Fs, R = ctypes.c_int(0), ctypes.c_int(0)
        assert L.fsn_train_rows(ctypes.byref(dims), ctypes.byref(Fs), ctypes.byref(R)) == 0
        order = S.row_order(d)
        assert (Fs.value, R.value) == (d.Fs, len(order)) and len(set(order)) == len(order)
        for Rp in (d.R, S.ru(d.R, 16), S.ru(d.R, 64)):
            assert L.fsn_train_den_elems(ctypes.byref(dims), Rp) == (d.B if norm == S.OFF else d.Tp * Rp)
        need = S.needed_ws_bytes(d)
        assert need <= L.fsn_train_glue_workspace_bytes(ctypes.byref(dims)) <= need + 256


# ---- target, MSE, Adam ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [r for r in S.TABLE if r.kind == "target"], ids=lambda r: r.id)
def test_target_oracle_accepts_torch_fp32(row):
    """mask.py:7-44 in torch at float32 against the numpy oracle at float64.  The hard figure is printed only (no
    documented expf bound); here the stand-in is the CPU evaluation itself, so the sharp ratio is 1."""
    st, worse = S.Stat("target"), S.Stat("target")
    for draw in range(S.target_draws(row)):
        ops = S.make_target_ops(row, draw)
        d, (ref, Sabs, cpu) = S.target_reference(row, ops)
        assert ref.shape == (d.B, 2, d.Fs, d.T) and float(ref.min()) < -9.99 and float(ref.max()) > 9.8
        assert ref[0, 0, 0, 0] == 0.0 and ref[0, 1, 0, 0] == 0.0  # the 0 + 0i noisy bin
        st.add(cpu, ref, Sabs, cpu)
        bad = cpu.copy()
        bad[0, 1] = cpu[0, 0]  # real part where the imaginary one belongs
        worse.add(bad, ref, Sabs, cpu)
    assert st.n >= S.POOL_ELEMS
    st.check()
    assert st.hard <= 1.0  # torch's own expf meets the k = 8 figure: the S of the target is not too small
    with pytest.raises(AssertionError):
        worse.check()


@pytest.mark.parametrize("row", [r for r in S.TABLE if r.kind == "mse" and r.draws == 1], ids=lambda r: r.id)
def test_mse_oracle_accepts_torch_fp32(row):
    x, y = S.make_mse_ops(row, 0)
    ref = S.mse_reference(x, y)
    for name in ("loss", "grad"):
        r, Sabs, cpu = ref[name]
        st = S.Stat(name)
        st.add(cpu, r, Sabs, cpu)
        assert st.hard <= (1.0 if name == "grad" else 8.0)  # torch sums the squares in fp32: beyond the kernel's k = 3
    if row.signal == "identical":
        assert ref["loss"][0][0] == 0.0 and not ref["grad"][0].any()


ADAM_ROWS = [r for r in S.TABLE if r.kind == "adam" and not r.kw.get("norm_only")]


def _case(row):
    return S.AdamCase(row.sizes, row.step, row.betas, row.clip, row.gval, row.scale)


@pytest.mark.parametrize("row", ADAM_ROWS, ids=lambda r: r.id)
def test_adam_oracle_agrees_with_torch(row):
    c = _case(row)
    ref = S.adam_oracle(c)
    t64, t32 = S.adam_torch(c, torch.float64), S.adam_torch(c, torch.float32)
    assert abs(t64["norm"][0] - ref["norm"][0][0]) <= 1e-12 * ref["norm"][0][0]
    if row.gval == 1.0:  # (gradients of 1e-30: torch's fp32 norm underflows to 0; the kernel's fp64 sum does not)
        assert abs(t32["norm"][0] - ref["norm"][0][0]) <= 1e-5 * ref["norm"][0][0]
    tol32 = dict(g=1e-6, p=2e-6, m=1e-6, v=1e-5)  # test_clip_adam_vs_torch's
    for name in ("g", "m", "v", "p"):
        for (r, _), a, b in zip(ref[name], t64[name], t32[name]):
            scale = max(float(np.abs(r).max()), 1e-300)
            assert float(np.abs(a - r).max()) <= 1e-12 * scale, name
            assert float(np.abs(b - r).max()) <= tol32[name] * (max(scale, 1.0) if name == "g" else 1.0), name


@pytest.mark.parametrize("row", ADAM_ROWS, ids=lambda r: r.id)
def test_adam_checker_accepts_torch_fp32(row):
    c = _case(row)
    t32 = S.adam_torch(c, torch.float32)
    stats = {}
    # gradients of 1e-30: torch's own fp32 norm underflows to 0 and is no acceptable norm; the kernel sums in fp64
    names = ("g", "m", "v", "p") if row.gval != 1.0 else ("norm", "g", "m", "v", "p")
    S.check_adam(stats, S.adam_oracle(c), t32, t32, names=names)
    for s in stats.values():
        s.check()


@pytest.mark.parametrize("variant,row_id", [("no_clamp", "adam-32-tensors-step2-above-clamp"), ("bc2_prev_step", "adam-scale65536"),
                                            ("bc2_prev_step", "adam-step1000-betas.5-.9999-clip1e-3"), ("bc2_prev_step", "adam-sizes-step1")])
def test_wrong_adam_is_rejected(variant, row_id):
    c = _case(ROW[row_id])
    bad = S.adam_oracle(c, variant=variant)
    got = {k: ([r.astype(np.float32) for r, _ in v] if k != "norm" else v[0]) for k, v in bad.items()}
    good = S.adam_oracle(c)
    t32 = S.adam_torch(c, torch.float32)
    stats = {}
    S.check_adam(stats, good, got, t32)
    with pytest.raises(AssertionError):
        for s in stats.values():
            s.check()


def test_pieces_reference_round_trip():
    for row in (r for r in S.TABLE if r.kind == "pieces"):
        src = np.random.default_rng(row.N).standard_normal((row.T, row.N, row.W)).astype(np.float32)
        pieces = S.pieces_reference(src, row.T, row.N, row.W, row.rows, row.n)
        assert pieces.shape == (row.n, row.T, row.rows, row.W)
        back = pieces.transpose(1, 0, 2, 3).reshape(row.T, row.n * row.rows, row.W)
        assert np.array_equal(back[:, :row.N], src) and not back[:, row.N:].any()
