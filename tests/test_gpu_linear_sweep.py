"""fsn_linear_forward / fsn_linear_backward held to an fp64 product over a shape sweep.  Needs an MI355X:
python -m pytest tests/test_gpu_linear_sweep.py -m gpu -s

Every nn.Linear and every weight / bias gradient of a training step runs through these two entries: the packed NN GEMM of
gemm_kernels.hip, the linear_small_out / linear_small_dx row-dot kernels, and the split-K C = A^T B family with its column
sums in gemm_tn_kernels.hip, whose host side picks one of five code paths from the shape alone.  TABLE below has one
row per shape, named after the path it is there for; the entries are called through fullsubnet_amd._lib directly so that
ldx, lddy, lddx and the three call forms of the backward are the test's to choose.

Two kinds of operands, two kinds of assertion (the checker, `check_outputs`, is also run on the CPU by
tests/test_linear_sweep_cpu.py with torch's fp32 product as a stand-in and with deliberately corrupted stand-ins):

* integer operands (x, dy in {0 .. 3} - {0, 1} where K is longest -, w in {-2 .. 2}, integer bias), drawn once by an index
  pattern and once by a seeded integer hash.  The test asserts on the fp64 reference that sum_k |a_k| |b_k| (+ |bias|)
  stays below 2^24 for every output element: every partial sum of every summation order is then an integer below 2^24,
  so fp32 FMA / MFMA accumulation is exact whatever the order and the number of K splits, and the HIP result must EQUAL
  the fp64 one.  Tolerance 0, derived.
* signed Gaussians (w * 0.1), two assertions per output tensor:
  hard  |C_hip - C_64| <= (K + S + 2) 2^-24 (|A|^T |B|)_ij per element ((K + S + 3) and + |bias| with a bias): K - 1
        additions and K products of a length-K dot product in ANY order lose at most one rounding each along the path
        of any term, S more for the sum of S split partials (S from fsn_debug_tn_plan for dw, 1 otherwise);
  sharp the root mean square over elements of err_ij / (|A|^T |B|)_ij is at most 4 x the same statistic of torch's CPU
        fp32 product (F.linear, dy @ w, dy.T @ x, dy.sum(0)) of the same operands against the same fp64 result.  A tensor
        of few elements is pooled over several draws (POOL_ELEMS) so that the statistic is one.
  Both statistics are printed per row (-s).

Also in every row: outputs are allocated larger than declared and pre-filled with a NaN sentinel, which must survive
outside [R][O], [R][I] of lddx, [O][I], [O], with finite values inside; the workspace is exactly
fsn_linear_workspace_bytes and pre-filled with 0xFF; results do not depend on ldx / lddy / lddx, ReLU equals the ReLU of
the plain result, the three forms of the backward and two calls in a row give the same bits.  Rows about the split-K plan
assert the split count they were written for (256 CUs) through fsn_debug_tn_plan.

Worst figures seen on an MI355X (hard = worst err / bound, must be <= 1; rms = sharp statistic in units of 2^-24):
  y   hard 0.20, rms hip / cpu 0.40 / 0.40 u (1.0 x): one FMA chain per element on both sides
  dx  hard 0.44 (fwd-manyrows R32785 I5 O3), rms 0.483 / 0.172 u = 2.8 x (colsum R255 I16 O1536: one chain of K = 1536
      against the CPU's blocked sum; 2.7 x on every K = 1536 row, 1.0 x on the small_dx kernel)
  dw  hard 0.35 (tn-reduce-only R7), rms 1.2 x at worst (tn-square R4128); 0.07 x at K = 2^20 + 3 (256 splits help)
  db  hard 0.19, rms 0.0108 / 0.0040 u = 2.7 x (colsum R1048579 O17; also tn-uneven-narrow R40100: 2.7 x).  With one chain
      of 2048 rows per block colsum_partial_kernel stood at 0.0190 / 0.0044 u = 4.3 x for R = 2^20 + 3, O >= 17 and failed
      this test; it now sums chains of 64 rows (same bits up to 64 rows per block, which is every shipped shape).
All integer rows equal the fp64 product, x of 2^31 + elements included (that row: 40 s; the module: 226 s, of which 112 s
are the CPU side of colsum R1048579 O1536); FSN_WS_CANARY=1: 169 passed.
"""
import ctypes
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENTINEL = 0x7FC0DEAD  # a quiet NaN with a recognisable payload
GUARD = 1024  # elements allocated (and checked) behind every output
POOL_ELEMS = 256  # rounding mode: draws are repeated until every output tensor has contributed this many elements ...
POOL_COST = 1 << 22  # ... as long as the row's draws together stay below this many operand elements
CHUNK = 1 << 17  # rows per block of the fp64 reference
LEAN = 1 << 28  # operand elements from which a row runs one layout only (the others would double several GB)
SHARP = 4.0


def ru16(n):
    return (n + 15) // 16 * 16


class Row:
    """One line of the sweep.  splits: None (not about the split plan), an int (exact count) or ">1"."""

    def __init__(self, path, R, I, O, splits=None, modes=("int", "gauss"), vmax=3):
        self.path, self.R, self.I, self.O, self.splits, self.modes, self.vmax = path, R, I, O, splits, modes, vmax

    @property
    def id(self):
        return f"{self.path}-R{self.R}-I{self.I}-O{self.O}"

    def scaled(self, r_max):
        """The same row with fewer rows (the CPU self-test of the checker); R % 16 is kept."""
        if self.R <= r_max:
            return self
        return Row(self.path, r_max + self.R % 16, self.I, self.O, None, self.modes, self.vmax)


def _table():
    rows = []
    # forward and dx: NN GEMM (pack in both orientations, bias, ReLU, edge tiles), small_out / small_dx (O <= 4, I % 64 == 0)
    shapes = [(1, 1), (5, 3), (16, 16), (17, 15), (20, 48), (64, 1), (64, 4), (64, 5), (65, 4), (128, 2), (257, 31),
              (384, 2), (512, 257), (130, 300)]
    n = 0
    for R in (1, 15, 16, 17, 33, 68, 4099):
        for I, O in shapes:
            small = O <= 4 and I % 64 == 0
            # rounding mode for every third row of the cross product: 14 shapes and 3 are coprime, so every R and every
            # shape has its share
            rows.append(Row("fwd-small" if small else "fwd-gemm", R, I, O, modes=("int", "gauss") if n % 3 == 0 else ("int",)))
            n += 1
    # >= 2048 row tiles: the NN GEMM's three many-row tile shapes (>= 4, 2 and 1 column tiles; 3 take the default) in y and dx
    for I, O in ((130, 300), (20, 48), (17, 15), (5, 3)):
        rows.append(Row("fwd-manyrows", (1 << 15) + 17, I, O))
    rows.append(Row("fwd-small-batch", (1 << 20) + 3, 384, 2, splits=">1"))  # the sub-band output layer at a real batch
    # x holds more than 2^31 elements (8.6 GB): index arithmetic; {0, 1} operands keep K = R = 2^22 + 5 exact
    rows.append(Row("fwd-small-2g", (1 << 22) + 5, 512, 2, splits=">1", modes=("int",), vmax=1))

    # dw / db: (O, I) = (M, Nc), R = K
    for R in (1, 7, 15):  # K < 16: tn_reduce_kernel forms the whole product, no split partial is read
        for O, I in ((2, 384), (48, 32), (257, 512)):
            rows.append(Row("tn-reduce-only", R, I, O, splits=1))
    for t in (0, 1, 13, 15):  # the K % 16 tail on every path
        rows.append(Row("tn-tail-swap", 2048 + t, 384, 2, splits=">1"))
        rows.append(Row("tn-tail-narrow", 2048 + t, 32, 48, splits=">1"))
        rows.append(Row("tn-tail-wide", 2048 + t, 512, 257, splits=">1"))
        rows.append(Row("tn-tail-square", 2048 + t, 384, 1536, splits=16))
    for O, I in ((1, 64), (2, 384), (32, 33), (4, 1000)):  # M <= 32 < Nc: operands swapped, partials transposed
        rows.append(Row("tn-swap", 1000, I, O, splits=">1"))
    for O, I in ((48, 32), (1536, 20), (600, 1), (513, 32)):  # 512 x 32 tiles; 513: a second M block of one row
        rows.append(Row("tn-narrow", 1000, I, O, splits=">1"))
    for O, I in ((257, 512), (300, 130), (256, 128), (1536, 257)):  # 256 x 128 tiles; (256, 128): exactly one
        rows.append(Row("tn-wide", 1000, I, O, splits=">1"))
    # 192 x 192 tiles, 256 / tiles splits pinned per XCD
    rows.append(Row("tn-square", 2061, 384, 1536, splits=16))
    rows.append(Row("tn-square", 4128, 384, 1536, splits=16))  # 258 chunks over 16 splits: a shorter last split
    rows.append(Row("tn-square", 8192 + 13, 384, 384, splits=64))
    rows.append(Row("tn-square", 32768, 192, 192, splits=256))
    # near-misses that must fall back to 256 x 128 tiles: K16 = 2032 < 16 x 128; 3 tiles do not divide 32 CUs per XCD
    rows.append(Row("tn-square-miss", 2047, 384, 1536, splits=13))
    rows.append(Row("tn-square-miss", 8192, 192, 576, splits=40))
    # a last split shorter than the others.  k_per_split is a multiple of 16, so the exact count pins it: 4992 rows in 32
    # splits and 40096 rows in 251 splits both mean 160 rows per split, the last one 32 / 96 rows
    rows.append(Row("tn-uneven-wide", 5000, 512, 257, splits=32))
    rows.append(Row("tn-uneven-narrow", 40100, 32, 48, splits=251))
    # column sums: colsum_narrow_kernel (<= 16 columns) / colsum_partial_kernel, one row block up to 513 of them
    for O in (1, 16, 17, 257, 1536):
        for R in (1, 255, 4099, (1 << 20) + 3):
            rows.append(Row("colsum", R, 16, O))
    return rows


TABLE = _table()


# ---- operands ---------------------------------------------------------------------------------------------------------

def _int_block(kind, salt, r0, r1, cols, lo, hi, device):
    """Integers in [lo, hi] as fp32, rows r0 .. r1 of a matrix: an index pattern (a row or column permutation shows) or a
    seeded hash of (row, column).  Element (0, 0) of every pattern is non-zero."""
    r = torch.arange(r0, r1, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(cols, dtype=torch.int64, device=device)[None, :]
    n = hi - lo + 1
    if kind == "pattern":
        a, b = ((1, 3), (3, 1), (1, 2), (2, 1))[salt % 4]
        v = (a * r + b * c + (1 - lo)) % n + lo
    else:
        h = (r * 0x9E3779B1 + c * 0x85EBCA77 + (salt + 1) * 0xC2B2AE3D) & 0xFFFFFFFF
        h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & 0xFFFFFFFF
        h = ((h ^ (h >> 12)) * 0x297A2D39) & 0xFFFFFFFF
        v = ((h ^ (h >> 15)) >> 8) % n + lo
    return v.to(torch.float32)


def _fill(rows, cols, fn, device):
    out = torch.empty((rows, cols), dtype=torch.float32, device=device)
    for r0 in range(0, rows, CHUNK):
        r1 = min(rows, r0 + CHUNK)
        out[r0:r1] = fn(r0, r1)
    return out


def make_operands(row, mode, draw, device):
    """x [R][I], w [O][I], b [O], dy [R][O] on `device`.  mode "int": draw 0 = index pattern, 1 = hash; "gauss": seed."""
    R, I, O = row.R, row.I, row.O
    if mode == "int":
        kind = "pattern" if draw == 0 else "hash"
        x = _fill(R, I, lambda a, b: _int_block(kind, 0, a, b, I, 0, row.vmax, device), device)
        dy = _fill(R, O, lambda a, b: _int_block(kind, 1, a, b, O, 0, row.vmax, device), device)
        w = _int_block(kind, 2, 0, O, I, -2, 2, device)
        b = _int_block(kind, 3, 0, 1, O, 1, 5, device)[0] if draw == 0 else _int_block(kind, 3, 0, 1, O, -3, 3, device)[0]
    else:
        g = torch.Generator(device=device).manual_seed(1000 * draw + R + 7 * I + 13 * O)
        x = _fill(R, I, lambda a, b: torch.randn(b - a, I, generator=g, device=device), device)
        dy = _fill(R, O, lambda a, b: torch.randn(b - a, O, generator=g, device=device), device)
        w = torch.randn(O, I, generator=g, device=device) * 0.1
        b = torch.randn(O, generator=g, device=device)
    return dict(x=x, w=w, b=b, dy=dy)


def cpu_products(ops):
    """torch's own fp32 CPU results: the reference implementation whose error the sharp bound is measured against."""
    x, w, b, dy = (ops[k] for k in ("x", "w", "b", "dy"))
    return dict(y=torch.nn.functional.linear(x, w, b), dx=dy @ w, dw=dy.t() @ x, db=dy.sum(0))


# ---- the checker ------------------------------------------------------------------------------------------------------

class Stat:
    """Error of one output tensor against fp64, accumulated over row blocks and draws."""

    def __init__(self, name, terms):
        self.name, self.terms = name, terms
        self.n = self.wrong = 0
        self.first_wrong = None
        self.max_abs = self.hard = 0.0
        self.ss = {"hip": 0.0, "cpu": 0.0}

    def add(self, got, ref64, abs64, cpu=None, r0=0):
        self.n += ref64.numel()
        self.max_abs = max(self.max_abs, float(abs64.max()))
        g = got.double()
        bad = g != ref64  # a NaN is unequal
        if bool(bad.any()):
            if self.first_wrong is None:
                i = [int(v) for v in bad.nonzero()[0]]
                self.first_wrong = ([i[0] + r0] + i[1:], float(g[tuple(i)]), float(ref64[tuple(i)]))
            self.wrong += int(bad.sum())
        if cpu is None:  # integer mode: equality is the whole check
            return
        pos = abs64 > 0
        for key, t in (("hip", g), ("cpu", cpu.double())):
            err = (t - ref64).abs()
            err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
            rel = torch.where(pos, err / torch.where(pos, abs64, torch.ones_like(abs64)),
                              torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
            self.ss[key] += float((rel * rel).sum())
            if key == "hip":
                self.hard = max(self.hard, float(rel.max()) / (self.terms * U))

    def rms(self, key):
        return math.sqrt(self.ss[key] / max(self.n, 1)) / U

    def assert_exact(self):
        assert self.max_abs < 2 ** 24, f"{self.name}: partial sums reach {self.max_abs:.0f} >= 2^24, the case is not exact"
        assert self.wrong == 0, (f"{self.name}: {self.wrong} of {self.n} elements differ from the fp64 product; first at "
                                 f"{self.first_wrong[0]}: got {self.first_wrong[1]!r}, expected {self.first_wrong[2]!r}")

    def assert_rounding(self):
        assert self.hard <= 1.0, f"{self.name}: worst element at {self.hard:.3f} of the (K + S + 2) 2^-24 |A|^T|B| bound"
        assert self.rms("hip") <= SHARP * self.rms("cpu"), \
            f"{self.name}: rms relative error {self.rms('hip'):.4f} u against {self.rms('cpu'):.4f} u of the CPU fp32 product"


def new_stats(row, splits):
    """One Stat per output; terms = the (K + S + 2) of the hard bound, one more where a bias is added."""
    return dict(y=Stat("y", row.I + 1 + 2 + 1), dx=Stat("dx", row.O + 1 + 2), dw=Stat("dw", row.R + splits + 2),
                db=Stat("db", row.R + 1 + 2))


def check_outputs(stats, ops, outs, cpu=None):
    """Accumulate into `stats` the comparison of outs = dict(y, dx, dw, db) (CPU fp32 tensors, the declared regions only;
    y WITHOUT ReLU) with the fp64 products of `ops`, formed in blocks of CHUNK rows; cpu: torch's fp32 results (rounding
    mode) or None."""
    w64, b64 = ops["w"].double(), ops["b"].double()
    R = ops["x"].shape[0]
    dw = torch.zeros_like(w64)
    dw_abs = torch.zeros_like(w64)
    db = torch.zeros_like(b64)
    db_abs = torch.zeros_like(b64)
    for r0 in range(0, R, CHUNK):
        r1 = min(R, r0 + CHUNK)
        x64, dy64 = ops["x"][r0:r1].double(), ops["dy"][r0:r1].double()
        xa, dya = x64.abs(), dy64.abs()
        if "y" in outs:
            stats["y"].add(outs["y"][r0:r1], x64 @ w64.t() + b64, xa @ w64.abs().t() + b64.abs(),
                           None if cpu is None else cpu["y"][r0:r1], r0)
        if "dx" in outs:
            stats["dx"].add(outs["dx"][r0:r1], dy64 @ w64, dya @ w64.abs(), None if cpu is None else cpu["dx"][r0:r1], r0)
        dw += dy64.t() @ x64
        dw_abs += dya.t() @ xa
        db += dy64.sum(0)
        db_abs += dya.sum(0)
    if "dw" in outs:
        stats["dw"].add(outs["dw"], dw, dw_abs, None if cpu is None else cpu["dw"])
    if "db" in outs:
        stats["db"].add(outs["db"], db, db_abs, None if cpu is None else cpu["db"])


def draws_for(row, mode):
    """Integer mode: the pattern and the hash.  Rounding mode: one draw, or as many as give the smallest output tensor
    (db: O elements) POOL_ELEMS elements, within POOL_COST operand elements."""
    if mode == "int":
        return 2
    want = -(-POOL_ELEMS // row.O)
    afford = max(1, POOL_COST // (row.R * (row.I + row.O)))
    return max(1, min(want, afford))


def tn_splits(L, row):
    s, bound = ctypes.c_int(0), ctypes.c_long(0)
    assert L.fsn_debug_tn_plan(row.O, row.I, row.R, 0, ctypes.byref(s), ctypes.byref(bound)) == 0
    assert 1 <= s.value <= bound.value
    return s.value


def check_plan(L, row):
    """The split count the row was written for (256 CUs): another device or a changed plan rule fails here instead of
    quietly testing a different path."""
    s = tn_splits(L, row)
    if row.splits == ">1":
        assert s > 1, f"{row.id}: one K split where the row is about several"
    elif row.splits is not None:
        assert s == row.splits, f"{row.id}: {s} K splits, the row expects {row.splits}"
    return s


# ---- the device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def _sentinel(n, dev):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)


def _untouched(buf, lo, what):
    assert bool((buf[lo:] == SENTINEL).all()), f"{what}: written outside its declared region"


def _padded(t, ld):
    """[rows][ld] copy of t with zero columns beyond its own (what the header requires of x and dy)."""
    if ld == t.shape[1]:
        return t.contiguous()
    out = torch.zeros((t.shape[0], ld), dtype=t.dtype, device=t.device)
    out[:, :t.shape[1]] = t
    return out


class Device:
    """The two entries on device operands, every output behind a sentinel and the workspace poisoned."""

    def __init__(self, fsn, row, ops):
        self.lib, self.L, self.row = fsn._lib, fsn._lib.lib(), row
        self.ops, self.dev = ops, ops["x"].device
        self.nbytes = self.L.fsn_linear_workspace_bytes(row.R, row.I, row.O)
        self._pads = {}

    def _ws(self):
        return self.lib.workspace(self.nbytes, self.dev).fill_(0xFF)  # 0xFFFFFFFF is a NaN; guarded under FSN_WS_CANARY

    def operand(self, name, ld):
        if (name, ld) not in self._pads:
            self._pads[(name, ld)] = _padded(self.ops[name], ld)
        return self._pads[(name, ld)]

    def forward(self, relu, ldx):
        R, I, O = self.row.R, self.row.I, self.row.O
        x, ws, buf = self.operand("x", ldx), self._ws(), _sentinel(R * O, self.dev)
        y = buf.view(torch.float32)
        p = self.lib.dev_ptr
        self.lib.check(self.L.fsn_linear_forward(p(x), ldx, p(self.ops["w"]), p(self.ops["b"]), R, I, O, relu, p(y),
                                                 ws.data_ptr(), ws.numel(), self.lib.stream_ptr(self.dev)))
        _untouched(buf, R * O, "y")
        y = y[:R * O].view(R, O)
        assert bool(torch.isfinite(y).all()), "y: not every declared element was written"
        return y

    def backward(self, ldx, lddy, lddx, want_dx=True, want_dw=True):
        R, I, O = self.row.R, self.row.I, self.row.O
        x, dy, ws = self.operand("x", ldx), self.operand("dy", lddy), self._ws()
        bufs = dict(dx=_sentinel(R * lddx, self.dev) if want_dx else None,
                    dw=_sentinel(O * I, self.dev) if want_dw else None, db=_sentinel(O, self.dev) if want_dw else None)
        p = self.lib.dev_ptr
        f = {k: (None if v is None else v.view(torch.float32)) for k, v in bufs.items()}
        self.lib.check(self.L.fsn_linear_backward(p(dy), lddy, p(x), ldx, p(self.ops["w"]), R, I, O,
                                                  p(f["dx"], allow_none=True), lddx, p(f["dw"], allow_none=True),
                                                  p(f["db"], allow_none=True), ws.data_ptr(), ws.numel(),
                                                  self.lib.stream_ptr(self.dev)))
        out = {}
        if want_dx:
            _untouched(bufs["dx"], R * lddx, "dx")
            if lddx > I:
                assert bool((bufs["dx"][:R * lddx].view(R, lddx)[:, I:] == SENTINEL).all()), "dx: columns beyond I written"
            out["dx"] = f["dx"][:R * lddx].view(R, lddx)[:, :I]
        if want_dw:
            _untouched(bufs["dw"], O * I, "dw")
            _untouched(bufs["db"], O, "db")
            out["dw"], out["db"] = f["dw"][:O * I].view(O, I), f["db"][:O]
        for k, v in out.items():
            assert bool(torch.isfinite(v).all()), f"{k}: not every declared element was written"
        return out


def _same(a, b, what):
    assert torch.equal(a, b), f"{what}: not bit-identical"


def run_draw(fsn, row, mode, draw, stats):
    dev = torch.device("cuda:0")
    ops = make_operands(row, mode, draw, dev)
    d = Device(fsn, row, ops)
    Ip, Op = ru16(row.I), ru16(row.O)
    lean = row.R * (Ip + Op) >= LEAN
    y = d.forward(0, Ip)
    _same(d.forward(1, Ip), torch.relu(y), "ReLU against the ReLU of the plain result")
    g = d.backward(Ip, Op, Ip)
    again = d.backward(Ip, Op, Ip)
    only_dx = d.backward(Ip, Op, Ip, want_dw=False)
    only_dw = d.backward(Ip, Op, Ip, want_dx=False)
    for k in ("dx", "dw", "db"):
        _same(again[k], g[k], f"{k}: two calls in a row")
        _same((only_dx if k == "dx" else only_dw)[k], g[k], f"{k}: alone against all three")
    del again, only_dx, only_dw
    if not lean:  # other leading dimensions (extra columns zero): the same bits
        _same(d.forward(0, Ip + 16), y, "y: ldx + 16")
        _same(d.forward(1, Ip + 16), torch.relu(y), "y: ldx + 16, ReLU")
        for ldx, lddy, lddx in ((Ip + 16, Op + 16, Ip + 20), (Ip, Op + 16, Ip + 20), (Ip + 16, Op, Ip)):
            h = d.backward(ldx, lddy, lddx)
            for k in ("dx", "dw", "db"):
                _same(h[k], g[k], f"{k}: ldx {ldx}, lddy {lddy}, lddx {lddx}")
        del h
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in ops.items()}
    outs = dict(y=y.cpu(), dx=g["dx"].cpu(), dw=g["dw"].cpu(), db=g["db"].cpu())
    del d, ops, y, g
    check_outputs(stats, host, outs, cpu_products(host) if mode == "gauss" else None)


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_linear_sweep(fsn, row):
    t0 = time.time()
    splits = check_plan(fsn._lib.lib(), row)
    for mode in row.modes:
        stats = new_stats(row, splits)
        for draw in range(draws_for(row, mode)):
            run_draw(fsn, row, mode, draw, stats)
        for s in stats.values():
            if mode == "int":
                s.assert_exact()
            else:
                print(f"[sweep] {row.id} {s.name}: n {s.n} S {splits} hard {s.hard:.4f} rms hip {s.rms('hip'):.4f} u "
                      f"cpu {s.rms('cpu'):.4f} u")
        if mode == "gauss":
            for s in stats.values():
                s.assert_rounding()
    print(f"[sweep] {row.id}: {time.time() - t0:.1f} s")
