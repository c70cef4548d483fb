"""Time of the streaming resampler (fsn_resample_stream_push, fullsubnet_amd.StreamResampler) on one MI355X, beside the
same work done with the offline call, and of a StreamPool tick at 48 kHz beside one at the model's rate:

    python tools/bench_stream_resample.py [--sessions 1 8 32 64] [--ticks 40] [--commit SHA] [--write] [--out profiles/stream_resample.md]

Per case (48 -> 16, 16 -> 48, 44.1 -> 16 kHz with "scipy", 48 -> 16 kHz with "sharp") and session count n, one tick is a
chunk of 16 ms per session (768, 256 and 706 samples), every session in mid-stream:
  entry     ONE fsn_resample_stream_push through the binding into buffers and an item table made once (the same items every
            time: the launch reads one history buffer and writes the other, so a repeat does the same work)
  push()    ONE StreamResampler.push({sid: chunk, ..}): the entry plus what Python does around it - the book, one
            torch.stack of the chunks (equal lengths), one small copy of the item table, the output
  offline   today's way: per session ONE resample.resample over its last J - 1 samples + the chunk (a torch.cat each), the
            outputs that depend on samples not yet there cut off - n library calls of two launches each
Every figure is the median of three windows of --ticks ticks between two device events, after ten warm-up ticks; where the
host cannot keep the device busy the window measures the host, which is what a server sees.  The pool: n push(chunk) + ONE
step() per tick, FullSubNet with seeded weights, at 48 kHz in and out and at the model's rate.  `--write` puts the tables
into profiles/stream_resample.md (or --out)."""
import argparse
import datetime
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# (sr_in, sr_out, design, samples of a 16 ms chunk)
CASES = ((48000, 16000, "scipy", 768), (16000, 48000, "scipy", 256), (44100, 16000, "scipy", 706), (48000, 16000, "sharp", 768))
WARMUP = 10


def windows_us(tick, ticks):
    """us per tick(i): median (and range) of three windows of ``ticks`` calls between device events."""
    import torch
    i = 0
    for _ in range(WARMUP):
        tick(i)
        i += 1
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(ticks):
            tick(i)
            i += 1
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / ticks * 1e3)
    return statistics.median(out), min(out), max(out)


def resampler_case(fsn, sr_in, sr_out, design, chunk, n, ticks):
    import torch
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    torch.manual_seed(n + sr_in)
    x = torch.randn(n, chunk, device="cuda")
    rs = fsn.StreamResampler(sr_in, sr_out, capacity=n, design=design)
    sids = [rs.open() for _ in range(n)]
    rs.push({sid: x[b] for b, sid in enumerate(sids)})  # mid-stream: every history is full of samples
    t_push = windows_us(lambda i: rs.push({sid: x[b] for b, sid in enumerate(sids)}), ticks)

    book = rs.book
    items = []
    for sid in sids:
        s = book.session(sid)
        items.append((s.slot, chunk, 0, s.parity, s.n_in, s.n_out, book.ready(s.n_in + chunk) - s.n_out, 0))
    O = max(it[6] for it in items)
    table = torch.tensor(items, dtype=torch.int64, device="cuda")
    y = torch.empty(n, O, device="cuda")
    args = (rs.state.data_ptr(), rs.state.numel(), n, sr_in, sr_out, rs.zeros, table.data_ptr(), n, x.data_ptr(), chunk,
            y.data_ptr(), O)
    t_entry = windows_us(lambda i: _lib.check(lib.fsn_resample_stream_push(*args, _lib.stream_ptr())), ticks)

    hist = [torch.randn(book.history, device="cuda") for _ in range(n)]
    due = items[0][6]

    def offline(i):
        for b in range(n):
            out, _ = fsn.resample.resample(torch.cat([hist[b], x[b]]), sr_in, sr_out, design=design)
            out[:due]
    t_off = windows_us(offline, ticks)
    return t_entry, t_push, t_off, book.history, O


def pool_case(fsn, model, n, ticks, rated):
    import torch
    chunk = 768 if rated else 256
    total = WARMUP + 3 * ticks + 2
    torch.manual_seed(n)
    x = 0.1 * torch.randn(n, total * chunk, device="cuda")
    pool = fsn.StreamPool(model, capacity=n, input_sr=48000, output_sr="input") if rated else fsn.StreamPool(model, capacity=n)
    sids = [pool.open() for _ in range(n)]
    for b, sid in enumerate(sids):
        pool.push(sid, x[b, :chunk])
    pool.step()
    frames = []

    def tick(i):
        for b, sid in enumerate(sids):
            pool.push(sid, x[b, (i + 1) * chunk:(i + 2) * chunk])
        frames.append(len(pool.step()))
    t = windows_us(tick, ticks)
    assert all(f == n for f in frames[WARMUP:]), "a tick without a frame for every session"
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--commit", default="")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_resample.md"))
    args = ap.parse_args()
    import torch
    import fullsubnet_amd as fsn
    from fsn_synthetic import make_params
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_resample.py measures on the device: no ROCm device here")
    lines = []
    for sr_in, sr_out, design, chunk in CASES:
        for n in args.sessions:
            (e, e_lo, e_hi), (p, _, _), (o, o_lo, o_hi), history, O = resampler_case(fsn, sr_in, sr_out, design, chunk, n, args.ticks)
            lines.append(f"| {sr_in} -> {sr_out}, {design} | {n} | {chunk} -> {O} | {history} | {e:.1f} | {e_lo:.1f} - {e_hi:.1f} | "
                         f"{p:.1f} | {o:.1f} | {o_lo:.1f} - {o_hi:.1f} | {o / p:.1f} x | {o / e:.1f} x |")
            print(lines[-1], flush=True)
    model = fsn.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                      fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                      sb_model_hidden_size=384, norm_type="cumulative_laplace_norm", num_groups_in_drop_band=1, weight_init=False)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(seed=3).items()})
    model = model.cuda().eval()
    pool_lines = []
    for n in args.sessions:
        (plain, p_lo, p_hi), (rated, r_lo, r_hi) = (pool_case(fsn, model, n, args.ticks, rated) for rated in (False, True))
        pool_lines.append(f"| {n} | {plain / 1e3:.3f} | {p_lo / 1e3:.3f} - {p_hi / 1e3:.3f} | {rated / 1e3:.3f} | {r_lo / 1e3:.3f} - "
                          f"{r_hi / 1e3:.3f} | {(rated - plain) / 1e3:+.3f} | {rated / plain:.3f} x | {rated / 16e3 * 100:.0f} % |")
        print(pool_lines[-1], flush=True)
    if not args.write:
        return
    with open(args.out, "w") as f:
        f.write(f"""# Sample-rate conversion of streams: fsn_resample_stream_push

Written by `tools/bench_stream_resample.py --write` on {datetime.date.today().isoformat()}{f' at commit {args.commit}' if args.commit else ''},
one MI355X, device {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Method: the tool's docstring - device events
around windows of {args.ticks} ticks, median of three, ten warm-up ticks.

## One tick of n sessions (us)

`entry` is the library call alone, `push()` the same through `StreamResampler.push` (book, one torch.stack of the
chunks, the item table's copy), `offline` today's way: per session one `resample.resample` over history + chunk.

| case | sessions | chunk -> outputs | history J - 1 | entry us | windows | push() us | offline, n calls us | windows | offline / push() | offline / entry |
|---|---|---|---|---|---|---|---|---|---|---|
""" + "\n".join(lines) + """

## A StreamPool tick: n push(16 ms) + one step() (ms)

FullSubNet with seeded weights, every session in mid-stream with a frame ready on every tick.

| sessions | at the model's rate ms | windows | 48 kHz in and out ms | windows | difference ms | ratio | share of the 16 ms hop |
|---|---|---|---|---|---|---|---|
""" + "\n".join(pool_lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
