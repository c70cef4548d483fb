"""Time per 10 ms tick of the streaming pool with Improved FullSubNet at 48 kHz, beside what the package offered before it,
on one MI355X:

    python tools/bench_improved_stream_pool.py [--sessions 1 8 32 64] [--commit SHA] [--write]

Shipped 48 kHz configuration (481 bins, 960 / 480, four band sections, hidden 512 / 384, both norms cumulative), k = 1,
every session ready on every tick.  For n sessions a tick is
  pool     n x StreamPool.push(hop) + ONE StreamPool.step() of StreamPool(improved_model)
  (a)      n x StreamingEnhancer(improved_model, batch_size=1).process(hop): what a server had to do before the pool took
           this model
  entry    fsn_improved_stream_pool_step alone on all n slots (the slot list uploaded beforehand)
  floor    fsn_improved_stream_step at B = n: all streams in lockstep; entry - floor is what the gather and the scatter cost
Each figure is the median over REPEATS windows of TICKS ticks, timed with device events around the window after WARMUP ticks.
--write puts the table, and whether the two claims the pool was built on hold in this run, into
profiles/improved_stream_pool.md."""
import argparse
import ctypes
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WARMUP, TICKS, REPEATS, HOP, F = 10, 40, 3, 480, 481
HOP_MS = 10.0


def timed(call):
    """ms per call(i): median over REPEATS event-timed windows of TICKS calls, i counting on from the warm-up."""
    import torch
    i = 0
    for _ in range(WARMUP):
        call(i)
        i += 1
    torch.cuda.synchronize()
    windows = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(TICKS):
            call(i)
            i += 1
        b.record()
        b.synchronize()
        windows.append(a.elapsed_time(b) / TICKS)
    windows.sort()
    return windows[len(windows) // 2]


def measure(n, m):
    import torch
    import fullsubnet_amd
    from fullsubnet_amd import _lib
    from fullsubnet_amd.streaming import StreamingEnhancer
    from fsn_synthetic import make_noisy
    L = _lib.lib()
    dev = torch.device("cuda")
    total = WARMUP + TICKS * REPEATS + 4
    noisy = torch.from_numpy(make_noisy(n, HOP * total, seed=1)).cuda()

    pool = fullsubnet_amd.StreamPool(m, capacity=n)
    sids = [pool.open() for _ in range(n)]
    for b, sid in enumerate(sids):  # the first hop alone completes no frame (frame 0 reflects sample 480)
        pool.push(sid, noisy[b, :HOP])

    def pool_tick(i):
        for b, sid in enumerate(sids):
            pool.push(sid, noisy[b, (i + 1) * HOP:(i + 2) * HOP])
        assert len(pool.step()) == n

    t_pool = timed(pool_tick)

    singles = [StreamingEnhancer(m, batch_size=1) for _ in range(n)]

    def singles_tick(i):
        for b, enh in enumerate(singles):
            enh.process(noisy[b:b + 1, i * HOP:(i + 1) * HOP])

    t_singles = timed(singles_tick)

    # the two entries alone on the same n rows
    cfg_s = m.stream_cfg()
    cfg = ctypes.byref(cfg_s)
    packed = m.stream_packed_weights()
    mag = torch.rand((n, 1, F, 1), device=dev) + 0.1
    mask = torch.empty((n, 2, F, 1), device=dev)
    lock_state = torch.zeros(L.fsn_improved_stream_state_bytes(cfg, n), dtype=torch.uint8, device=dev)

    def floor(i):
        ws = _lib.workspace(L.fsn_improved_stream_workspace_bytes(cfg, n, 1), dev)
        _lib.check(L.fsn_improved_stream_step(cfg, packed.data_ptr(), lock_state.data_ptr(), lock_state.numel(), i, _lib.dev_ptr(mag), n, 1,
                                              _lib.dev_ptr(mask), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))

    t_floor = timed(floor)

    state = torch.zeros(L.fsn_improved_stream_pool_state_bytes(cfg, n), dtype=torch.uint8, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    ws_bytes = L.fsn_improved_stream_pool_workspace_bytes(cfg, n, 1)

    def entry(i):
        ws = _lib.workspace(ws_bytes, dev)
        _lib.check(L.fsn_improved_stream_pool_step(cfg, packed.data_ptr(), state.data_ptr(), state.numel(), n, rows.data_ptr(), n,
                                                   _lib.dev_ptr(mag), 1, _lib.dev_ptr(mask), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))

    t_entry = timed(entry)
    torch.cuda.synchronize()
    assert torch.isfinite(mask).all()
    return {"sessions": n, "pool_ms": t_pool, "singles_ms": t_singles, "entry_ms": t_entry, "floor_ms": t_floor}


def table(rows, commit):
    out = ["# Streaming pool for Improved FullSubNet at 48 kHz: time per 10 ms tick", "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_improved_stream_pool.py`: shipped 48 kHz "
           f"configuration (481 bins, 960 / 480, four band sections, hidden 512 / 384), both norms cumulative, k = 1, every session ready; "
           f"median of {REPEATS} windows of {TICKS} ticks after {WARMUP} warm-up ticks, device events around each window.  A 480-sample "
           f"hop lasts {HOP_MS:g} ms.", "",
           "| sessions | pool tick: n push + step (ms) | per session (ms) | (a) one StreamingEnhancer(batch_size=1) each (ms) | (a) / pool | "
           "fsn_improved_stream_pool_step alone (ms) | floor: fsn_improved_stream_step at B = n (ms) | gather + scatter: entry - floor (ms) | "
           "pool tick, share of the 10 ms hop |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['sessions']} | {r['pool_ms']:.3f} | {r['pool_ms'] / r['sessions']:.3f} | {r['singles_ms']:.3f} | "
                   f"{r['singles_ms'] / r['pool_ms']:.2f} | {r['entry_ms']:.3f} | {r['floor_ms']:.3f} | {r['entry_ms'] - r['floor_ms']:+.3f} | "
                   f"{r['pool_ms'] / HOP_MS * 100:.1f} % |")
    out += ["", "What was to hold, in this run:", ""]
    for r in rows:
        if r["sessions"] >= 8:
            ok = r["pool_ms"] < r["singles_ms"]
            out.append(f"- {r['sessions']} sessions: the pool tick ({r['pool_ms']:.3f} ms) is {'below' if ok else 'NOT below'} n x one enhancer's "
                       f"tick ({r['singles_ms']:.3f} ms = {r['sessions']} x {r['singles_ms'] / r['sessions']:.3f}): {'holds' if ok else 'FAILS'}.")
    big = [r for r in rows if r["sessions"] == 64]
    for r in big:
        ok = r["pool_ms"] < HOP_MS
        out.append(f"- 64 sessions: the pool tick ({r['pool_ms']:.3f} ms) is {'below' if ok else 'NOT below'} the {HOP_MS:g} ms hop: "
                   f"{'holds' if ok else 'FAILS'}.")
    if not big:
        out.append("- 64 sessions were not measured in this run.")
    out.append("")
    one = rows[0]
    if one["sessions"] == 1:
        verdict = "slower than" if one["pool_ms"] > one["singles_ms"] else "not slower than"
        out.append(f"At one session the pool tick ({one['pool_ms']:.3f} ms) is {verdict} one `StreamingEnhancer(batch_size=1).process` "
                   f"({one['singles_ms']:.3f} ms): the pool pays a gather and a scatter and its own frame kernels for a single row.")
    out.append("Columns: the pool tick is n `push(hop)` calls (one `torch.cat` each) plus one `step()`: frame analysis "
               "(`fsn_improved_stream_pool_analysis`), the model step and frame synthesis (`fsn_improved_stream_pool_synthesis`) on the "
               "list of ready slots, around one `torch.stack` of the new hops and one small upload of the slot list.  (a) is what the "
               "parent commit offered a server for this model.  The floor needs all streams in lockstep from the same frame on.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help="write profiles/improved_stream_pool.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "improved_stream_pool.md"))
    args = ap.parse_args()
    from bench_improved_stream import model
    m = model()
    rows = []
    for n in args.sessions:
        rows.append(measure(n, m))
        print(rows[-1], flush=True)
    text = table(rows, args.commit)
    print(text)
    if args.write:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
