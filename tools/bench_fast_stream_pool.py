"""Time per 16 ms tick of the streaming pool with Fast FullSubNet, sessions at different phases of a down-sampling block,
beside what the package offered before it, on one MI355X:

    python tools/bench_fast_stream_pool.py [--sessions 1 8 32 64] [--commit SHA] [--write]

Shipped configuration (shrink 2, look-ahead 2, neighbours (5, 0), bottleneck 384 x 2), k = 1, every session ready; the
sessions' phases are spread evenly over a block: every other session is one step ahead (with one session there is one
phase per tick, and the two alternate).  For n sessions a tick is
  pool        n x StreamPool.push(hop) + ONE StreamPool.step() of StreamPool(fast_model)
  (a)         n x StreamingEnhancer(fast_model, batch_size=1).process(hop): what a server had to do before the pool took the
              fast model
  floor       fsn_fast_stream_step at B = n: all streams in lockstep, the two phases alternate call by call, so the figure is
              their mean.  At a tick of the pool HALF the sessions run the bottleneck, on every tick
  fullsubnet  the same n push + step() tick of StreamPool(fullsubnet_model)
  entry       fsn_fast_stream_pool_step alone on all n slots in the order fast_pool_order gives, both slot orders uploaded
              beforehand; entry - floor is what the order check, the gathers and the scatters cost (and the difference in the
              bottleneck's row count: the pool steps n / 2 x 64 rows every tick, the floor n x 64 every other tick)
Each figure is the median over REPEATS windows of TICKS ticks, timed with device events around the window after WARMUP ticks.
--write puts the table into profiles/fast_stream_pool.md."""
import argparse
import ctypes
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, TICKS, REPEATS, HOP = 10, 40, 3, 256
HOP_MS = 16.0


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


def pool_tick_of(pool, n, noisy):
    """n sessions, every other one a step ahead; tick(i) pushes one hop to each and steps once."""
    sids = [pool.open() for _ in range(n)]
    for b, sid in enumerate(sids):  # the first hop alone completes no frame (frame 0 reflects sample 256)
        pool.push(sid, noisy[b, :HOP])
    ahead = sids[1::2]
    for b, sid in enumerate(sids):
        if sid in ahead:
            pool.push(sid, noisy[b, HOP:2 * HOP])
    if ahead:
        assert sorted(pool.step()) == sorted(ahead)
    pos = {sid: (2 if sid in ahead else 1) * HOP for sid in sids}

    def tick(i):
        for b, sid in enumerate(sids):
            pool.push(sid, noisy[b, pos[sid]:pos[sid] + HOP])
            pos[sid] += HOP
        assert len(pool.step()) == n

    return tick


def measure(n, fast, full):
    import torch
    import fullsubnet_amd
    from fullsubnet_amd import _lib
    from fullsubnet_amd.stream_pool import fast_pool_order
    from fullsubnet_amd.streaming import StreamingEnhancer
    from fsn_synthetic import make_noisy
    L = _lib.lib()
    dev = torch.device("cuda")
    total = WARMUP + TICKS * REPEATS + 4
    noisy = torch.from_numpy(make_noisy(n, HOP * total, seed=1)).cuda()

    t_pool = timed(pool_tick_of(fullsubnet_amd.StreamPool(fast, capacity=n), n, noisy))
    t_full = timed(pool_tick_of(fullsubnet_amd.StreamPool(full, capacity=n), n, noisy))

    singles = [StreamingEnhancer(fast, batch_size=1) for _ in range(n)]

    def singles_tick(i):
        for b, enh in enumerate(singles):
            enh.process(noisy[b:b + 1, i * HOP:(i + 1) * HOP])

    t_singles = timed(singles_tick)

    # the two entries alone on the same n rows
    cfg_s = fast.stream_cfg()
    cfg, la, shrink = ctypes.byref(cfg_s), int(fast.look_ahead), int(fast.shrink_size)
    packed = fast.stream_packed_weights()
    mag = torch.rand((n, 1, 257, 1), device=dev) + 0.1
    crm = torch.empty((n, 2, 257, 1), device=dev)
    lock_state = torch.zeros(L.fsn_fast_stream_state_bytes(cfg, n), dtype=torch.uint8, device=dev)

    def floor(i):
        ws = _lib.workspace(L.fsn_fast_stream_workspace_bytes(cfg, n, 1), dev)
        _lib.check(L.fsn_fast_stream_step(cfg, packed.data_ptr(), lock_state.data_ptr(), lock_state.numel(), i, _lib.dev_ptr(mag), n, 1,
                                          _lib.dev_ptr(crm), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))

    t_floor = timed(floor)

    state = torch.zeros(L.fsn_fast_stream_pool_state_bytes(cfg, la, n), dtype=torch.uint8, device=dev)
    ws_bytes = L.fsn_fast_stream_pool_workspace_bytes(cfg, n, 1)
    counts = [0] * n
    if n > 1:  # every other slot a step ahead
        ahead = list(range(1, n, 2))
        rows = torch.tensor(ahead, dtype=torch.int32, device=dev)
        ws = _lib.workspace(L.fsn_fast_stream_pool_workspace_bytes(cfg, len(ahead), 1), dev)
        _lib.check(L.fsn_fast_stream_pool_step(cfg, la, packed.data_ptr(), state.data_ptr(), state.numel(), n, rows.data_ptr(), len(ahead),
                                               len(ahead), _lib.dev_ptr(mag[:len(ahead)].contiguous()), 1, _lib.dev_ptr(crm), ws.data_ptr(),
                                               ws.numel(), _lib.stream_ptr(dev)))
        for s in ahead:
            counts[s] = 1
    orders = {}  # the slot order of a tick depends on the parity of the tick alone: both are uploaded once

    def entry(i):
        perm, n_long = fast_pool_order(counts, 1, shrink)
        key = tuple(perm)
        if key not in orders:
            orders[key] = torch.tensor(perm, dtype=torch.int32, device=dev)
        ws = _lib.workspace(ws_bytes, dev)
        _lib.check(L.fsn_fast_stream_pool_step(cfg, la, packed.data_ptr(), state.data_ptr(), state.numel(), n, orders[key].data_ptr(), n,
                                               n_long, _lib.dev_ptr(mag), 1, _lib.dev_ptr(crm), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(dev)))
        for s in range(n):
            counts[s] += 1

    t_entry = timed(entry)
    torch.cuda.synchronize()
    assert torch.isfinite(crm).all() and len(orders) <= 2
    return {"sessions": n, "pool_ms": t_pool, "singles_ms": t_singles, "floor_ms": t_floor, "fullsubnet_ms": t_full, "entry_ms": t_entry}


def table(rows, commit):
    out = ["# Streaming pool for Fast FullSubNet: time per 16 ms tick", "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_fast_stream_pool.py`: shipped configuration "
           f"(shrink 2, look-ahead 2, neighbours (5, 0), bottleneck 384 x 2), k = 1, every session ready, every other session one step "
           f"ahead (both phases of a block in every tick); median of {REPEATS} windows of {TICKS} ticks after {WARMUP} warm-up ticks, "
           f"device events around each window.", "",
           "| sessions | pool tick: n push + step (ms) | (a) one StreamingEnhancer(fast, batch_size=1) each (ms) | (a) / pool | "
           "FullSubNet pool tick (ms) | FullSubNet / fast pool | fsn_fast_stream_pool_step alone (ms) | floor: fsn_fast_stream_step at "
           "B = n, mean of both phases (ms) | check + gather + scatter: entry - floor (ms) | pool tick, share of the 16 ms hop |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['sessions']} | {r['pool_ms']:.3f} | {r['singles_ms']:.3f} | {r['singles_ms'] / r['pool_ms']:.2f} | "
                   f"{r['fullsubnet_ms']:.3f} | {r['fullsubnet_ms'] / r['pool_ms']:.2f} | {r['entry_ms']:.3f} | {r['floor_ms']:.3f} | "
                   f"{r['entry_ms'] - r['floor_ms']:+.3f} | {r['pool_ms'] / HOP_MS * 100:.1f} % |")
    out.append("")
    one = rows[0]
    if one["sessions"] == 1:
        verdict = "slower than" if one["pool_ms"] > one["singles_ms"] else "not slower than"
        out.append(f"At one session the pool tick ({one['pool_ms']:.3f} ms) is {verdict} one `StreamingEnhancer(batch_size=1).process` "
                   f"({one['singles_ms']:.3f} ms): the pool pays the order check, two gathers and two scatters and its own frame kernels for "
                   "a single row.")
    out.append("Columns: the pool tick is n `push(hop)` calls (one `torch.cat` each) plus one `step()`: frame analysis, the model step "
               "and frame synthesis on the list of ready slots, which the pool lists long rows first so that the model step moves no "
               "rows.  (a) is what the parent commit offered a server for the fast model.  The floor needs all streams in phase; its "
               "bottleneck runs on n x 64 rows every other call, the pool's on n / 2 x 64 rows every call, so entry - floor holds that "
               "difference beside the order check, the (h, c) gathers and the scatters.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help="write profiles/fast_stream_pool.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast_stream_pool.md"))
    args = ap.parse_args()
    from bench_fast_stream import models
    fast, full = models()
    rows = []
    for n in args.sessions:
        rows.append(measure(n, fast, full))
        print(rows[-1], flush=True)
    text = table(rows, args.commit)
    print(text)
    if args.write:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
