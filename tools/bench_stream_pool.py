"""Time per 16 ms tick of the streaming pool in steady state (one frame per session per tick, every session ready) beside
what the package offered before it, on one MI355X:

    python tools/bench_stream_pool.py [--sessions 1 8 32 64] [--commit SHA] [--out profiles/stream_pool.md]

For n sessions a tick is
  pool      n x StreamPool.push(hop) + ONE StreamPool.step(); step() is also timed alone, and the model-step entry alone
            beside fsn_fullsubnet_stream_step at B = n (what the (h, c) gather and scatter cost)
  (a)       n x StreamingEnhancer(batch_size=1).process(hop): one object per call, what a server had to do so far
  (b)       ONE lockstep StreamingEnhancer(batch_size=n).process(hops): the floor without slot indirection (only usable
            when all streams start together and stay phase-aligned)
Each figure is the median over REPEATS timed blocks of TICKS ticks (one synchronize per block) after WARMUP ticks.  Every
session count runs in a child process of its own under a time limit; the parent never opens the device and stops at the
first child that fails.  The table goes to stdout and to --out."""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, TICKS, REPEATS, HOP = 10, 10, 7, 256
CHILD_LIMIT_S = 240


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def timed(tick, sync):
    """ms per tick: median over REPEATS blocks of TICKS calls of tick(i), i counting on from the warm-up."""
    i = 0
    for _ in range(WARMUP):
        tick(i)
        i += 1
    sync()
    blocks = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(TICKS):
            tick(i)
            i += 1
        sync()
        blocks.append((time.perf_counter() - t0) / TICKS * 1e3)
    return median(blocks)


def measure(n):
    import torch
    import fullsubnet_amd
    from fullsubnet_amd.streaming import StreamingEnhancer
    from fsn_synthetic import make_noisy, make_params

    model = fullsubnet_amd.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0,
                                 sb_num_neighbors=15, fb_output_activate_function="ReLU",
                                 sb_output_activate_function=False, fb_model_hidden_size=512, sb_model_hidden_size=384,
                                 norm_type="cumulative_laplace_norm", num_groups_in_drop_band=1, weight_init=False)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(seed=3).items()})
    model = model.cuda().eval()
    total = WARMUP + TICKS * REPEATS + 2
    noisy = torch.from_numpy(make_noisy(n, HOP * total, seed=1)).cuda()
    hop = lambda i: noisy[:, i * HOP:(i + 1) * HOP]  # noqa: E731
    sync = torch.cuda.synchronize

    pool = fullsubnet_amd.StreamPool(model, capacity=n)
    sids = [pool.open() for _ in range(n)]
    for b, sid in enumerate(sids):  # the first hop alone completes no frame (frame 0 reflects sample 256)
        pool.push(sid, noisy[b, :HOP])

    def pool_tick(i):
        h = hop(i + 1)
        for b, sid in enumerate(sids):
            pool.push(sid, h[b])
        out = pool.step()
        assert len(out) == n

    t_pool = timed(pool_tick, sync)

    # step() alone: a block's hops are pushed (one push per session) before its clock starts
    more = torch.from_numpy(make_noisy(n, HOP * TICKS * (REPEATS + 1), seed=2)).cuda()
    blocks = []
    for r in range(REPEATS + 1):  # the first block is the warm-up
        for b, sid in enumerate(sids):
            pool.push(sid, more[b, r * TICKS * HOP:(r + 1) * TICKS * HOP])
        sync()
        t0 = time.perf_counter()
        for _ in range(TICKS):
            assert len(pool.step()) == n
        sync()
        blocks.append((time.perf_counter() - t0) / TICKS * 1e3)
    t_step = median(blocks[1:])

    # the model-step entry alone on all n slots beside the lockstep entry at B = n: what gather / scatter cost
    import ctypes
    from fullsubnet_amd import _lib
    L = _lib.lib()
    mag = torch.rand((n, 1, 257, 1), device="cuda") + 0.1
    slots = list(range(n))
    slots_dev = torch.tensor(slots, dtype=torch.int32, device="cuda")
    t_entry_pool = timed(lambda i: pool.model_step(slots, mag, slots_dev=slots_dev), sync)
    cfg = ctypes.byref(model._cfg)
    state = torch.zeros(L.fsn_fullsubnet_stream_state_bytes(cfg, n), dtype=torch.uint8, device="cuda")
    crm = torch.empty((n, 2, 257, 1), device="cuda")
    packed = model.packed_weights()

    def lock_entry(i):
        ws = _lib.workspace(L.fsn_fullsubnet_stream_workspace_bytes(cfg, n, 1), mag.device)
        _lib.check(L.fsn_fullsubnet_stream_step(cfg, packed.data_ptr(), state.data_ptr(), state.numel(), i, _lib.dev_ptr(mag), n,
                                                1, _lib.dev_ptr(crm), ws.data_ptr(), ws.numel(), _lib.stream_ptr(mag.device)))

    t_entry_lock = timed(lock_entry, sync)

    singles = [StreamingEnhancer(model, batch_size=1) for _ in range(n)]

    def singles_tick(i):
        h = hop(i)
        for b, enh in enumerate(singles):
            enh.process(h[b:b + 1])

    t_singles = timed(singles_tick, sync)
    lock = StreamingEnhancer(model, batch_size=n)
    t_lock = timed(lambda i: lock.process(hop(i)), sync)
    return {"sessions": n, "pool_ms": t_pool, "step_ms": t_step, "singles_ms": t_singles, "lockstep_ms": t_lock,
            "entry_pool_ms": t_entry_pool, "entry_lock_ms": t_entry_lock}


def table(rows, commit):
    out = ["# Streaming pool: time per 16 ms tick", "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_stream_pool.py`: k = 1, every session "
           f"ready, median of {REPEATS} blocks of {TICKS} ticks after {WARMUP} warm-up ticks, one synchronize per block.", "",
           "| sessions | pool tick: n push + step (ms) | of which step() (ms) | (a) one StreamingEnhancer(batch_size=1) each (ms) | "
           "(a) / pool | (b) lockstep batch (ms) | pool / (b) | model step: pool entry (ms) | lockstep entry (ms) | "
           "gather + scatter, share of the lockstep entry | pool tick, share of the 16 ms hop |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['sessions']} | {r['pool_ms']:.3f} | {r['step_ms']:.3f} | {r['singles_ms']:.3f} | "
                   f"{r['singles_ms'] / r['pool_ms']:.2f} | {r['lockstep_ms']:.3f} | {r['pool_ms'] / r['lockstep_ms']:.2f} | "
                   f"{r['entry_pool_ms']:.3f} | {r['entry_lock_ms']:.3f} | "
                   f"{(r['entry_pool_ms'] - r['entry_lock_ms']) / r['entry_lock_ms'] * 100:+.0f} % | {r['pool_ms'] / 16 * 100:.0f} % |")
    out.append("")
    fit = [r for r in rows if r["pool_ms"] <= 16.0]
    if fit:
        last = fit[-1]
        line = f"Largest measured pool that keeps up with real time (a tick under 16 ms): {last['sessions']} sessions."
        if last is rows[-1] and len(rows) >= 2:
            prev = rows[-2]
            slope = (last["pool_ms"] - prev["pool_ms"]) / (last["sessions"] - prev["sessions"])
            if slope > 0:
                line += (f"  Extrapolated along the last two points ({slope * 1e3:.0f} us per further session): about "
                         f"{int(last['sessions'] + (16.0 - last['pool_ms']) / slope)} sessions fit in a hop (not measured).")
        out.append(line)
    else:
        out.append("No measured pool size keeps up with real time (every tick took more than 16 ms).")
    out.append("Columns: the pool tick is n `push(hop)` calls (one `torch.cat` each) plus one `step()`; `step()` alone is timed with "
               "a block's hops pushed before the clock starts, so the difference is what the per-session pushes cost.  (b) runs "
               "`torch.stft` / `istft` on three-frame segments around the lockstep entry, the pool its own frame kernels, so pool / (b) "
               "compares two whole paths.  The gather + scatter share compares the two model-step ENTRIES alone on the same n rows: "
               "`fsn_fullsubnet_stream_pool_step` on all n slots against `fsn_fullsubnet_stream_step` at B = n, k = 1.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_pool.md"))
    ap.add_argument("--one", type=int, help="(child) measure this session count and print one JSON line")
    args = ap.parse_args()
    if args.one:
        print("RESULT " + json.dumps(measure(args.one)), flush=True)
        return 0
    rows = []
    for n in args.sessions:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n)], capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{n} sessions: no result within {CHILD_LIMIT_S} s; stopping", file=sys.stderr)
            return 1
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"{n} sessions: child failed ({p.returncode}); stopping\n{p.stdout}\n{p.stderr}", file=sys.stderr)
            return 1
        rows.append(json.loads(res[-1][len("RESULT "):]))
        print(rows[-1], flush=True)
    text = table(rows, args.commit)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
