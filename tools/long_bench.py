"""What tools/bench_long.py, bench_long_fast.py and bench_long_improved.py share: the command line, the parent's loop over
one child process per run (a time limit each, stop at the first that fails, a ``RESULT`` line of JSON back) and the child's
warm-up and timing of one call.  A tool supplies how its model is built and called, its sample rate and hop, the
``segment_frames`` its plan class settles on, and its ``table()``; the parent never opens the device."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHILD_LIMIT_S = 380


def measure(minutes, segment_frames, sr, hop, build, one_call, long_call, used, staged=False):
    """One run, in the child.  segment_frames: 0 = the one call, -1 = enhance_long at its default workspace limit, else
    enhance_long at that k.  ``build()`` -> the model on the device, ``one_call(model, x)`` / ``long_call(model, x, k)`` ->
    enhanced [1, L], ``used(model, L, k)`` -> the plan's segment_frames.  ``staged``: one more call, synchronised at the end of
    every stage that ``long_call(model, x, k, on_stage)`` reports."""
    import torch
    from fsn_synthetic import make_noisy

    model = build()
    L = int(minutes * 60 * sr)
    # one seeded minute, repeated (an hour of fresh noise is minutes of host time): the model's cost does not depend on the samples
    base = torch.from_numpy(make_noisy(1, min(L, 60 * sr), seed=1))
    noisy = base.repeat(1, -(-L // base.shape[1]))[:, :L].contiguous().cuda()
    k = None if segment_frames < 0 else segment_frames
    run = (lambda x: one_call(model, x)) if segment_frames == 0 else (lambda x: long_call(model, x, k))
    # warm-up: the recording itself up to ten minutes (kernels loaded AND the allocator holding the call's buffers - FullSubNet's
    # one call takes a 100 GB workspace at ten minutes, which costs seconds to allocate the first time), a 20-second one beyond
    run(noisy if minutes <= 10 else noisy[:, :20 * sr])
    torch.cuda.synchronize()
    times = []
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3 if minutes <= 2 else 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(noisy)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    peak = torch.cuda.max_memory_allocated()
    assert out.shape == noisy.shape and bool(torch.isfinite(out).all())
    del out
    row = {"minutes": minutes, "frames": 1 + L // hop, "segment_frames": 0 if segment_frames == 0 else used(model, L, k),
           "default_k": segment_frames < 0, "seconds": sorted(times)[len(times) // 2], "calls": len(times), "peak_bytes": peak}
    if staged:
        row["stages"] = {}
        if segment_frames != 0:
            last = [0.0]

            def mark(stage):
                torch.cuda.synchronize()
                now = time.perf_counter()
                row["stages"][stage] = now - last[0]
                last[0] = now

            torch.cuda.synchronize()
            last[0] = time.perf_counter()
            long_call(model, noisy, k, mark)
    return row


def rows_table(rows, one_call):
    """The table every profile opens with, as lines: one row per run; ``one_call`` names the one-call path."""
    out = ["| recording | frames | path | seconds | us per frame | x real time | vs one call | peak memory (MB) | MB per 1000 frames |",
           "|---|---|---|---|---|---|---|---|---|"]
    ref_of = {r["minutes"]: r["seconds"] for r in rows if r["segment_frames"] == 0}
    for r in rows:
        path = f"`{one_call}` (one call)" if r["segment_frames"] == 0 else (
            f"`enhance_long`, segment_frames {r['segment_frames']}" + (" (default: 4 GiB workspace limit)" if r["default_k"] else ""))
        ref = ref_of.get(r["minutes"])
        rel = "-" if r["segment_frames"] == 0 or ref is None else f"{r['seconds'] / ref:.2f} x"
        out.append(f"| {r['minutes']:g} min | {r['frames']} | {path} | {r['seconds']:.3f} | {r['seconds'] / r['frames'] * 1e6:.1f} | "
                   f"{r['minutes'] * 60 / r['seconds']:.0f} | {rel} | {r['peak_bytes'] / 1e6:.0f} | "
                   f"{r['peak_bytes'] / 1e6 / r['frames'] * 1000:.1f} |")
    return out


def main(tool, table, profile, minutes, long_minutes, **how):
    """The command line of ``tool`` (its ``__file__``).  ``table(rows, args)`` -> the text of profiles/``profile``; ``minutes``
    and ``long_minutes`` are the defaults of the two options, ``how`` the keywords of ``measure``."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=minutes)
    ap.add_argument("--segments", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--long-minutes", type=float, nargs="*", default=long_minutes, help="0 or no value: no such run")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help=f"write profiles/{profile}")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", profile))
    ap.add_argument("--one", type=float, nargs=2, metavar=("MINUTES", "SEGMENT"), help="(child) one run, one JSON line")
    args = ap.parse_args()
    if args.one:
        print("RESULT " + json.dumps(measure(args.one[0], int(args.one[1]), **how)), flush=True)
        return 0
    runs = [(m, k) for m in args.minutes for k in [0] + args.segments] + [(m, -1) for m in args.long_minutes if m > 0]
    rows = []
    for m, k in runs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(tool), "--one", str(m), str(k)], capture_output=True, text=True,
                               timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{m} min / {k}: no result within {CHILD_LIMIT_S} s; stopping", file=sys.stderr)
            return 1
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"{m} min / {k}: child failed ({p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        rows.append(json.loads(res[-1][len("RESULT "):]))
        print(rows[-1], flush=True)
    text = table(rows, args)
    print(text)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0
