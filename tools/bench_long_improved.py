"""Time per frame and peak memory of long recordings on Improved FullSubNet (48 kHz, BASELINE config 5) at B = 1 on one
MI355X, through the one call (``model(y)``) and through segments with carried state (``Model.enhance_long``), in the form of
tools/bench_long_fast.py:

    python tools/bench_long_improved.py [--minutes 0.5 1] [--segments 256 1024 4096] [--long-minutes 10 60] [--commit SHA] --write

For every recording length of ``--minutes``: ``model(y)`` and ``enhance_long`` at each ``segment_frames``; for every length of
``--long-minutes`` ``enhance_long`` alone, at the segment its default workspace limit picks.  A run is one child process under
a time limit: the call is warmed first (on the recording itself up to ten minutes, so that the allocator already holds its
buffers; on a 20-second recording beyond), then the whole call is timed on the host clock, a device synchronise at both ends;
recordings of up to two minutes take the median of three calls, longer ones are timed once.  The split over the stages
(transforms, the three passes) comes from one more call with a device synchronise at the end of every stage
(``improved_long_form.enhance_long(..., on_stage=...)``).  Peak memory is PyTorch's peak allocated bytes over the timed
call, the recording itself ([1, L] floats on the device) included.  The parent never opens the device and stops at the first child that fails: a
``model(y)`` that does not fit is a failed child, so ``--minutes`` names only lengths at which both paths run.  ``--write``
puts the table into profiles/long_recording_improved.md."""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOP, SR = 480, 48000
CHILD_LIMIT_S = 380
STAGES = ("stft", "stats", "fullband", "sections", "istft")


def measure(minutes, segment_frames):
    """segment_frames: 0 = model(y), -1 = enhance_long at its default workspace limit, else enhance_long at that k."""
    import torch
    from fullsubnet_amd import improved_long_form
    from fullsubnet_amd.improved_fullsubnet import Model
    from fsn_synthetic import IMPROVED_48K, make_improved_params, make_noisy

    model = Model(**IMPROVED_48K)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_improved_params(IMPROVED_48K, seed=3).items()}, strict=True)
    model = model.cuda().eval()
    L = int(minutes * 60 * SR)
    # one seeded minute, repeated (an hour of fresh noise is minutes of host time): the model's cost does not depend on the samples
    base = torch.from_numpy(make_noisy(1, min(L, 60 * SR), seed=1))
    noisy = base.repeat(1, -(-L // base.shape[1]))[:, :L].contiguous().cuda()
    k = None if segment_frames < 0 else segment_frames

    def run(x, on_stage=None):
        with torch.no_grad():
            if segment_frames == 0:
                return model(x)[:, 0]
            return improved_long_form.enhance_long(model, x, segment_frames=k, on_stage=on_stage)

    run(noisy if minutes <= 10 else noisy[:, :20 * SR])  # warm-up: kernels loaded, the allocator holding the call's buffers
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
    stages = {}
    if segment_frames != 0:  # one more call, synchronised at every stage's end
        last = [0.0]

        def mark(stage):
            torch.cuda.synchronize()
            now = time.perf_counter()
            stages[stage] = now - last[0]
            last[0] = now

        torch.cuda.synchronize()
        last[0] = time.perf_counter()
        run(noisy, on_stage=mark)
    frames = 1 + L // HOP
    used = 0 if segment_frames == 0 else improved_long_form.ImprovedLongPlan(model.stream_cfg(), 960, "offline", 1, L, k).segment_frames
    return {"minutes": minutes, "frames": frames, "segment_frames": used, "default_k": segment_frames < 0,
            "seconds": sorted(times)[len(times) // 2], "calls": len(times), "peak_bytes": peak, "stages": stages}


def table(rows, commit):
    out = ["# Improved FullSubNet, long recordings: time per frame and peak memory, B = 1", "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_long_improved.py`: the shipped Improved "
           "FullSubNet configuration (BASELINE config 5: 48 kHz, n_fft 960 / hop 480, four band sections, offline_laplace_norm in "
           "both places, fp32).  Host clock around the whole call with a device synchronise at both ends, after one warm-up call "
           "(on the recording itself up to ten minutes, on a 20-second one beyond); up to two minutes the median of three calls, "
           "longer recordings one call.  Peak memory: PyTorch's peak allocated bytes over the call, the recording on the device "
           "included.  `model(y)` and `enhance_long` are measured on this commit, on this box, in this run.", "",
           "| recording | frames | path | seconds | us per frame | x real time | vs one call | peak memory (MB) | MB per 1000 frames |",
           "|---|---|---|---|---|---|---|---|---|"]
    one_call = {r["minutes"]: r["seconds"] for r in rows if r["segment_frames"] == 0}
    for r in rows:
        path = "`model(y)` (one call)" if r["segment_frames"] == 0 else (
            f"`enhance_long`, segment_frames {r['segment_frames']}" + (" (default: 4 GiB workspace limit)" if r["default_k"] else ""))
        ref = one_call.get(r["minutes"])
        rel = "-" if r["segment_frames"] == 0 or ref is None else f"{r['seconds'] / ref:.2f} x"
        out.append(f"| {r['minutes']:g} min | {r['frames']} | {path} | {r['seconds']:.3f} | {r['seconds'] / r['frames'] * 1e6:.1f} | "
                   f"{r['minutes'] * 60 / r['seconds']:.0f} | {rel} | {r['peak_bytes'] / 1e6:.0f} | "
                   f"{r['peak_bytes'] / 1e6 / r['frames'] * 1000:.1f} |")
    out += ["", "## The split over the stages of `enhance_long`", "",
            "One more call per row with a device synchronise at the end of every stage; us per frame.  `stats`, `fullband` and "
            "`sections` are the three passes (fsn_improved_segment_stats / _fullband / _sections over all segments), `stft` and "
            "`istft` the slabbed transforms with the mask products.", "",
            "| recording | segment_frames | " + " | ".join(STAGES) + " | sum |", "|---|---|" + "---|" * (len(STAGES) + 1)]
    for r in rows:
        if r["stages"]:
            us = [r["stages"].get(s, 0.0) / r["frames"] * 1e6 for s in STAGES]
            out.append(f"| {r['minutes']:g} min | {r['segment_frames']} | " + " | ".join(f"{u:.1f}" for u in us) + f" | {sum(us):.1f} |")
    out += ["",
            "`vs one call`: the segment path's time over `model(y)` on the same recording (above 1: slower, below 1: faster).  The "
            "segment path makes three passes over the recording (two utterance means, each needed before the next stage starts) "
            "and runs every recurrence as per-step launches of the stateful layer entry on carried state - per frame two for the "
            "full-band block and two for each of the four sections - where the one call runs the full-band pair as one chain "
            "kernel and the sections on persistent or chain kernels.  What it buys is the recording's length and its memory: the "
            "one call keeps gate planes of hidden-state width for every frame, the segment path planes of F floats.  Recordings "
            "with no one-call row were not tried on `model(y)`."]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[0.5, 1])
    ap.add_argument("--segments", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--long-minutes", type=float, nargs="*", default=[10, 60])
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help="write profiles/long_recording_improved.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_recording_improved.md"))
    ap.add_argument("--one", type=float, nargs=2, metavar=("MINUTES", "SEGMENT"), help="(child) one run, one JSON line")
    args = ap.parse_args()
    if args.one:
        print("RESULT " + json.dumps(measure(args.one[0], int(args.one[1]))), flush=True)
        return 0
    runs = [(m, k) for m in args.minutes for k in [0] + args.segments] + [(m, -1) for m in args.long_minutes]
    rows = []
    for m, k in runs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(m), str(k)], capture_output=True,
                               text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{m} min / {k}: no result within {CHILD_LIMIT_S} s; stopping", file=sys.stderr)
            return 1
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"{m} min / {k}: child failed ({p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        rows.append(json.loads(res[-1][len("RESULT "):]))
        print(rows[-1], flush=True)
    text = table(rows, args.commit)
    print(text)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
