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
import datetime
import sys

import long_bench

HOP, SR = 480, 48000
STAGES = ("stft", "stats", "fullband", "sections", "istft")


def build():
    import torch
    from fullsubnet_amd.improved_fullsubnet import Model
    from fsn_synthetic import IMPROVED_48K, make_improved_params
    model = Model(**IMPROVED_48K)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_improved_params(IMPROVED_48K, seed=3).items()}, strict=True)
    return model.cuda().eval()


def one_call(model, x):
    import torch
    with torch.no_grad():
        return model(x)[:, 0]


def long_call(model, x, k, on_stage=None):
    from fullsubnet_amd import improved_long_form
    return improved_long_form.enhance_long(model, x, segment_frames=k, on_stage=on_stage)


def used(model, L, k):
    from fullsubnet_amd.improved_long_form import ImprovedLongPlan
    return ImprovedLongPlan(model.stream_cfg(), 960, "offline", 1, L, k).segment_frames


def table(rows, args):
    out = ["# Improved FullSubNet, long recordings: time per frame and peak memory, B = 1", "",
           f"{datetime.date.today().isoformat()}, commit {args.commit}, one MI355X; `tools/bench_long_improved.py`: the shipped Improved "
           "FullSubNet configuration (BASELINE config 5: 48 kHz, n_fft 960 / hop 480, four band sections, offline_laplace_norm in "
           "both places, fp32).  Host clock around the whole call with a device synchronise at both ends, after one warm-up call "
           "(on the recording itself up to ten minutes, on a 20-second one beyond); up to two minutes the median of three calls, "
           "longer recordings one call.  Peak memory: PyTorch's peak allocated bytes over the call, the recording on the device "
           "included.  `model(y)` and `enhance_long` are measured on this commit, on this box, in this run.", "",
           *long_bench.rows_table(rows, "model(y)")]
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


if __name__ == "__main__":
    sys.exit(long_bench.main(__file__, table, "long_recording_improved.md", [0.5, 1], [10, 60], sr=SR, hop=HOP, build=build, used=used,
                             one_call=one_call, long_call=long_call, staged=True))
