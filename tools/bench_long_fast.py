"""Time per frame and peak memory of long recordings on Fast FullSubNet at B = 1 on one MI355X, through the one call
(``Model.enhance``) and through segments with carried state (``Model.enhance_long``), in the form of tools/bench_long.py:

    python tools/bench_long_fast.py [--minutes 2 10] [--segments 256 1024 4096] [--long-minutes 60] [--commit SHA] --write

For every recording length: ``enhance`` and ``enhance_long`` at each ``segment_frames``; for ``--long-minutes`` (beyond the
65 535 frames ``enhance`` takes) ``enhance_long`` alone, at the segment its default workspace limit picks - the only run that
crosses 65 535 frames on the device (no test does).  A run is one child process under a time limit: the call is warmed first
(on the recording itself up to ten minutes, so that the allocator already holds its buffers; on a 20-second recording
beyond), then the whole call is timed on the host clock, a device synchronise at both ends; recordings of up to two minutes
take the median of three calls, longer ones are timed once.  Peak memory is PyTorch's peak allocated bytes over the timed
call, the recording itself ([1, L] floats on the device) included.  The parent never opens the device and stops at the first
child that fails.  ``--write`` puts the table into profiles/long_recording_fast.md."""
import datetime
import sys

import long_bench

HOP, SR = 256, 16000
ONE_CALL_FRAMES = 65535  # fsn_fast_decoder_input's limit
FAST_KW = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257, bottleneck_hidden_size=384,
               bottleneck_num_layers=2, noisy_input_num_neighbors=5, encoder_output_num_neighbors=0,
               norm_type="offline_laplace_norm", weight_init=False)  # BASELINE config 4


def build():
    import torch
    from fullsubnet_amd.fast_fullsubnet import Model
    from fsn_synthetic import make_fast_params
    model = Model(**FAST_KW)
    sd = {k: torch.from_numpy(v) for k, v in make_fast_params(seed=3).items()}
    sd["mel_scale.fb"] = model.mel_scale.fb.clone()
    model.load_state_dict(sd, strict=True)
    return model.cuda().eval()


def used(model, L, k):
    from fullsubnet_amd.fast_long_form import FastLongPlan
    return FastLongPlan(model.stream_cfg(), model.look_ahead, 1, L, k).segment_frames


def table(rows, args):
    out = ["# Fast FullSubNet, long recordings: time per frame and peak memory, B = 1", "",
           f"{datetime.date.today().isoformat()}, commit {args.commit}, one MI355X; `tools/bench_long_fast.py`: the shipped Fast FullSubNet "
           "configuration (BASELINE config 4: shrink 2, look-ahead 2, offline_laplace_norm, fp32), 16 kHz, hop 256.  Host clock "
           "around the whole call with a device synchronise at both ends, after one warm-up call (on the recording itself up to "
           "ten minutes, on a 20-second one beyond); up to two minutes the median of three calls, longer recordings one call.  "
           "Peak memory: PyTorch's peak allocated bytes over the call, the recording on the device included.", "",
           *long_bench.rows_table(rows, "enhance")]
    crossed = [r for r in rows if r["frames"] > ONE_CALL_FRAMES]
    out += ["",
            "`vs one call`: the segment path's time over `enhance` on the same recording (above 1: slower, below 1: faster).  "
            "The segment path makes three passes over the recording (the model divides by two utterance means) where the one "
            "call makes one, and runs every recurrence as per-step launches on carried state (four layers per step and the "
            "bottleneck's per low-rate frame), where the one call runs the encoder pair and the decoder pair as one chain-kernel "
            "launch each: per frame the segment path is the slower one wherever both run, by the same factor at every "
            "`segment_frames`.  What it buys is the recording's length and its memory.  Larger batches, where the one call "
            "moves to persistent kernels the segment path does not use, are not measured here - so `[inferencer] "
            f"segment_frames` stays an explicit key and not a heuristic.  Recordings beyond {ONE_CALL_FRAMES} frames (17.5 "
            "minutes) have no one-call row: `enhance` refuses them.", "",
            (f"The {crossed[-1]['minutes']:g}-minute row ran: {crossed[-1]['frames']} frames, the only run of the project that crosses "
             f"{ONE_CALL_FRAMES} frames of this model on the device (its output was checked for shape and finiteness only)."
             if crossed else
             f"No row beyond {ONE_CALL_FRAMES} frames ran (--long-minutes {' '.join(f'{m:g}' for m in args.long_minutes)}): crossing that count on the device is unmeasured.")]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    sys.exit(long_bench.main(__file__, table, "long_recording_fast.md", [2, 10], [60], sr=SR, hop=HOP, build=build, used=used,
                             one_call=lambda model, x: model.enhance(x),
                             long_call=lambda model, x, k: model.enhance_long(x, segment_frames=k)))
