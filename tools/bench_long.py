"""Time per frame and peak memory of long recordings at B = 1 on one MI355X, through the one call (``Model.enhance``) and
through segments with carried state (``Model.enhance_long``):

    python tools/bench_long.py [--minutes 2 10] [--segments 256 1024 4096] [--long-minutes 60] [--commit SHA] --write

For every recording length: ``enhance`` and ``enhance_long`` at each ``segment_frames``; for ``--long-minutes`` (beyond the
100 000 frames ``enhance`` takes) ``enhance_long`` alone, at the segment its default workspace limit picks.  A run is one
child process under a time limit: the call is warmed first (on the recording itself up to ten minutes, so that the
allocator already holds its buffers; on a 20-second recording beyond), then the whole call is timed on the host clock, a
device synchronise at both ends; recordings of up to two minutes take the median of three calls, longer ones are timed once.  Peak memory is PyTorch's peak allocated bytes over the
timed call (every buffer of the path comes from its allocator), the recording itself ([1, L] floats on the device) included.
The parent never opens the device and stops at the first child that fails.  ``--write`` puts the table into
profiles/long_recording.md."""
import datetime
import sys

import long_bench

HOP, SR = 256, 16000


def build():
    import torch
    import fullsubnet_amd
    from fsn_synthetic import make_params
    model = fullsubnet_amd.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0,
                                 sb_num_neighbors=15, fb_output_activate_function="ReLU",
                                 sb_output_activate_function=False, fb_model_hidden_size=512, sb_model_hidden_size=384,
                                 norm_type="offline_laplace_norm", num_groups_in_drop_band=1, weight_init=False)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(seed=3).items()})
    return model.cuda().eval()


def used(model, L, k):
    from fullsubnet_amd.long_form import LongPlan
    return LongPlan(model._cfg, 1, L, k).segment_frames


def table(rows, args):
    out = ["# Long recordings: time per frame and peak memory, B = 1", "",
           f"{datetime.date.today().isoformat()}, commit {args.commit}, one MI355X; `tools/bench_long.py`: the shipped FullSubNet "
           "configuration (offline_laplace_norm, fp32), 16 kHz, hop 256.  Host clock around the whole call with a device "
           "synchronise at both ends, after one warm-up call (on the recording itself up to ten minutes, on a 20-second one "
           "beyond); up to two minutes the median of three calls, longer recordings one call.  Peak memory: PyTorch's peak allocated bytes over the call, the recording on the device "
           "included.", "",
           *long_bench.rows_table(rows, "enhance")]
    out += ["",
            "`vs one call`: the segment path's time over `enhance` on the same recording (above 1: slower, below 1: faster).  "
            "This table is B = 1 only: there both paths run the recurrences as per-step launches; at larger batches the one "
            "call moves to persistent kernels the segment path does not use, which is not measured here - so "
            "`[inferencer] segment_frames` stays an explicit key and not a heuristic.  Recordings beyond 26.7 minutes have no "
            "one-call row: `enhance` refuses them."]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    sys.exit(long_bench.main(__file__, table, "long_recording.md", [2, 10], [60], sr=SR, hop=HOP, build=build, used=used,
                             one_call=lambda model, x: model.enhance(x),
                             long_call=lambda model, x, k: model.enhance_long(x, segment_frames=k)))
