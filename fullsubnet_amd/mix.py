"""Training pairs mixed on the device: the loader side of fsn_mix_pairs (include/fsn_hip.h).

The reference's training set (recipes/dns_interspeech_2020/dataset_train.py) crops, concatenates, convolves and levels
every item on the host.  Here the source audio sits in device memory (`MixBank`), the host only DRAWS - `draw_item` issues
the random calls of ``Dataset.__getitem__`` in the reference's order and returns a descriptor - and one library call per
batch (`mix_batch`) does the arithmetic.  `MixLoader` is the iterable a `Trainer` takes as ``train_dataloader``.
"""
import ctypes
import math
import random
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib

SLAB_FORMATS = {"f32": 0, "i16": 1}  # FSN_SLAB_F32 / FSN_SLAB_I16
MAX_L = 131072                       # FSN_MIX_MAX_L

# fsn_mix_item / fsn_mix_seg of include/fsn_hip.h (natural C alignment)
ITEM_DTYPE = np.dtype([("clean_off", np.int64), ("clean_len", np.int32), ("seg_begin", np.int32), ("seg_count", np.int32),
                       ("rir_off", np.int64), ("rir_len", np.int32), ("snr_db", np.float32), ("target_dbfs", np.float32),
                       ("noisy_target_dbfs", np.float32)], align=True)
SEG_DTYPE = np.dtype([("src_off", np.int64), ("dst_off", np.int32), ("len", np.int32)], align=True)
# fsn_mix_target: the descriptor of a row's dereverberation target (fsn_rir_shorten / fsn_mix_pairs_target)
TARGET_DTYPE = np.dtype([("q", np.float64), ("after_max", np.int32), ("mode", np.int32)], align=True)
assert ITEM_DTYPE.itemsize == 48 and SEG_DTYPE.itemsize == 16 and TARGET_DTYPE.itemsize == 16
TARGET_MODES = {"reverberant": 0, "shortened": 1, "early": 2}


def shortening_q(original_T60, target_T60, sr):
    """The window's decay per sample in decades, as audio_zen/acoustics/rvb.py forms it (the same expression in the same
    order: the same double)."""
    return 3 / (target_T60 * sr) - 3 / (original_T60 * sr)


def target_of(cfg, original_T60=None):
    """(mode, q, after_max) of a reverberant row under `cfg`.  A response that already decays as fast as the target
    (original_T60 <= target_T60: q <= 0 would LENGTHEN its tail) keeps its reverberant row, mode 0."""
    mode = TARGET_MODES[cfg.target]
    if mode == 0:
        return 0, 0.0, 0
    after_max = int(math.floor(cfg.time_after_max * cfg.sr))
    if mode == 2:
        return 2, 0.0, after_max
    if original_T60 is None:
        raise ValueError('target = "shortened" needs the T60 of every response: MixBank(..., rir_t60=...)')
    if not original_T60 > cfg.target_T60:
        return 0, 0.0, 0
    return 1, shortening_q(float(original_T60), cfg.target_T60, cfg.sr), after_max


@dataclass
class MixConfig:
    """The mixing arguments of the reference's Dataset (train.toml [train_dataset.args])."""
    sr: int = 16000
    sub_sample_length: float = 3.072
    silence_length: float = 0.2
    snr_range: tuple = (-5, 20)
    reverb_proportion: float = 0.75
    target_dB_FS: int = -25
    target_dB_FS_floating_value: int = 10
    snr_list: list = field(default=None)
    target: str = "reverberant"    # the second tensor of a pair: the reverberant clean row (the reference's), or the clean
    target_T60: float = 0.15       # row under the response "shortened" to this T60 / cut to its "early" part,
    time_after_max: float = 0.002  # both from this long behind the response's peak on (rvb.py's defaults)

    def __post_init__(self):
        if self.target not in TARGET_MODES:
            raise ValueError(f'target = {self.target!r}: "reverberant", "shortened" or "early"')
        if not (self.target_T60 > 0 and self.time_after_max >= 0):
            raise ValueError("target_T60 > 0 and time_after_max >= 0 are required")
        if self.snr_list is None:  # base_dataset.py:_parse_snr_range
            low, high = self.snr_range
            assert low <= high, "The low SNR should not larger than high SNR."
            self.snr_list = list(range(low, high + 1))
        assert 0 <= self.reverb_proportion <= 1, "The 'reverb_proportion' should be in [0, 1]."

    @property
    def samples(self):
        return int(self.sub_sample_length * self.sr)


@dataclass
class MixItem:
    """One row's draws.  Indices refer to the bank's lists; the noise row is silence except for `segments`,
    (noise index, first sample in that file, first sample of the row, samples)."""
    clean_index: int
    clean_start: int
    clean_len: int
    segments: list
    snr: int
    rir_index: int  # -1: no reverb
    rir_row: int
    noisy_target_dB_FS: int
    target_dB_FS: int
    target_mode: int = 0       # fsn_mix_target of the row (target_of): 0 the reverberant row, 1 shortened, 2 early
    target_q: float = 0.0
    target_after_max: int = 0


def _to_slab(waves, fmt):
    """(slab array, offsets, lengths) of a list of 1-D waveforms."""
    lens = np.asarray([int(np.shape(w)[-1]) for w in waves], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(waves) else np.zeros(0, np.int64)
    parts = []
    for w in waves:
        w = np.asarray(w)
        if w.ndim != 1:
            raise ValueError(f"a bank holds 1-D waveforms (got shape {w.shape})")
        if fmt == "f32":
            if w.dtype == np.int16:
                w = w.astype(np.float32) / np.float32(32768.0)
            parts.append(np.ascontiguousarray(w, dtype=np.float32))
        else:
            if w.dtype != np.int16:
                q = np.rint(np.asarray(w, dtype=np.float64) * 32768.0)
                if q.size and (np.abs(q / 32768.0 - w).max() > 0 or q.min() < -32768 or q.max() > 32767):
                    raise ValueError('fmt="i16" takes 16-bit PCM: int16 arrays, or floats that are exactly v / 32768')
                w = q.astype(np.int16)
            parts.append(np.ascontiguousarray(w))
    dt = np.float32 if fmt == "f32" else np.int16
    slab = np.concatenate(parts) if parts else np.zeros(0, dt)
    if slab.size == 0:
        slab = np.zeros(1, dt)  # a valid device pointer for an empty list
    return slab, offs, lens


class MixBank:
    """Clean speech, noise and room impulse responses as three device slabs plus host-side offset / length tables.
    `clean`, `noise`: lists of 1-D waveforms; `rir`: 1-D responses or 2-D arrays whose rows are responses (one is drawn per
    item).  fmt "f32" keeps fp32 samples; "i16" keeps 16-bit PCM (int16 arrays, read as v / 32768 - what a 16-bit wav loads
    as) at half the memory.  rir_t60: the reverberation time of every response in seconds (a number per 1-D response, a
    number or one per row for a 2-D one) - what a "shortened" target is measured against; it is given, never estimated."""

    def __init__(self, clean, noise, rir, device, fmt="f32", rir_t60=None):
        if fmt not in SLAB_FORMATS:
            raise ValueError(f'fmt = {fmt!r}: "f32" or "i16"')
        self.fmt, self.slab_format = fmt, SLAB_FORMATS[fmt]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.FsnError(f"a MixBank lives on a ROCm device (got {self.device}); there is no CPU path")
        if not len(clean) or not len(noise):
            raise ValueError("a bank needs at least one clean and one noise waveform")
        rir_rows, self.rir_first_row, self.rir_rows, self.rir_2d = [], [], [], []
        self.rir_t60 = None if rir_t60 is None else rir_t60_rows(rir, rir_t60)
        for r in rir:
            r = np.asarray(r)
            self.rir_2d.append(r.ndim > 1)  # the reference draws a row of every 2-D response, a single row included
            rows = [r] if r.ndim == 1 else list(r.reshape(-1, r.shape[-1]))
            self.rir_first_row.append(len(rir_rows))
            self.rir_rows.append(len(rows))
            rir_rows += rows
        self.slabs = {}
        for name, waves in (("clean", clean), ("noise", noise), ("rir", rir_rows)):
            slab, offs, lens = _to_slab(waves, fmt)
            self.slabs[name] = torch.from_numpy(slab).to(self.device)
            setattr(self, name + "_off", offs)
            setattr(self, name + "_len", lens)

    def __len__(self):
        return len(self.clean_len)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in self.slabs.values())


def rir_t60_rows(rir, rir_t60):
    """rir_t60 as one float array per response, a value per row."""
    if len(rir_t60) != len(rir):
        raise ValueError(f"rir_t60 has {len(rir_t60)} entries for {len(rir)} responses")
    out = []
    for i, (r, t) in enumerate(zip(rir, rir_t60)):
        rows = 1 if np.ndim(r) == 1 else int(np.prod(np.shape(r)[:-1]))
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if t.size == 1:
            t = np.repeat(t, rows)
        if t.size != rows or not (t > 0).all():
            raise ValueError(f"rir_t60[{i}]: one positive T60, or one per row ({rows}), is needed")
        out.append(t)
    return out


def draw_item(index, bank, cfg, py_random=random, np_random=np.random):
    """The draws of ``Dataset.__getitem__(index)`` (dataset_train.py:197-224) in the reference's order - with the same
    seeds and the same preloaded lists it picks what the reference picks:
    crop start (feature.py:subsample), the noise files with their silences and the crop of the concatenation
    (_select_noise_y), the SNR, the reverb coin, the response, its row when it is 2-D, the level of the mixture.
    cfg.target adds no draw: the row's target descriptor follows from the response that was drawn."""
    L = cfg.samples
    n = int(bank.clean_len[index])
    start = int(np_random.randint(n - L)) if n > L else 0
    clean_len = min(n, L)
    # _select_noise_y: files and silences until the target length is covered
    pieces, total, remaining = [], 0, L
    silence = int(cfg.sr * cfg.silence_length)
    while remaining > 0:
        k = py_random.choice(range(len(bank.noise_len)))
        ln = int(bank.noise_len[k])
        pieces.append((k, total, ln))
        total += ln
        remaining -= ln
        if remaining > 0:
            sl = min(remaining, silence)
            total += sl
            remaining -= sl
    w0 = int(np_random.randint(total - L)) if total > L else 0
    segments = []
    for k, p0, ln in pieces:
        lo, hi = max(p0, w0), min(p0 + ln, w0 + L)
        if hi > lo:
            segments.append((k, lo - p0, lo - w0, hi - lo))
    snr = py_random.choice(cfg.snr_list)
    use_reverb = bool(np_random.random(1) < cfg.reverb_proportion)
    rir_index, rir_row = -1, 0
    if use_reverb:
        if not len(bank.rir_rows):
            raise ValueError("reverb_proportion > 0 needs room impulse responses in the bank")
        rir_index = py_random.choice(range(len(bank.rir_rows)))
        if bank.rir_2d[rir_index]:
            rir_row = int(np_random.randint(0, bank.rir_rows[rir_index]))
    level = int(np_random.randint(cfg.target_dB_FS - cfg.target_dB_FS_floating_value,
                                  cfg.target_dB_FS + cfg.target_dB_FS_floating_value))
    mode, q, after_max = 0, 0.0, 0
    if rir_index >= 0 and cfg.target != "reverberant":
        t60 = getattr(bank, "rir_t60", None)
        mode, q, after_max = target_of(cfg, None if t60 is None else float(t60[rir_index][rir_row]))
    return MixItem(index, start, clean_len, segments, int(snr), rir_index, rir_row, level, int(cfg.target_dB_FS), mode, q,
                   after_max)


def pack_items(bank, items, L):
    """(item table, segment table, longest response) of a batch as the structured arrays fsn_mix_pairs reads.  Everything
    the device cannot check is checked here: every crop, segment and response lies inside its waveform and the row."""
    if not 1 <= L <= MAX_L:
        raise _lib.FsnError(f"L = {L}: 1 <= L <= {MAX_L}")
    tab = np.zeros(len(items), ITEM_DTYPE)
    segs, longest = [], 0
    for b, it in enumerate(items):
        n = int(bank.clean_len[it.clean_index])
        if not (0 <= it.clean_start and 0 <= it.clean_len <= L and it.clean_start + it.clean_len <= n):
            raise _lib.FsnError(f"item {b}: clean crop [{it.clean_start}, +{it.clean_len}) outside waveform {it.clean_index} "
                                f"of {n} samples or longer than L = {L}")
        tab[b]["clean_off"] = bank.clean_off[it.clean_index] + it.clean_start
        tab[b]["clean_len"] = it.clean_len
        tab[b]["seg_begin"], tab[b]["seg_count"] = len(segs), len(it.segments)
        for k, src, dst, ln in it.segments:
            if not (0 <= src and ln >= 0 and src + ln <= int(bank.noise_len[k]) and 0 <= dst and dst + ln <= L):
                raise _lib.FsnError(f"item {b}: noise segment ({k}, {src}, {dst}, {ln}) outside its waveform or the row")
            segs.append((bank.noise_off[k] + src, dst, ln))
        if it.rir_index >= 0:
            if not 0 <= it.rir_row < bank.rir_rows[it.rir_index]:
                raise _lib.FsnError(f"item {b}: response {it.rir_index} has no row {it.rir_row}")
            row = bank.rir_first_row[it.rir_index] + it.rir_row
            tab[b]["rir_off"], tab[b]["rir_len"] = bank.rir_off[row], bank.rir_len[row]
            longest = max(longest, int(bank.rir_len[row]))
        tab[b]["snr_db"], tab[b]["target_dbfs"] = it.snr, it.target_dB_FS
        tab[b]["noisy_target_dbfs"] = it.noisy_target_dB_FS
    seg_tab = np.zeros(max(len(segs), 1), SEG_DTYPE)
    for i, s in enumerate(segs):
        seg_tab[i] = s
    return tab, seg_tab, len(segs), longest


def pack_targets(items):
    """The fsn_mix_target table of a batch.  A row without a response, and a shortened one whose q <= 0 (it would lengthen
    the tail), keep their reverberant row: mode 0.  A mode the device does not know is refused here - its table is in
    device memory, where the library's host code cannot look."""
    tab = np.zeros(len(items), TARGET_DTYPE)
    for b, it in enumerate(items):
        if it.target_mode not in (0, 1, 2):
            raise _lib.FsnError(f"item {b}: target mode {it.target_mode} is outside 0 - 2 (reverberant, shortened, early)")
        if it.target_after_max < 0:
            raise _lib.FsnError(f"item {b}: target_after_max = {it.target_after_max}")
        keep = it.rir_index < 0 or (it.target_mode == 1 and not it.target_q > 0)
        if it.target_mode != 0 and not keep:
            tab[b] = (it.target_q if it.target_mode == 1 else 0.0, it.target_after_max, it.target_mode)
    return tab


def mix_batch(bank, items, L, out=None, eps=1e-6, max_rir_len=None, target=None):
    """One fsn_mix_pairs call: (noisy, clean) fp32 device tensors [B, L] of the descriptors `items` (MixItem list).  The
    descriptors go up in ONE non-blocking copy from pinned memory; the call is enqueued on the current stream and nothing
    synchronises.  out: a (noisy, clean) pair to write into.  max_rir_len: size the transform for this response length
    instead of the batch's longest (a fixed plan, e.g. for bit-identical repeats across batches).
    target: True returns (noisy, target) through fsn_mix_pairs_target, the clean rows under their shortened / early
    responses (MixItem.target_*); False is the call above, whatever the items say; None: True if any item asks for it."""
    if target is None:
        target = any(it.target_mode != 0 for it in items)
    if target:
        return _mix_batch_target(bank, items, L, out, eps, max_rir_len)
    tab, seg_tab, n_segs, longest = pack_items(bank, items, L)
    B = len(items)
    if B < 1:
        raise _lib.FsnError("an empty batch")
    longest = longest if max_rir_len is None else max(longest, int(max_rir_len))
    dev = bank.device
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(B, L, dtype=torch.float32, device=dev), torch.empty(B, L, dtype=torch.float32, device=dev))
        noisy, clean = out
        if tuple(noisy.shape) != (B, L) or tuple(clean.shape) != (B, L):
            raise _lib.FsnError(f"out: two [{B}, {L}] tensors are needed")
        # both tables in one pinned block (PyTorch's pinned allocator does not hand the block out again before the copy ran)
        seg_at = (tab.nbytes + 255) // 256 * 256
        host = torch.empty(seg_at + seg_tab.nbytes, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:tab.nbytes] = tab.view(np.uint8)
        hv[seg_at:] = seg_tab.view(np.uint8)
        desc = host.to(dev, non_blocking=True)
        ws = _lib.workspace(_lib.lib().fsn_mix_workspace_bytes(B, L, longest), dev)
        mix_pairs(bank, desc, seg_at, n_segs, noisy, clean, ws, eps)
    return noisy, clean


def _mix_batch_target(bank, items, L, out, eps, max_rir_len):
    tab, seg_tab, n_segs, longest = pack_items(bank, items, L)
    tgt = pack_targets(items)
    B = len(items)
    if B < 1:
        raise _lib.FsnError("an empty batch")
    longest = longest if max_rir_len is None else max(longest, int(max_rir_len))
    dev = bank.device
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(B, L, dtype=torch.float32, device=dev), torch.empty(B, L, dtype=torch.float32, device=dev))
        noisy, target = out
        if tuple(noisy.shape) != (B, L) or tuple(target.shape) != (B, L):
            raise _lib.FsnError(f"out: two [{B}, {L}] tensors are needed")
        seg_at = (tab.nbytes + 255) // 256 * 256
        tgt_at = (seg_at + seg_tab.nbytes + 255) // 256 * 256
        host = torch.empty(tgt_at + tgt.nbytes, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:tab.nbytes] = tab.view(np.uint8)
        hv[seg_at:seg_at + seg_tab.nbytes] = seg_tab.view(np.uint8)
        hv[tgt_at:] = tgt.view(np.uint8)
        desc = host.to(dev, non_blocking=True)
        ws = _lib.workspace(_lib.lib().fsn_mix_target_workspace_bytes(B, L, longest), dev)
        mix_pairs_target(bank, desc, seg_at, n_segs, tgt_at, noisy, None, target, ws, eps)
    return noisy, target


def mix_pairs_target(bank, desc, seg_at, n_segs, tgt_at, noisy, clean, target, ws, eps=1e-6):
    """fsn_mix_pairs_target as it stands: `desc` as for `mix_pairs`, with the target table (pack_targets) from byte tgt_at
    (a multiple of 8) on; `clean` may be None; `ws` a byte tensor of fsn_mix_target_workspace_bytes.  Only enqueues."""
    B, L = noisy.shape
    _lib.check(_lib.lib().fsn_mix_pairs_target(bank.slabs["clean"].data_ptr(), bank.slabs["noise"].data_ptr(),
                                               bank.slabs["rir"].data_ptr(), bank.slab_format, desc.data_ptr(),
                                               desc.data_ptr() + seg_at, n_segs, B, L, ctypes.c_float(eps),
                                               desc.data_ptr() + tgt_at, _lib.dev_ptr(noisy, "noisy"),
                                               _lib.dev_ptr(clean, "clean", allow_none=True),
                                               _lib.dev_ptr(target, "target"), ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(bank.device)))


def mix_pairs(bank, desc, seg_at, n_segs, noisy, clean, ws, eps=1e-6):
    """fsn_mix_pairs as it stands: `desc` is a device byte tensor holding the item table (pack_items) and, from byte seg_at
    (a multiple of 8) on, the segment table; `ws` a byte tensor of fsn_mix_workspace_bytes.  Only enqueues on the current
    stream - capturable in a graph whose replays read the descriptors `desc` holds at that time."""
    B, L = noisy.shape
    _lib.check(_lib.lib().fsn_mix_pairs(bank.slabs["clean"].data_ptr(), bank.slabs["noise"].data_ptr(),
                                        bank.slabs["rir"].data_ptr(), bank.slab_format, desc.data_ptr(),
                                        desc.data_ptr() + seg_at, n_segs, B, L, ctypes.c_float(eps),
                                        _lib.dev_ptr(noisy, "noisy"), _lib.dev_ptr(clean, "clean"), ws.data_ptr(), ws.numel(),
                                        _lib.stream_ptr(bank.device)))


class MixLoader:
    """Iterable of (noisy, clean) device tensors [batch_size, L], a drop-in for ``Trainer(train_dataloader=...)`` (whose
    ``noisy.to(self.device)`` is then a no-op): every batch is one `mix_batch` call on the CURRENT stream, so the training
    step enqueued after it is ordered behind it and the host does no audio arithmetic.

    Outputs rotate through a two-deep ring: the pair yielded for batch k is overwritten when batch k + 2 is produced, i.e.
    it stays valid while the consumer holds batch k and batch k + 1.  Clone what must live longer.

    Each epoch shuffles the clean indices with (seed, epoch) - call `set_epoch` like a DistributedSampler - and rank r of
    world_size takes every world_size-th index from r on, so ranks see disjoint items; the draws of a rank are seeded by
    (seed, epoch, rank): two loaders with the same arguments yield bit-identical batches.

    cfg.target "shortened" / "early" makes the second tensor the dereverberation target (fsn_mix_pairs_target): `noisy`
    keeps its bits, and the target equals the reverberant clean row on every row whose descriptor says mode 0."""

    def __init__(self, bank, cfg, batch_size, seed, rank=0, world_size=1, drop_last=True):
        if not (0 <= rank < world_size) or batch_size < 1:
            raise ValueError("0 <= rank < world_size and batch_size >= 1 are required")
        self.bank, self.cfg, self.batch_size, self.seed = bank, cfg, int(batch_size), int(seed)
        self.rank, self.world_size, self.drop_last = rank, world_size, drop_last
        self.epoch = 0
        self.per_rank = len(bank) // world_size  # every rank the same number of items
        self.max_rir_len = int(bank.rir_len.max()) if len(bank.rir_len) and cfg.reverb_proportion > 0 else 0
        if cfg.target == "shortened" and self.max_rir_len and getattr(bank, "rir_t60", None) is None:
            raise ValueError('target = "shortened" needs the T60 of every response: MixBank(..., rir_t60=...)')
        self._ring = None

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        full, rest = divmod(self.per_rank, self.batch_size)
        return full if self.drop_last or rest == 0 else full + 1

    def indices(self):
        """This rank's clean indices for the current epoch."""
        perm = np.random.RandomState([self.seed, self.epoch]).permutation(len(self.bank))
        return [int(i) for i in perm[self.rank::self.world_size][:self.per_rank]]

    def draws(self):
        """The descriptor lists of this rank's batches for the current epoch, in order (host work only)."""
        B = self.batch_size
        py = random.Random(self.seed * 1000003 + self.epoch * 1009 + self.rank)
        npr = np.random.RandomState([self.seed, self.epoch, self.rank, 1])
        idx = self.indices()
        for k in range(len(self)):
            yield [draw_item(i, self.bank, self.cfg, py, npr) for i in idx[k * B:(k + 1) * B]]

    def __iter__(self):
        L, B, dev = self.cfg.samples, self.batch_size, self.bank.device
        if self._ring is None:
            self._ring = [tuple(torch.empty(B, L, dtype=torch.float32, device=dev) for _ in range(2)) for _ in range(2)]
        for k, items in enumerate(self.draws()):
            noisy, clean = self._ring[k % 2]
            if len(items) < B:  # the short last batch of drop_last = False
                noisy, clean = noisy[:len(items)], clean[:len(items)]
            yield mix_batch(self.bank, items, L, out=(noisy, clean), max_rir_len=self.max_rir_len,
                            target=self.cfg.target != "reverberant")
