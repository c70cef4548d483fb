"""Drop-in ``Inferencer`` for recipes/dns_interspeech_2020/inferencer.py (+ audio_zen/inferencer/
base_inferencer.py): same constructor ``(config, checkpoint_path, output_dir)``, same ``__call__``
dispatch on ``config["inferencer"]["type"]``, same ``full_band_crm_mask(noisy, inference_args)``.

Only the mode every shipped TOML selects (``full_band_crm_mask``, */inference*.toml:10) is built; the
legacy modes raise.  ``enhance_batch`` is the batched entry the reference lacks (its loop is
hard-wired to one utterance per call, base_inferencer.py:78,173)."""
import importlib
from functools import partial
from pathlib import Path

import numpy as np
import torch

from .acoustics.feature import istft, stft
from .acoustics.mask import decompress_cIRM
from .ragged import pad_utterances, trim_rows


def initialize_module(path, args=None, initialize=True):
    """audio_zen/utils.py:70-105 semantics: "pkg.mod.Name" -> Name(**args)."""
    module_path, _, name = path.rpartition(".")
    obj = getattr(importlib.import_module(module_path), name)
    if not initialize:
        return obj
    return obj(**args) if args else obj()


def _write_wav(path, data, sr):
    try:
        import soundfile as sf
        sf.write(path, data, samplerate=sr)
    except ImportError:
        from scipy.io import wavfile
        wavfile.write(str(path), sr, data)


class Inferencer:
    def __init__(self, config, checkpoint_path=None, output_dir=None, model=None, dataloader=None):
        """``model`` / ``dataloader`` may be injected (tests, services); otherwise they are built
        from ``config["model"]`` / ``config["dataset"]`` exactly like base_inferencer.py:72-81,144-161."""
        if not torch.cuda.is_available():
            raise RuntimeError("fullsubnet_amd needs a ROCm device: this path has no CPU implementation")
        self.device = torch.device("cuda:0")  # audio_zen/utils.py:135-162 always picks cuda:0
        self.config = config
        self.inference_config = config["inferencer"]
        self.acoustic_config = config["acoustics"]
        self.n_fft = self.acoustic_config["n_fft"]
        self.hop_length = self.acoustic_config["hop_length"]
        self.win_length = self.acoustic_config["win_length"]
        self.sr = self.acoustic_config["sr"]
        self.torch_stft = partial(stft, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length)
        self.torch_istft = partial(istft, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length)
        self.fused_call = True  # one utterance per call on the fused FullSubNet configurations: fsn_enhance (False: stage by stage)
        # [inferencer] segment_frames (optional): items longer than that many frames run in segments (Model.enhance_long)
        self.segment_frames = self.inference_config.get("segment_frames")
        if self.segment_frames is not None:
            self.segment_frames = int(self.segment_frames)
            if not 1 <= self.segment_frames <= 4096:
                raise ValueError(f"[inferencer] segment_frames must be in [1, 4096], got {self.segment_frames}")
        # [inferencer] input_sr / output_sr / resample_design (optional): loader items at another rate than the model's
        self.input_sr, self.output_sr, self.resample_design = self.resample_keys(self.inference_config)

        epoch = 0
        if model is None:
            model, epoch = self._load_model(config["model"], checkpoint_path, self.device)
        self.model = model.to(self.device).eval()
        if dataloader is None and "dataset" in config:
            dataset = initialize_module(config["dataset"]["path"], args=config["dataset"]["args"])
            dataloader = torch.utils.data.DataLoader(dataset=dataset, batch_size=1, num_workers=0)
        self.dataloader = dataloader
        if output_dir is not None:
            root = Path(output_dir).expanduser().absolute()
            self.enhanced_dir = root / f"enhanced_{str(epoch).zfill(4)}"
            self.noisy_dir = root / "noisy"
            for d in (self.enhanced_dir, self.noisy_dir):
                d.mkdir(parents=True, exist_ok=True)

    @staticmethod
    def _load_model(model_config, checkpoint_path, device):
        model = initialize_module(model_config["path"], args=model_config["args"])
        checkpoint = torch.load(Path(checkpoint_path).expanduser().absolute(), map_location="cpu", weights_only=False)
        state = {k.replace("module.", ""): v for k, v in checkpoint["model"].items()}  # DDP prefix
        model.load_state_dict(state)  # strict
        return model.to(device).eval(), checkpoint["epoch"]

    # -- recipes/dns_interspeech_2020/inferencer.py:130-145 --------------------------------------
    @torch.no_grad()
    def full_band_crm_mask(self, noisy, inference_args=None):
        model = self.model
        if self._is_long(noisy):
            if not hasattr(model, "enhance_long"):
                from ._lib import FsnError
                raise FsnError(f"[inferencer] segment_frames: {type(model).__module__}.Model has no enhance_long (FullSubNet's "
                               "fused configurations and Fast FullSubNet have one); remove the key for this model")
            return model.enhance_long(noisy, segment_frames=self.segment_frames, n_fft=self.n_fft,
                                      hop_length=self.hop_length).detach().squeeze(0).cpu().numpy()
        if (self.fused_call and noisy.dim() == 2 and noisy.shape[0] == 1 and getattr(model, "_fused", False)
                and self.n_fft == self.win_length == 512 and self.hop_length == 256 and noisy.shape[1] > self.n_fft // 2):
            # ONE utterance (the reference's loop, base_inferencer.py:78,173): band dropping does not fire (model.py:114), so the
            # six lines below are exactly what libfsn_hip's fsn_enhance does in one call - transforms, model, decompress_cIRM
            # and the complex mask inside its kernels (same fp32 products and differences, no contraction)
            return model.enhance(noisy, n_fft=self.n_fft, hop_length=self.hop_length).detach().squeeze(0).cpu().numpy()
        noisy_mag, _, noisy_real, noisy_imag = self.torch_stft(noisy)
        noisy_mag = noisy_mag.unsqueeze(1)
        pred_crm = self.model(noisy_mag)
        pred_crm = pred_crm.permute(0, 2, 3, 1)
        pred_crm = decompress_cIRM(pred_crm)
        enhanced_real = pred_crm[..., 0] * noisy_real - pred_crm[..., 1] * noisy_imag
        enhanced_imag = pred_crm[..., 1] * noisy_real + pred_crm[..., 0] * noisy_imag
        enhanced = self.torch_istft((enhanced_real, enhanced_imag), length=noisy.size(-1), input_type="real_imag")
        return enhanced.detach().squeeze(0).cpu().numpy()

    def _is_long(self, noisy):
        """[inferencer] segment_frames = N: one-utterance items of more than N frames go through ``Model.enhance_long``
        (segments of N frames with carried state, memory that does not grow with the recording at hidden-state width)."""
        n = self.__dict__.get("segment_frames")
        return n is not None and noisy.dim() == 2 and noisy.shape[0] == 1 and 1 + noisy.shape[1] // self.hop_length > n

    @torch.no_grad()
    def enhance_batch(self, noisy, lengths=None):
        """noisy [B, L] (device) -> enhanced [B, L] (device): the fused single-call path
        (libfsn_hip ``fsn_enhance``) for B independent utterances.  ``lengths``: a ragged batch, row b holds
        ``lengths[b]`` samples (``Model.enhance``; libfsn_hip ``fsn_enhance_ragged``)."""
        return self.model.enhance(noisy.to(self.device), n_fft=self.n_fft, hop_length=self.hop_length, lengths=lengths)

    @staticmethod
    def resample_keys(inference_config):
        """``(input_sr, output_sr, design)`` of ``[inferencer]``: ``input_sr`` the rate of the loader's items (None: the
        model's), ``output_sr`` what is written - "model" (default), "input" or a rate -, ``resample_design`` one of
        ``resample.DESIGNS`` (default "scipy").  Raises ``ValueError`` on anything else."""
        input_sr = inference_config.get("input_sr")
        if input_sr is not None:
            if isinstance(input_sr, bool) or not isinstance(input_sr, int) or input_sr < 1:
                raise ValueError(f"[inferencer] input_sr must be a positive integer, got {input_sr!r}")
        output_sr = inference_config.get("output_sr", "model")
        if output_sr not in ("model", "input"):
            if isinstance(output_sr, bool) or not isinstance(output_sr, int) or output_sr < 1:
                raise ValueError(f'[inferencer] output_sr must be "model", "input" or a positive integer, got {output_sr!r}')
        design = inference_config.get("resample_design", "scipy")
        if design not in ("scipy", "sharp"):
            raise ValueError(f'[inferencer] resample_design must be "scipy" or "sharp", got {design!r}')
        return input_sr, output_sr, design

    def _rates(self, sr, output_sr):
        """The rate of the input and the rate to return (``output_sr``: None / "model", "input" or a number)."""
        sr_in = self.sr if sr is None else int(sr)
        if output_sr is None or output_sr == "model":
            return sr_in, self.sr
        return sr_in, sr_in if output_sr == "input" else int(output_sr)

    @torch.no_grad()
    def enhance_utterances(self, utterances, sr=None, output_sr=None, design="scipy"):
        """1-D utterances of any lengths -> their enhanced 1-D waveforms (device), in ONE ragged call: padded to the
        longest, enhanced with their lengths, cut back.

        ``sr``: the rate of the utterances when it is not the model's (``[acoustics] sr``): they are resampled to the
        model's rate on the device in one ragged call (``resample.resample``, filter ``design``), enhanced, and returned at
        ``output_sr`` - the model's rate (default), ``"input"`` or a rate in Hz - cut to ``out_length`` of their original
        lengths (``"input"``: exactly the original lengths)."""
        sr_in, sr_out = self._rates(sr, output_sr)
        if sr_in == self.sr and sr_out == self.sr:
            noisy, lengths = pad_utterances(utterances, device=self.device)
            return trim_rows(self.enhance_batch(noisy, lengths=lengths), lengths)
        from . import resample as rs
        noisy, lengths = pad_utterances(utterances, device=self.device)
        if sr_in != self.sr:
            noisy, _ = rs.resample(noisy, sr_in, self.sr, lengths=lengths, design=design)
        enhanced = self._enhance_model_rate(trim_rows(noisy, [rs.out_length(n, sr_in, self.sr) for n in lengths]))
        if sr_out == self.sr:
            return enhanced
        rows, row_lengths = pad_utterances(enhanced, device=self.device)
        rows, _ = rs.resample(rows, self.sr, sr_out, lengths=row_lengths, design=design)
        return trim_rows(rows, [rs.out_length(n, sr_in, sr_out) for n in lengths])

    def _enhance_model_rate(self, utterances):
        """Utterances at the model's rate -> enhanced, as ``__call__`` runs a group: one ragged call where the model has one
        and no item is past ``segment_frames``, otherwise one ``full_band_crm_mask`` each (``enhance_long`` for those)."""
        items = [(u.unsqueeze(0), None) for u in utterances]
        if self._ragged_ok(items):
            noisy, lengths = pad_utterances(utterances, device=self.device)
            return trim_rows(self.enhance_batch(noisy, lengths=lengths), lengths)
        args = self.inference_config.get("args", {})
        return [torch.as_tensor(self.full_band_crm_mask(n.to(self.device), args), device=self.device) for n, _ in items]

    def _ragged_ok(self, items):
        """Whether a group of loader items runs as one ragged call: 1-D utterances (one channel) on a model whose
        ``ragged_enhance_ok`` says it enhances a ragged batch in one call at this transform (FullSubNet's fused
        configurations, Fast FullSubNet's time-major path), long enough for the STFT's reflect padding."""
        ragged_ok = getattr(self.model, "ragged_enhance_ok", None)
        return (self.fused_call and ragged_ok is not None and ragged_ok(self.n_fft, self.hop_length)
                and self.n_fft == self.win_length and not any(self._is_long(n) for n, _ in items)
                and all(n.dim() == 2 and n.shape[0] == 1 and n.shape[1] > self.n_fft // 2 for n, _ in items))

    def __getattr__(self, name):
        if name in ("mag", "scaled_mask", "sub_band_crm_mask", "overlapped_chunk", "time_domain"):
            raise NotImplementedError(f"inference type {name!r} is outside the FullSubNet path (no shipped TOML uses it)")
        raise AttributeError(name)

    @torch.no_grad()
    def __call__(self):
        """base_inferencer.py:163-195."""
        inference_type = self.inference_config["type"]
        assert inference_type == "full_band_crm_mask", f"Not implemented Inferencer type: {inference_type}"
        inference_args = self.inference_config.get("args", {})
        # [inferencer] batch_size (optional, default 1 = the reference's loop): enhance that many loader items per call
        batch_size = int(self.inference_config.get("batch_size", 1))
        if batch_size < 1:
            raise ValueError(f"[inferencer] batch_size must be >= 1, got {batch_size}")
        resampled = self.__dict__.get("input_sr") is not None or self.__dict__.get("output_sr", "model") != "model"
        group = []
        for noisy, name in self.dataloader:
            assert len(name) == 1, "The batch size of inference stage must 1."
            if resampled:
                group.append((noisy, name[0]))
                if len(group) == batch_size:
                    self._enhance_group_resampled(group)
                    group = []
                continue
            if batch_size == 1:
                enhanced = getattr(self, inference_type)(noisy.to(self.device), inference_args)
                self._write_item(name[0], noisy, enhanced)
                continue
            group.append((noisy, name[0]))
            if len(group) == batch_size:
                self._enhance_group(group, inference_type, inference_args)
                group = []
        if group:  # the last, partial group
            if resampled:
                self._enhance_group_resampled(group)
            else:
                self._enhance_group(group, inference_type, inference_args)

    def _enhance_group_resampled(self, items):
        """Loader items at ``[inferencer] input_sr``: resampled, enhanced and resampled to ``output_sr`` on the device
        (``enhance_utterances``); the enhanced file carries the output rate, the noisy file beside it the input's."""
        for noisy, name in items:
            if noisy.dim() != 2 or noisy.shape[0] != 1:
                raise ValueError(f"[inferencer] input_sr / output_sr: item {name!r} of shape {tuple(noisy.shape)} is not one "
                                 "single-channel utterance [1, L]")
        sr_in, sr_out = self._rates(self.input_sr, self.output_sr)
        outs = self.enhance_utterances([n[0] for n, _ in items], sr=sr_in, output_sr=sr_out, design=self.resample_design)
        for (noisy, name), enhanced in zip(items, outs):
            self._write_item(name, noisy, enhanced.detach().cpu().numpy(), enhanced_sr=sr_out, noisy_sr=sr_in)

    def _enhance_group(self, items, inference_type, inference_args):
        """Several loader items as ONE ragged call of the library where the model has one; otherwise one
        ``full_band_crm_mask`` each.  Every file is written exactly as the one-item loop writes it."""
        if self._ragged_ok(items):
            outs = self.enhance_utterances([n[0] for n, _ in items])
            outs = [o.detach().cpu().numpy() for o in outs]
        else:
            outs = [getattr(self, inference_type)(n.to(self.device), inference_args) for n, _ in items]
        for (noisy, name), enhanced in zip(items, outs):
            self._write_item(name, noisy, enhanced)

    def _write_item(self, name, noisy, enhanced, enhanced_sr=None, noisy_sr=None):
        """base_inferencer.py:178-195: the enhanced waveform peak-normalised to 0.8 of int16 full scale, the noisy
        input beside it trimmed to the same length (whole when the two files are at different rates)."""
        enhanced_sr = self.sr if enhanced_sr is None else enhanced_sr
        noisy_sr = self.sr if noisy_sr is None else noisy_sr
        amp = np.iinfo(np.int16).max
        enhanced = np.int16(0.8 * amp * enhanced / np.max(np.abs(enhanced)))
        _write_wav(self.enhanced_dir / f"{name}.wav", enhanced, enhanced_sr)
        noisy = noisy.detach().squeeze(0).numpy()
        if np.ndim(noisy) > 1:
            noisy = noisy[0, :]
        _write_wav(self.noisy_dir / f"{name}.wav", noisy[: enhanced.shape[-1]] if noisy_sr == enhanced_sr else noisy, noisy_sr)
