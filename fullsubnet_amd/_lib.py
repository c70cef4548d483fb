"""ctypes binding of libfsn_hip.so (include/fsn_hip.h).

There is deliberately NO fallback: if the HIP library is missing or a call fails, the caller
gets an exception.  PyTorch is used for device memory and streams only.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfsn_hip.so")

NORM_TYPES = {"offline_laplace_norm": 0, "cumulative_laplace_norm": 1}  # the fused FullSubNet kernels (cfg.norm_type)
ALL_NORM_TYPES = {"offline_laplace_norm": 0, "cumulative_laplace_norm": 1, "offline_gaussian_norm": 2,
                  "cumulative_layer_norm": 3, "forgetting_norm": 4}  # fsn_norm

_f32p = ctypes.c_void_p
_lib = None


class FsnError(RuntimeError):
    pass


class Cfg(ctypes.Structure):
    _fields_ = [("num_freqs", ctypes.c_int), ("look_ahead", ctypes.c_int), ("sb_num_neighbors", ctypes.c_int),
                ("fb_hidden", ctypes.c_int), ("sb_hidden", ctypes.c_int), ("norm_type", ctypes.c_int),
                ("arith", ctypes.c_int)]


# FSN_ARITH_* of include/fsn_hip.h.  "f32" is the default and what every parity claim refers to; "f16x3" is
# the opt-in split-precision experiment (Model.arithmetic = "f16x3", or FSN_F16X3=1 in the environment of the
# HOST process - the library itself reads no environment variables).
ARITH = {"f32": 0, "f16x3": 1, "f16": 2, "bf16": 3}  # "f16" / "bf16": training entries only (autocast arithmetic)
ARITH_SAVES16 = 0x100  # FSN_ARITH_SAVES16: "f16+s16" / "bf16+s16" - the saved gates in the 16-bit type too
ARITH.update({"f16+s16": 2 | ARITH_SAVES16, "bf16+s16": 3 | ARITH_SAVES16})


def default_arith():
    return "f16x3" if os.environ.get("FSN_F16X3", "")[:1] == "1" else "f32"


PARAM_FIELDS = [
    "fb_w_ih_l0", "fb_w_hh_l0", "fb_b_ih_l0", "fb_b_hh_l0", "fb_w_ih_l1", "fb_w_hh_l1", "fb_b_ih_l1", "fb_b_hh_l1",
    "fb_fc_w", "fb_fc_b",
    "sb_w_ih_l0", "sb_w_hh_l0", "sb_b_ih_l0", "sb_b_hh_l0", "sb_w_ih_l1", "sb_w_hh_l1", "sb_b_ih_l1", "sb_b_hh_l1",
    "sb_fc_w", "sb_fc_b",
]
# reference state_dict key of each field
STATE_KEYS = [
    "fb_model.sequence_model.weight_ih_l0", "fb_model.sequence_model.weight_hh_l0",
    "fb_model.sequence_model.bias_ih_l0", "fb_model.sequence_model.bias_hh_l0",
    "fb_model.sequence_model.weight_ih_l1", "fb_model.sequence_model.weight_hh_l1",
    "fb_model.sequence_model.bias_ih_l1", "fb_model.sequence_model.bias_hh_l1",
    "fb_model.fc_output_layer.weight", "fb_model.fc_output_layer.bias",
    "sb_model.sequence_model.weight_ih_l0", "sb_model.sequence_model.weight_hh_l0",
    "sb_model.sequence_model.bias_ih_l0", "sb_model.sequence_model.bias_hh_l0",
    "sb_model.sequence_model.weight_ih_l1", "sb_model.sequence_model.weight_hh_l1",
    "sb_model.sequence_model.bias_ih_l1", "sb_model.sequence_model.bias_hh_l1",
    "sb_model.fc_output_layer.weight", "sb_model.fc_output_layer.bias",
]


class Lstm2Stack(ctypes.Structure):
    """fsn_lstm2_stack (include/fsn_hip.h)."""
    _fields_ = ([("x", ctypes.c_void_p), ("ldx", ctypes.c_long)] +
                [(n, ctypes.c_void_p) for n in ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1")] +
                [("N", ctypes.c_int), ("I", ctypes.c_int), ("H0", ctypes.c_int), ("H1", ctypes.c_int),
                 ("hseq1", ctypes.c_void_p)])


class AdamCfg(ctypes.Structure):
    _fields_ = [("lr", ctypes.c_float), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("max_norm", ctypes.c_float), ("step", ctypes.c_int)]


ADAM_MAX_TENSORS = 32  # FSN_ADAM_MAX_TENSORS


class TrainDims(ctypes.Structure):  # fsn_train_dims
    _fields_ = [("B", ctypes.c_int), ("F", ctypes.c_int), ("T", ctypes.c_int), ("look_ahead", ctypes.c_int),
                ("nb", ctypes.c_int), ("groups", ctypes.c_int), ("norm", ctypes.c_int)]


ABI_VERSION = 118  # FSN_ABI_VERSION of include/fsn_hip.h these signatures were written against


class MaskSection(ctypes.Structure):  # fsn_mask_section
    _fields_ = [("o", ctypes.c_void_p), ("Np", ctypes.c_int), ("ld", ctypes.c_int), ("lower", ctypes.c_int),
                ("units", ctypes.c_int), ("center", ctypes.c_int)]


class Params(ctypes.Structure):
    _fields_ = [(n, _f32p) for n in PARAM_FIELDS]


class FastCfg(ctypes.Structure):  # fsn_fast_cfg
    _fields_ = [(n, ctypes.c_int) for n in ("F", "num_mels", "shrink", "mel_neighbors", "enc_neighbors", "bn_hidden",
                                            "bn_layers", "norm")]


_LAYER = ("w_ih", "w_hh", "b_ih", "b_hh")
FAST_PARAM_FIELDS = (["mel_w"] + [f"enc0_{n}" for n in _LAYER] + [f"enc1_{n}" for n in _LAYER] + ["enc1_fc_w", "enc1_fc_b"] +
                     [f"bn_{n}_l0" for n in _LAYER] + [f"bn_{n}_l1" for n in _LAYER] + ["bn_fc_w", "bn_fc_b"] +
                     [f"dec0_{n}" for n in _LAYER] + [f"dec1_{n}" for n in _LAYER] + ["dec1_fc_w", "dec1_fc_b"])


class FastParams(ctypes.Structure):  # fsn_fast_params
    _fields_ = [(n, _f32p) for n in FAST_PARAM_FIELDS]


IMPROVED_MAX_SECTIONS = 8  # FSN_IMPROVED_MAX_SECTIONS
IMPROVED_BLOCK_FIELDS = tuple(f"{n}_l{l}" for l in (0, 1) for n in _LAYER) + ("fc_w", "fc_b")  # one block of fsn_improved_params


class ImprovedSection(ctypes.Structure):  # fsn_improved_section
    _fields_ = [(n, ctypes.c_int) for n in ("lower", "upper", "sb_center", "sb_neighbors", "fb_center", "fb_neighbors")]


class ImprovedCfg(ctypes.Structure):  # fsn_improved_cfg
    _fields_ = [("F", ctypes.c_int), ("fdrc", ctypes.c_float), ("num_sections", ctypes.c_int), ("fb_hidden", ctypes.c_int),
                ("sb_hidden", ctypes.c_int), ("cell", ctypes.c_int), ("fb_activation", ctypes.c_int),
                ("sb_activation", ctypes.c_int), ("sec", ImprovedSection * IMPROVED_MAX_SECTIONS)]


class ImprovedParams(ctypes.Structure):  # fsn_improved_params
    _fields_ = [("fb", _f32p * 10), ("sb", (_f32p * 10) * IMPROVED_MAX_SECTIONS)]


# name -> (restype, argtypes); must list every symbol declared in include/fsn_hip.h
_c = ctypes
SIGNATURES = {
    "fsn_last_error": (_c.c_char_p, []),
    "fsn_version": (_c.c_int, []),
    "fsn_stft": (_c.c_int, [_f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _f32p, _f32p, _f32p, _f32p,
                            _c.c_void_p]),
    "fsn_stft_ragged": (_c.c_int, [_f32p, _c.c_void_p] + [_c.c_int] * 5 + [_f32p, _f32p, _f32p, _f32p, _c.c_void_p]),
    "fsn_stft_ragged_generic": (_c.c_int, [_f32p, _c.c_void_p] + [_c.c_int] * 5 + [_f32p, _f32p, _f32p, _f32p, _c.c_void_p]),
    "fsn_istft_ragged_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_istft_ragged": (_c.c_int, [_f32p, _f32p, _c.c_void_p] + [_c.c_int] * 5 + [_f32p, _c.c_int, _f32p, _c.c_void_p,
                                                                               _c.c_size_t, _c.c_void_p]),
    "fsn_mask_istft_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_mask_istft": (_c.c_int, [_f32p, _f32p, _f32p, _c.c_void_p] + [_c.c_int] * 6 + [_f32p, _c.c_int, _f32p, _c.c_void_p,
                                                                                         _c.c_size_t, _c.c_void_p]),
    "fsn_istft_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_istft": (_c.c_int, [_f32p, _f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _f32p, _c.c_int, _f32p,
                             _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_decompress_cirm": (_c.c_int, [_f32p, _f32p, _c.c_size_t, _c.c_void_p]),
    "fsn_compress_cirm": (_c.c_int, [_f32p, _f32p, _c.c_size_t, _c.c_void_p]),
    "fsn_build_cirm": (_c.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _c.c_size_t, _c.c_void_p]),
    "fsn_norm_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_norm": (_c.c_int, [_f32p, _f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_float,
                            _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_packed_bytes": (_c.c_size_t, [_c.POINTER(Cfg)]),
    "fsn_fullsubnet_pack": (_c.c_int, [_c.POINTER(Cfg), _c.POINTER(Params), _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_workspace_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int, _c.c_int]),
    "fsn_fullsubnet_forward": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p,
                                          _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_fullband": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p,
                                           _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_rows_workspace_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int, _c.c_int, _c.c_long, _c.c_long]),
    "fsn_fullsubnet_forward_rows": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _f32p, _c.c_int, _c.c_int, _c.c_long,
                                               _c.c_long, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_enhance_workspace_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_enhance": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                               _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_enhance_ragged": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _f32p, _f32p, _c.c_void_p, _c.c_int, _c.c_int,
                                      _c.c_int, _c.c_int, _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_stream_state_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int]),
    "fsn_fullsubnet_stream_workspace_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int, _c.c_int]),
    "fsn_fullsubnet_stream_step": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _f32p,
                                              _c.c_int, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_segment_state_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int]),
    "fsn_fullsubnet_segment_workspace_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int, _c.c_int]),
    "fsn_fullsubnet_segment_stats": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_size_t, _f32p, _c.c_int, _c.c_int,
                                                _c.c_void_p]),
    "fsn_fullsubnet_segment_fullband": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                                   _c.c_void_p, _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t,
                                                   _c.c_void_p]),
    "fsn_fullsubnet_segment_subband": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                                  _c.c_void_p, _f32p, _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p,
                                                  _c.c_size_t, _c.c_void_p]),
    "fsn_fullsubnet_segment_divisors": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_int, _f32p,
                                                   _f32p, _c.c_void_p]),
    "fsn_fullsubnet_stream_pool_state_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int]),
    "fsn_fullsubnet_stream_pool_workspace_bytes": (_c.c_size_t, [_c.POINTER(Cfg), _c.c_int, _c.c_int]),
    "fsn_fullsubnet_stream_pool_reset": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p,
                                                    _c.c_int, _c.c_void_p]),
    "fsn_fullsubnet_stream_pool_step": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                                   _c.c_void_p, _c.c_int, _f32p, _c.c_int, _f32p, _c.c_void_p,
                                                   _c.c_size_t, _c.c_void_p]),
    "fsn_stream_pool_analysis": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                            _f32p, _f32p, _c.c_void_p, _c.c_int, _c.c_int, _f32p, _f32p, _c.c_void_p]),
    "fsn_stream_pool_synthesis": (_c.c_int, [_c.POINTER(Cfg), _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                             _f32p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _f32p, _f32p,
                                             _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_debug_poison_if": (_c.c_int, [_c.c_void_p, _f32p, _c.c_size_t, _c.c_void_p]),
    "fsn_lstm_layer_save_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm_layer_fwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm_layer_forward": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                          _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                          _c.c_void_p]),
    "fsn_lstm_layer_bwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm2_train_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm2_train_is_persistent": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm2_forward_train": (_c.c_int, [_f32p, _c.c_long] + [_f32p] * 8 + [_c.c_int] * 4 + [_f32p, _f32p, _c.c_void_p,
                                           _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "fsn_lstm2_bwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm2_backward": (_c.c_int, [_f32p, _f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p] + [_c.c_int] * 4 +
                           [_f32p, _f32p, _c.c_void_p, _c.c_void_p, _f32p, _c.c_long] + [_f32p] * 6 +
                           [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "fsn_lstm_layer_plan_rows": (_c.c_int, [_c.c_int, _c.c_int]),
    "fsn_lstm_layer_fc_supported": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_long, _c.c_int, _c.c_int]),
    "fsn_lstm_layer_fc_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "fsn_lstm_layer_forward_fc": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p] + [_c.c_int] * 4 +
                                  [_f32p, _f32p, _c.c_int, _f32p, _f32p, _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_lstm2_backward_phase": (_c.c_int, [_f32p, _f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p] + [_c.c_int] * 4 +
                                 [_f32p, _f32p, _c.c_void_p, _c.c_void_p, _f32p, _c.c_long] + [_f32p] * 6 +
                                 [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_lstm_layer_backward": (_c.c_int, [_f32p, _f32p, _c.c_long, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _f32p, _c.c_void_p, _f32p, _c.c_long, _f32p, _f32p, _f32p,
                                           _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_lstm2_forward_is_persistent": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_long, _c.c_int, _c.c_int]),
    "fsn_lstm2_fwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm2_forward": (_c.c_int, [_f32p, _c.c_long] + [_f32p] * 8 + [_c.c_int] * 5 + [_f32p, _c.c_void_p, _c.c_size_t,
                                                                                         _c.c_void_p]),
    "fsn_improved_section_input_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "fsn_improved_section_input": (_c.c_int, [_f32p, _f32p] + [_c.c_int] * 11 + [_c.c_float, _f32p, _c.c_int, _c.c_int,
                                                                                _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_improved_section_input_ragged": (_c.c_int, [_f32p, _f32p, _c.c_void_p] + [_c.c_int] * 11
                                          + [_c.c_float, _f32p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_improved_front_norm_ragged_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_improved_front_norm_ragged": (_c.c_int, [_f32p, _c.c_void_p] + [_c.c_int] * 4 + [_c.c_float, _f32p, _f32p, _c.c_void_p,
                                                                                         _c.c_size_t, _c.c_void_p]),
    "fsn_lstm2_multi_is_persistent": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_lstm2_multi_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_lstm2_forward_multi": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_lstm_layer_packed_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "fsn_lstm_layer_pack": (_c.c_int, [_f32p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t,
                                       _c.c_void_p]),
    "fsn_lstm_layer_state_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm_layer_forward_state": (_c.c_int, [_f32p, _c.c_long, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                                _f32p, _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_gru2_forward_supported": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru2_fwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru2_forward": (_c.c_int, [_f32p, _c.c_long] + [_f32p] * 8 + [_c.c_int] * 4 + [_f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_gru_layer_is_persistent": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_long, _c.c_int]),
    "fsn_gru_layer_save_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru_layer_fwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru_layer_forward": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                         _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                         _c.c_void_p]),
    "fsn_gru_layer_forward_state": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                               _c.c_int, _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_gru_layer_bwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru_layer_backward": (_c.c_int, [_f32p, _f32p, _c.c_long, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                          _f32p, _c.c_void_p, _f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p,
                                          _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_linear_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_linear_forward": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _f32p,
                                      _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_linear_backward": (_c.c_int, [_f32p, _c.c_long, _f32p, _c.c_long, _f32p, _c.c_int, _c.c_int, _c.c_int, _f32p,
                                       _c.c_long, _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_mse_loss_workspace_bytes": (_c.c_size_t, [_c.c_size_t]),
    "fsn_mse_loss": (_c.c_int, [_f32p, _f32p, _c.c_size_t, _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_clip_adam_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.POINTER(_c.c_size_t)]),
    "fsn_clip_adam_step": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p),
                                      _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_void_p), _c.POINTER(_c.c_size_t),
                                      _c.c_void_p, _f32p, _f32p, _f32p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                      _c.c_void_p]),
    "fsn_train_rows": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_int)]),
    "fsn_train_glue_workspace_bytes": (_c.c_size_t, [_c.c_void_p]),
    "fsn_train_den_elems": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "fsn_train_fb_input": (_c.c_int, [_c.c_void_p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_train_sb_input": (_c.c_int, [_c.c_void_p, _f32p, _f32p, _c.c_long, _c.c_int, _c.c_int, _f32p, _c.c_int, _f32p,
                                      _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_train_sb_input_backward": (_c.c_int, [_c.c_void_p, _f32p, _f32p, _c.c_int, _f32p, _f32p, _c.c_long, _c.c_int, _f32p,
                                               _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_train_mask_out": (_c.c_int, [_c.c_void_p, _f32p, _c.c_int, _f32p, _c.c_void_p]),
    "fsn_train_mask_grad": (_c.c_int, [_c.c_void_p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_train_rows_pieces": (_c.c_int, [_f32p, _f32p, _c.c_int, _c.c_long, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_train_cirm_target": (_c.c_int, [_c.c_void_p, _f32p, _f32p, _f32p, _f32p, _f32p, _c.c_void_p]),
    "fsn_scale_by_scalar": (_c.c_int, [_f32p, _f32p, _f32p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_low_rate_frames": (_c.c_int, [_c.c_int, _c.c_int]),
    "fsn_fast_glue_workspace_bytes": (_c.c_size_t, [_c.c_int] * 4),
    "fsn_fast_spec_rows": (_c.c_int, [_f32p] + [_c.c_int] * 4 + [_f32p, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_fast_norm_rows": (_c.c_int, [_f32p] + [_c.c_int] * 4 + [_f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_bottleneck_input": (_c.c_int, [_f32p, _f32p, _c.c_long] + [_c.c_int] * 7 + [_f32p, _c.c_int, _c.c_int, _c.c_void_p,
                                             _c.c_size_t, _c.c_void_p]),
    "fsn_fast_decoder_input": (_c.c_int, [_f32p, _c.c_long, _f32p, _c.c_long, _c.c_long] + [_c.c_int] * 6 + [_f32p, _c.c_void_p]),
    "fsn_fast_mask_out": (_c.c_int, [_f32p, _c.c_long] + [_c.c_int] * 5 + [_f32p, _c.c_void_p]),
    "fsn_fast_spec_rows_ragged": (_c.c_int, [_f32p, _c.c_void_p] + [_c.c_int] * 4 + [_f32p, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_fast_norm_rows_ragged": (_c.c_int, [_f32p, _c.c_void_p] + [_c.c_int] * 5 + [_f32p, _c.c_void_p, _c.c_size_t,
                                                                                     _c.c_void_p]),
    "fsn_fast_bottleneck_input_ragged": (_c.c_int, [_f32p, _f32p, _c.c_long, _c.c_void_p] + [_c.c_int] * 8
                                         + [_f32p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_mask_out_ragged": (_c.c_int, [_f32p, _c.c_long, _c.c_void_p] + [_c.c_int] * 5 + [_f32p, _c.c_void_p]),
    "fsn_profile_enable": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "fsn_stream_timeout_policy": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "fsn_debug_g16_kernels": (_c.c_int, [_c.c_int]),
    "fsn_debug_tn16h_wide": (_c.c_int, [_c.c_int]),
    "fsn_set_persistent_mode": (_c.c_int, [_c.c_int]),
    "fsn_set_persistent_timeout_ms": (_c.c_int, [_c.c_int]),
    "fsn_stream_status": (_c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_uint), _c.POINTER(_c.c_uint)]),
    "fsn_stream_status_clear": (_c.c_int, [_c.c_void_p]),
    "fsn_debug_hog": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_float, _f32p, _c.c_void_p]),
    "fsn_debug_persist_stats": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "fsn_debug_persist_set_fits": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_void_p]),
    "fsn_debug_tn_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_long, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "fsn_debug_lstm2_plan16": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_long, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_debug_gemm_tn_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_long]),
    "fsn_debug_tn16_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_long, _c.c_void_p, _c.c_void_p]),
    "fsn_debug_to16": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "fsn_debug_gemm_tn16h": (_c.c_int, [_c.c_void_p, _c.c_long, _c.c_void_p, _c.c_long, _c.c_void_p, _c.c_long, _c.c_int, _c.c_int,
                                        _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "fsn_debug_gemm_tn16n": (_c.c_int, [_c.c_void_p, _c.c_long, _c.c_void_p, _c.c_long, _c.c_void_p, _c.c_long, _c.c_int, _c.c_int,
                                        _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "fsn_debug_gemm_tn": (_c.c_int, [_c.c_void_p, _c.c_long, _c.c_void_p, _c.c_long, _c.c_void_p, _c.c_long, _c.c_int, _c.c_int,
                                     _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p]),
    "fsn_debug_gemm_dx16": (_c.c_int, [_c.c_void_p, _c.c_long, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_long,
                                       _c.c_long, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_debug_core_chunks": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_debug_core_plan": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_debug_core_call_plan": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_long, _c.c_long, _c.c_void_p, _c.c_int]),
    "fsn_debug_core_last_launches": (_c.c_uint, []),
    "fsn_debug_stream_state_layout": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_debug_stream_pool_layout": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    "fsn_improved_front": (_c.c_int, [_f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _f32p, _c.c_void_p]),
    "fsn_bft_to_rows": (_c.c_int, [_f32p, _c.c_int, _c.c_int, _c.c_int, _f32p, _c.c_int, _c.c_int, _c.c_void_p]),
    "fsn_rows_to_bft": (_c.c_int, [_f32p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _f32p, _c.c_void_p]),
    "fsn_improved_mask_apply": (_c.c_int, [_c.c_int, _c.c_void_p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int, _f32p, _f32p,
                                           _c.c_void_p]),
    "fsn_conv_rows_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_conv_rows": (_c.c_int, [_f32p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _f32p,
                                 _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_mix_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_mix_pairs": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                 _c.c_int, _c.c_int, _c.c_float, _f32p, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_rir_shorten": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _f32p,
                                   _c.c_int, _f32p, _c.c_void_p, _c.c_void_p]),
    "fsn_mix_target_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_mix_pairs_target": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                        _c.c_int, _c.c_int, _c.c_float, _c.c_void_p, _f32p, _f32p, _f32p, _c.c_void_p,
                                        _c.c_size_t, _c.c_void_p]),
    "fsn_stoi_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_stoi": (_c.c_int, [_f32p, _f32p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                            _c.c_void_p]),
    "fsn_si_sdr": (_c.c_int, [_f32p, _f32p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "fsn_resample_out_length": (_c.c_long, [_c.c_long, _c.c_int, _c.c_int]),
    "fsn_resample_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_double]),
    "fsn_resample_taps": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_double, _c.c_double, _c.c_void_p, _c.c_size_t,
                                     _c.c_void_p]),
    "fsn_resample": (_c.c_int, [_f32p, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double,
                                _c.c_double, _f32p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_debug_resample_plan": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_resample_stream_ready": (_c.c_long, [_c.c_long, _c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_resample_stream_state_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_resample_stream_init": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_double,
                                            _c.c_double, _c.c_void_p]),
    "fsn_resample_stream_push": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                            _c.c_int, _f32p, _c.c_int, _f32p, _c.c_int, _c.c_void_p]),
    "fsn_resample_stream_reset": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                             _c.c_int, _c.c_void_p]),
    "fsn_lstm_bilayer_save_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm_bilayer_fwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm_bilayer_forward": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                            _c.c_int, _f32p, _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                            _c.c_void_p]),
    "fsn_lstm_bilayer_bwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_lstm_bilayer_backward": (_c.c_int, [_f32p, _c.c_long, _f32p, _c.c_long, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                             _c.c_int, _f32p, _c.c_long, _c.c_void_p, _f32p, _c.c_long, _f32p, _f32p, _f32p,
                                             _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_gru_bilayer_save_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru_bilayer_fwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru_bilayer_forward": (_c.c_int, [_f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _f32p, _c.c_long, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                           _c.c_void_p]),
    "fsn_gru_bilayer_bwd_workspace_bytes": (_c.c_size_t, [_c.c_int, _c.c_int, _c.c_int, _c.c_int]),
    "fsn_gru_bilayer_backward": (_c.c_int, [_f32p, _c.c_long, _f32p, _c.c_long, _f32p, _f32p, _c.c_int, _c.c_int, _c.c_int,
                                            _c.c_int, _f32p, _c.c_long, _c.c_void_p, _f32p, _c.c_long, _f32p, _f32p, _f32p, _f32p,
                                            _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_debug_bilayer_last_step_launches": (_c.c_uint, []),
    "fsn_fast_stream_packed_bytes": (_c.c_size_t, [_c.c_void_p]),
    "fsn_fast_stream_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_stream_state_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "fsn_fast_stream_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "fsn_fast_stream_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _f32p, _c.c_int,
                                        _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_debug_fast_stream_state_layout": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_fast_segment_state_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "fsn_fast_segment_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "fsn_fast_segment_stats": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _f32p, _c.c_int, _c.c_int, _f32p,
                                          _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_segment_encoder": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _f32p,
                                            _c.c_int, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_segment_decoder": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _f32p,
                                            _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_segment_divisors": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_int, _f32p, _f32p,
                                             _c.c_void_p]),
    "fsn_debug_fast_segment_state_layout": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_fast_stream_pool_state_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "fsn_fast_stream_pool_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "fsn_fast_stream_pool_reset": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                              _c.c_void_p]),
    "fsn_fast_stream_pool_step": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p,
                                             _c.c_int, _c.c_int, _f32p, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_fast_stream_pool_analysis": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                                 _f32p, _f32p, _c.c_void_p, _c.c_int, _c.c_int, _f32p, _f32p, _c.c_void_p]),
    "fsn_fast_stream_pool_synthesis": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                                  _f32p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int, _f32p, _f32p,
                                                  _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_debug_fast_stream_pool_layout": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_improved_stream_packed_bytes": (_c.c_size_t, [_c.c_void_p]),
    "fsn_improved_stream_pack": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_improved_stream_state_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "fsn_improved_stream_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "fsn_improved_stream_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_long, _f32p, _c.c_int,
                                            _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_debug_improved_stream_state_layout": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_int]),
    "fsn_debug_improved_stream_form": (_c.c_int, [_c.c_int]),
    "fsn_improved_segment_stats": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_long, _c.c_void_p, _f32p, _c.c_int,
                                              _c.c_int, _c.c_void_p]),
    "fsn_improved_segment_fullband": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_long,
                                                 _c.c_void_p, _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t,
                                                 _c.c_void_p]),
    "fsn_improved_segment_sections": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_long, _c.c_void_p,
                                                 _f32p, _f32p, _c.c_int, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_improved_segment_divisors": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_int, _f32p, _f32p,
                                                 _c.c_void_p]),
    "fsn_improved_stream_pool_state_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int]),
    "fsn_improved_stream_pool_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_int, _c.c_int]),
    "fsn_improved_stream_pool_reset": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                                  _c.c_void_p]),
    "fsn_improved_stream_pool_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p,
                                                 _c.c_int, _f32p, _c.c_int, _f32p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "fsn_improved_stream_pool_analysis": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int, _f32p,
                                                     _f32p, _c.c_void_p, _c.c_int, _c.c_int, _f32p, _f32p, _c.c_void_p]),
    "fsn_improved_stream_pool_synthesis": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_int,
                                                      _f32p, _c.c_void_p, _c.c_int, _c.c_int, _f32p, _f32p, _c.c_void_p]),
    "fsn_debug_improved_stream_pool_layout": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    "fsn_profile_num_stages": (_c.c_int, []),
    "fsn_profile_stage_name": (_c.c_char_p, [_c.c_int]),
    "fsn_profile_read": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_float), _c.c_int]),
}
# Entries added to revision 118 without a new number: a library built from an older tree of the same revision lacks them
ADDED_IN_118 = ("fsn_stoi_workspace_bytes", "fsn_stoi", "fsn_si_sdr", "fsn_resample_out_length",
                "fsn_resample_workspace_bytes", "fsn_resample_taps", "fsn_resample", "fsn_debug_resample_plan",
                "fsn_resample_stream_ready", "fsn_resample_stream_state_bytes", "fsn_resample_stream_init",
                "fsn_resample_stream_push", "fsn_resample_stream_reset", "fsn_debug_stream_state_layout",
                "fsn_debug_stream_pool_layout", "fsn_lstm_bilayer_forward", "fsn_lstm_bilayer_backward",
                "fsn_gru_bilayer_forward", "fsn_gru_bilayer_backward", "fsn_debug_bilayer_last_step_launches",
                "fsn_fast_stream_packed_bytes", "fsn_fast_stream_pack", "fsn_fast_stream_state_bytes",
                "fsn_fast_stream_workspace_bytes", "fsn_fast_stream_step", "fsn_debug_fast_stream_state_layout",
                "fsn_fast_stream_pool_state_bytes", "fsn_fast_stream_pool_workspace_bytes", "fsn_fast_stream_pool_reset",
                "fsn_fast_stream_pool_step", "fsn_fast_stream_pool_analysis", "fsn_fast_stream_pool_synthesis",
                "fsn_debug_fast_stream_pool_layout",
                "fsn_fast_segment_state_bytes", "fsn_fast_segment_workspace_bytes", "fsn_fast_segment_stats",
                "fsn_fast_segment_encoder", "fsn_fast_segment_decoder", "fsn_fast_segment_divisors",
                "fsn_debug_fast_segment_state_layout",
                "fsn_improved_stream_packed_bytes", "fsn_improved_stream_pack", "fsn_improved_stream_state_bytes",
                "fsn_improved_stream_workspace_bytes", "fsn_improved_stream_step", "fsn_debug_improved_stream_state_layout",
                "fsn_debug_improved_stream_form",
                "fsn_improved_segment_stats", "fsn_improved_segment_fullband", "fsn_improved_segment_sections",
                "fsn_improved_segment_divisors",
                "fsn_improved_stream_pool_state_bytes", "fsn_improved_stream_pool_workspace_bytes",
                "fsn_improved_stream_pool_reset", "fsn_improved_stream_pool_step", "fsn_improved_stream_pool_analysis",
                "fsn_improved_stream_pool_synthesis", "fsn_debug_improved_stream_pool_layout",
                "fsn_rir_shorten", "fsn_mix_target_workspace_bytes", "fsn_mix_pairs_target")


def lib():
    """Load (once) and return the HIP library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FsnError(
                f"{LIB_PATH} is missing: build it with `python -m fullsubnet_amd.build` (hipcc, gfx950). "
                "There is no CPU / PyTorch fallback for this path.")
        handle = ctypes.CDLL(LIB_PATH)
        handle.fsn_version.restype = ctypes.c_int
        built = handle.fsn_version()
        if built != ABI_VERSION:  # argument lists differ between revisions: a stale library would misread them silently
            raise FsnError(f"{LIB_PATH} was built for ABI revision {built}, this package binds revision {ABI_VERSION}: "
                           "rebuild it with `python -m fullsubnet_amd.build`")
        missing = [name for name in ADDED_IN_118 if not hasattr(handle, name)]
        if missing:
            raise FsnError(f"{LIB_PATH} has no {', '.join(missing)}: it was built before these entries were added; "
                           "rebuild it with `python -m fullsubnet_amd.build`")
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the ABI drifted from include/fsn_hip.h
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


class FsnTimeout(FsnError):
    """A persistent kernel ran out of time waiting for its partner workgroups (FSN_ERR_TIMEOUT, include/fsn_hip.h
    "residency contract"): its outputs are NaN and the stream refuses further persistent launches until
    `stream_status_clear()`."""


def check(rc):
    if rc == -4:
        raise FsnTimeout(f"libfsn_hip error {rc}: {lib().fsn_last_error().decode()}")
    if rc != 0:
        raise FsnError(f"libfsn_hip error {rc}: {lib().fsn_last_error().decode()}")


def stream_status(device=None, synchronize=True, raise_on_timeout=True):
    """(status, events) of the current stream of `device`: the sticky record of persistent launches that ran out of
    time (0, 0 = none).  Raises FsnTimeout when raised (unless raise_on_timeout is False)."""
    st, ev = ctypes.c_uint(0), ctypes.c_uint(0)
    rc = lib().fsn_stream_status(stream_ptr(device), 1 if synchronize else 0, ctypes.byref(st), ctypes.byref(ev))
    if rc != 0 and (raise_on_timeout or rc != -4):
        check(rc)
    return st.value, ev.value


def stream_status_clear(device=None):
    check(lib().fsn_stream_status_clear(stream_ptr(device)))


def stream_timeout_policy(policy, device=None):
    """"refuse" (default): a raised timeout record makes later persistent launches on the current stream of `device`
    fail with FsnTimeout until cleared.  "defer": they run regardless (a training step in flight; the poison is NaN,
    the fused optimizer skips, the caller reads `stream_status` once per step)."""
    check(lib().fsn_stream_timeout_policy(stream_ptr(device), {"refuse": 0, "defer": 1}[policy]))


def persist_stats():
    """(launches, waits, unreported) of the persistent-launch gate (test hook)."""
    v = [ctypes.c_uint(0) for _ in range(3)]
    check(lib().fsn_debug_persist_stats(*(ctypes.byref(x) for x in v)))
    return tuple(x.value for x in v)


def set_persistent_mode(mode):
    """"auto" (default) or "never": whether the kernels that need their whole grid resident may be used."""
    check(lib().fsn_set_persistent_mode({"auto": 0, "never": 1}[mode]))


def set_persistent_timeout_ms(ms):
    check(lib().fsn_set_persistent_timeout_ms(int(ms)))


def dev_ptr(t, name="tensor", allow_none=False):
    """Validated raw device pointer of a contiguous fp32 ROCm tensor."""
    if t is None:
        if allow_none:
            return None
        raise FsnError(f"{name} is None")
    if not t.is_cuda:
        raise FsnError(f"{name} must live on a ROCm device (got {t.device}); this path has no CPU implementation")
    if t.dtype != torch.float32:
        raise FsnError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise FsnError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_CANARY = 4096     # bytes of guard pattern behind every workspace when FSN_WS_CANARY is set (memory-safety runs)
_canaries = []      # (guarded tensor, payload bytes) not yet verified


def workspace(nbytes, device):
    """Workspace from PyTorch's caching allocator (the library never allocates).  With FSN_WS_CANARY in the environment
    (tools/gpu_run_nocache.sh) every workspace is followed by a guard pattern that `check_canaries` verifies: a kernel
    that writes beyond the size its `*_workspace_bytes` query promised is caught even when the overrun stays inside
    memory the process owns."""
    if nbytes <= 0:
        raise FsnError(f"workspace query failed: {lib().fsn_last_error().decode()}")
    if os.environ.get("FSN_WS_CANARY"):
        buf = torch.empty(nbytes + _CANARY, dtype=torch.uint8, device=device)
        buf[nbytes:].fill_(0xA5)
        _canaries.append((buf, nbytes))
        return buf[:nbytes]
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def check_canaries():
    """Verify and forget the guard patterns of the workspaces handed out since the last call (synchronises)."""
    bad = []
    while _canaries:
        buf, n = _canaries.pop()
        if not bool((buf[n:] == 0xA5).all()):
            bad.append(n)
    if bad:
        raise FsnError(f"workspace overrun: the guard behind workspaces of {bad} bytes was overwritten")


def profile_enable(on, device=None):
    """Per-stage hipEvent timing for calls made on the current stream of `device` (per stream: two callers do not
    race on it)."""
    check(lib().fsn_profile_enable(stream_ptr(device), 1 if on else 0))


def profile_stage_names():
    L = lib()
    return [L.fsn_profile_stage_name(i).decode() for i in range(L.fsn_profile_num_stages())]


def core_plan(cfg, B, T):
    """How the sub-band model of a B-utterance, T-frame call is spread over the device (fsn_debug_core_plan)."""
    buf = (ctypes.c_int * 9)()
    if lib().fsn_debug_core_plan(ctypes.byref(cfg), B, T, buf, 9) != 0:
        raise FsnError("fsn_debug_core_plan: bad arguments")
    keys = ("rows", "tiles", "row_tiles_per_workgroup", "persistent_workgroups", "left_over_tiles", "group_clusters",
            "fullband_chain", "chunks", "persistent_rows_all_chunks")  # the first seven: the FIRST chunk's plan
    return dict(zip(keys, list(buf)))


CORE_CALL_PLAN = ("rows", "tiles", "npad", "rt", "main_wgs", "left_tiles", "grp_clusters", "grp_aux_tiles", "cu_tiles",
                  "aux_tiles", "fb_chain", "npad_fb", "fc_fused", "l1x", "kin_chunks")
# bits of fsn_debug_core_last_launches, in the order of FsnTraceBit (csrc/fsn_common.h)
LAUNCH_BITS = ("lstm_rec", "lstm_rec_in", "lstm_rec_x", "lstm_step", "lstm_step_cu", "lstm_wavefront2", "lstm2_group", "fb_chain",
               "gemm_sb_proj", "gemm_sb_l1", "gemm_sb_out")


def core_call_plan(cfg, B, T, row_begin=0, row_end=-1):
    """The plan of ONE model-core call (fsn_debug_core_call_plan): the B utterances whole (row_end < 0; what a chunk of
    fsn_fullsubnet_forward runs) or the rows [row_begin, row_end) as fsn_fullsubnet_forward_rows forms them."""
    buf = (ctypes.c_int * len(CORE_CALL_PLAN))()
    if lib().fsn_debug_core_call_plan(ctypes.byref(cfg), B, T, row_begin, row_end, buf, len(buf)) != 0:
        raise FsnError("fsn_debug_core_call_plan: bad arguments")
    return dict(zip(CORE_CALL_PLAN, list(buf)))


def core_last_launches():
    """Names of the launchers (and sub-band GEMM sites) the last library call of THIS thread went through."""
    m = lib().fsn_debug_core_last_launches()
    return {name for k, name in enumerate(LAUNCH_BITS) if m >> k & 1}


STREAM_STATE_LAYOUT = ("fb_h0", "fb_h1", "fb_c0", "fb_c1", "sb_h0", "sb_h1", "sb_c0", "sb_c1", "fb_sum", "sb_sum", "npad_fb",
                       "npad_sb", "bytes")
STREAM_POOL_LAYOUT = ("fb_h0", "fb_h1", "fb_c0", "fb_c1", "sb_h0", "sb_h1", "sb_c0", "sb_c1", "fb_sum", "sb_sum", "steps",
                      "in_tail", "ola_tail", "ring_re", "ring_im", "slot_bytes", "F", "FP", "Hf", "Hs", "R")


def stream_state_layout(cfg, B):
    """Byte offsets of the arrays of the stream step's state blob at batch B, its padded row counts and its size
    (fsn_debug_stream_state_layout); the blob of the segment entries starts with the same arrays."""
    buf = (ctypes.c_long * len(STREAM_STATE_LAYOUT))()
    if lib().fsn_debug_stream_state_layout(ctypes.byref(cfg), B, buf, len(buf)) != 0:
        raise FsnError("fsn_debug_stream_state_layout: bad arguments")
    return dict(zip(STREAM_STATE_LAYOUT, list(buf)))


def stream_pool_layout(cfg):
    """Byte offsets into one record of the streaming pool, its size and dimensions (fsn_debug_stream_pool_layout)."""
    buf = (ctypes.c_long * len(STREAM_POOL_LAYOUT))()
    if lib().fsn_debug_stream_pool_layout(ctypes.byref(cfg), buf, len(buf)) != 0:
        raise FsnError("fsn_debug_stream_pool_layout: bad arguments")
    return dict(zip(STREAM_POOL_LAYOUT, list(buf)))


FAST_STREAM_STATE_LAYOUT = ("enc0_h", "enc0_c", "enc1_h", "enc1_c", "dec0_h", "dec0_c", "dec1_h", "dec1_c", "bn_h0", "bn_c0",
                            "bn_h1", "bn_c1", "mel_sum", "unit_sum", "partial", "held", "rows", "bn_rows", "enc1_hidden",
                            "unit_width", "bytes")


def fast_stream_state_layout(cfg, B):
    """Byte offsets of the fields of fsn_fast_stream_step's state blob at batch B (-1: a bottleneck layer the configuration
    does not have), its row counts, encoder.1's padded hidden size, the unit width and its size
    (fsn_debug_fast_stream_state_layout)."""
    buf = (ctypes.c_long * len(FAST_STREAM_STATE_LAYOUT))()
    if lib().fsn_debug_fast_stream_state_layout(ctypes.byref(cfg), B, buf, len(buf)) != 0:
        raise FsnError("fsn_debug_fast_stream_state_layout: bad arguments")
    return dict(zip(FAST_STREAM_STATE_LAYOUT, list(buf)))


FAST_SEGMENT_STATE_LAYOUT = FAST_STREAM_STATE_LAYOUT[:16] + ("acc_mel", "acc_unit", "stat_partial", "stream_end", "rows", "bn_rows",
                                                             "enc1_hidden", "unit_width", "bytes")


def fast_segment_state_layout(cfg, B):
    """Byte offsets of the fields of the fsn_fast_segment_* state blob at batch B: fsn_fast_stream_step's fields, then the two
    fp64 accumulators and the statistic pass's block sum; ``stream_end`` is where the stream step's fields end
    (fsn_debug_fast_segment_state_layout)."""
    buf = (ctypes.c_long * len(FAST_SEGMENT_STATE_LAYOUT))()
    if lib().fsn_debug_fast_segment_state_layout(ctypes.byref(cfg), B, buf, len(buf)) != 0:
        raise FsnError("fsn_debug_fast_segment_state_layout: bad arguments")
    return dict(zip(FAST_SEGMENT_STATE_LAYOUT, list(buf)))


def improved_stream_state_layout(cfg, B):
    """Byte offsets of the fields of fsn_improved_stream_step's state blob at batch B: ``fb`` [h0, c0, h1, c1], ``sb`` the same
    per section, ``fb_sum``, ``sb_sum`` [sections][B] and ``steps`` [B]; ``rows`` / ``sb_rows`` the padded row counts and
    ``bytes`` its size (fsn_debug_improved_stream_state_layout)."""
    buf = (ctypes.c_long * 50)()
    if lib().fsn_debug_improved_stream_state_layout(ctypes.byref(cfg), B, buf, len(buf)) != 0:
        raise FsnError("fsn_debug_improved_stream_state_layout: bad arguments")
    v, n = list(buf), buf[48]
    return {"fb": v[0:4], "sb": [v[4 + 4 * i:8 + 4 * i] for i in range(n)], "fb_sum": v[36], "sb_sum": v[37], "steps": v[38],
            "rows": v[39], "sb_rows": v[40:40 + n], "sections": n, "bytes": v[49]}


FAST_STREAM_POOL_LAYOUT = ("enc0_h", "enc0_c", "enc1_h", "enc1_c", "dec0_h", "dec0_c", "dec1_h", "dec1_c", "bn_h0", "bn_c0", "bn_h1",
                           "bn_c1", "mel_sum", "unit_sum", "partial", "held", "steps", "in_tail", "ola_tail", "ring_re", "ring_im",
                           "slot_bytes", "F", "FP", "R", "bn_hidden", "bn_layers", "unit_width")


def fast_stream_pool_layout(cfg, look_ahead):
    """Byte offsets into one record of Fast FullSubNet's streaming pool (-1: a bottleneck layer the configuration does not
    have), its size and dimensions (fsn_debug_fast_stream_pool_layout)."""
    buf = (ctypes.c_long * len(FAST_STREAM_POOL_LAYOUT))()
    if lib().fsn_debug_fast_stream_pool_layout(ctypes.byref(cfg), look_ahead, buf, len(buf)) != 0:
        raise FsnError("fsn_debug_fast_stream_pool_layout: bad arguments")
    return dict(zip(FAST_STREAM_POOL_LAYOUT, list(buf)))


def improved_stream_pool_layout(cfg):
    """Byte offsets into one record of Improved FullSubNet's streaming pool: ``fb`` [h0, c0, h1, c1], ``sb`` the same per
    section, ``fb_sum``, ``sb_sum`` (8 doubles), ``steps`` (a long), the transform fields ``in_tail`` / ``ola_tail`` [hop],
    ``spec_re`` / ``spec_im`` [F] and ``frame`` (an int); ``slot_bytes`` its size, and its dimensions
    (fsn_debug_improved_stream_pool_layout)."""
    buf = (ctypes.c_long * 58)()
    if lib().fsn_debug_improved_stream_pool_layout(ctypes.byref(cfg), buf, len(buf)) != 0:
        raise FsnError("fsn_debug_improved_stream_pool_layout: bad arguments")
    v, n = list(buf), buf[49]
    out = {"fb": v[0:4], "sb": [v[4 + 4 * i:8 + 4 * i] for i in range(n)], "sections": n, "units": v[50:50 + n]}
    out.update(zip(("fb_sum", "sb_sum", "steps", "in_tail", "ola_tail", "spec_re", "spec_im", "frame", "slot_bytes", "F", "hop",
                    "fb_hidden", "sb_hidden"), v[36:49]))
    return out


def profile_read(device=None):
    """Stage times (ms) of the last profiled call on the current stream of `device`."""
    L = lib()
    n = L.fsn_profile_num_stages()
    buf = (ctypes.c_float * n)()
    check(L.fsn_profile_read(stream_ptr(device), buf, n))
    return dict(zip(profile_stage_names(), list(buf)))
