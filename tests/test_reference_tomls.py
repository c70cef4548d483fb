"""Every TOML the reference ships (recipes/dns_interspeech_2020/*/*.toml) names a model class and its keyword
arguments; `initialize_module(path, args)` (audio_zen/utils.py:70-105) builds the class from them.  The drop-in
contract: each `[model.args]` table instantiates the corresponding fullsubnet_amd class unchanged, with the
reference's parameter names, shapes and counts.  What the TOMLs say and what the reference classes built from them look
like is stored in tests/golden/reference_tomls.json (made by tests/golden/make_golden_tomls.py).  CPU only."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tomls.json")
with open(GOLDEN) as _f:
    TOMLS = json.load(_f)

# [model].path of the TOML (relative to its recipe directory or absolute) -> the class here
OURS = {"fullsubnet": "fullsubnet_amd.model.Model", "fast_fullsubnet": "fullsubnet_amd.fast_fullsubnet.Model",
        "fullband_baseline": "fullsubnet_amd.fullband_baseline.Model"}
# the reference's own stale file: its [model.args] (n_freqs, use_offline_laplace_norm ...) are not the keywords of
# fullband_baseline/model.py:9-18 - the reference class rejects them too
STALE = {"fullband_baseline/inference.toml"}


def _load(dotted):
    mod, cls = dotted.rsplit(".", 1)
    return getattr(__import__(mod, fromlist=[cls]), cls)


def test_the_reference_ships_the_tomls_this_file_expects():
    assert len(TOMLS) == 9, sorted(TOMLS)
    assert {rel for rel, t in TOMLS.items() if "reference_raises" in t} == STALE


@pytest.mark.parametrize("rel", sorted(TOMLS))
def test_shipped_toml_instantiates_the_drop_in_class(rel):
    cfg = TOMLS[rel]
    recipe = rel.split("/")[0]
    args = cfg["model_args"]
    assert cfg["model_path"].endswith("model.Model")
    ours_cls = _load(OURS[recipe])
    if rel in STALE:
        assert cfg["reference_raises"] == "TypeError"  # the reference class rejects them
        with pytest.raises(TypeError):
            ours_cls(**args)
        return
    torch.manual_seed(0)
    ours = ours_cls(**args)
    want = {k: tuple(v[0]) for k, v in cfg["state_dict"].items()}
    got = {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    assert got == want  # names and shapes: strict load_state_dict works in both directions
    assert {k: str(v.dtype).replace("torch.", "") for k, v in ours.state_dict().items()} == \
        {k: v[1] for k, v in cfg["state_dict"].items()}
    assert sum(p.numel() for p in ours.parameters()) == cfg["num_parameters"]
    # a state_dict of the reference's names, shapes and dtypes loads strictly, and ours round-trips
    g = torch.Generator().manual_seed(1)
    theirs = {k: torch.randn(tuple(s), generator=g).to(getattr(torch, dt)) for k, (s, dt) in cfg["state_dict"].items()}
    ours.load_state_dict(theirs, strict=True)
    assert all(torch.equal(ours.state_dict()[k], v) for k, v in theirs.items())
    # the inferencer / trainer sections name classes as well: their mirrors exist with the same entry points
    if cfg["inferencer_type"] is not None:  # */inference*.toml:8-13: the inference mode is a method name of the Inferencer
        from fullsubnet_amd.inferencer import Inferencer
        assert callable(getattr(Inferencer, cfg["inferencer_type"]))
    if cfg["has_trainer"]:
        from fullsubnet_amd.trainer import Trainer
        assert hasattr(Trainer, "_train_epoch") and hasattr(Trainer, "_validation_epoch")
