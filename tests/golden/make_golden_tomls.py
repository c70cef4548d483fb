"""Fixture for tests/test_reference_tomls.py: what every TOML the reference ships (recipes/dns_interspeech_2020/*/*.toml)
says about its model, and what the reference class built from it looks like.  Run from the repo root with the path of
a reference checkout:   python tests/golden/make_golden_tomls.py <reference checkout>

Per TOML (keyed by its path relative to the recipe directory): [model].path and [model.args], the inferencer type,
whether a [trainer] section exists, and the reference class's state_dict (name -> shape, dtype) and parameter count -
or, where the reference class rejects its own TOML's arguments, the exception it raises.  Written to
tests/golden/reference_tomls.json.

fast_fullsubnet/model.py imports torchaudio and torchinfo (neither in the reference tree): the stubs of
make_golden_family.py, restated so that this script reads only the checkout it is given.
"""
import glob
import json
import os
import sys
import types

import numpy as np
import tomli
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import model_family_oracle as MF  # noqa: E402


class _MelScale(torch.nn.Module):
    def __init__(self, n_mels, sample_rate, f_min, f_max, n_stft):
        super().__init__()
        fb = MF.melscale_fbanks(n_stft, f_min, f_max, n_mels, sample_rate).astype(np.float32)
        self.register_buffer("fb", torch.from_numpy(fb))

    def forward(self, specgram):
        return torch.matmul(specgram.transpose(-1, -2), self.fb).transpose(-1, -2)


def _install_stubs():
    ta = types.ModuleType("torchaudio")
    ta.transforms = types.ModuleType("torchaudio.transforms")
    ta.transforms.MelScale = _MelScale
    ti = types.ModuleType("torchinfo")
    ti.summary = lambda *a, **k: None
    sys.modules.update({"torchaudio": ta, "torchaudio.transforms": ta.transforms, "torchinfo": ti})
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))  # feature.py:3, used by load_wav only


def main(ref):
    recipe_dir = os.path.join(ref, "recipes", "dns_interspeech_2020")
    _install_stubs()
    for p in (ref, recipe_dir):
        sys.path.insert(0, p)
    out = {}
    for path in sorted(glob.glob(os.path.join(recipe_dir, "*", "*.toml"))):
        rel = os.path.relpath(path, recipe_dir)
        recipe = rel.split(os.sep)[0]
        with open(path, "rb") as f:
            cfg = tomli.load(f)
        mod = __import__(f"{recipe}.model", fromlist=["Model"])
        entry = {"recipe": recipe, "model_path": cfg["model"]["path"], "model_args": cfg["model"]["args"],
                 "inferencer_type": cfg.get("inferencer", {}).get("type"), "has_trainer": "trainer" in cfg}
        torch.manual_seed(0)
        try:
            m = mod.Model(**cfg["model"]["args"])
        except TypeError as e:
            entry["reference_raises"] = type(e).__name__
        else:
            entry["state_dict"] = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()}
            entry["num_parameters"] = int(sum(p.numel() for p in m.parameters()))
        out[rel.replace(os.sep, "/")] = entry
    dst = os.path.join(HERE, "reference_tomls.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{dst}: {len(out)} TOMLs")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(os.path.abspath(sys.argv[1]))
