"""Shared by the embedding plug-in tests: the four recorded settings of tests/golden/emb_plugin.npz
(tools/gen_emb_plugin_golden.py) and how to rebuild tokenizer, embedding file and module from a fixture."""
import hashlib
import importlib

import numpy as np
import torch

from conftest import PKG_NAME

D = 12
SETTINGS = {
    'reg': dict(fuse=0, temperature=1),
    'fixed': dict(fuse=0.3, temperature=2),
    'learn': dict(fuse=-1, temperature=-1),
    'vocab': dict(fuse=-2, temperature=-2, fuse_normalize=True, freeze=False),
}


def _mod(name):
    return importlib.import_module(PKG_NAME + "." + name)


def tokenizer(chars):
    return _mod("src.text").CharacterTextEncoder([str(c) for c in chars])


def write_embedding(lines, path):
    with open(path, "w") as f:
        f.write("\n".join(str(l) for l in lines) + "\n")
    return str(path)


def build(g, tag, tmp_path, dec_dim=D, seed=11, weight=None):
    """the module of setting `tag`, constructed from seed exactly as the generator constructed the reference's"""
    src = write_embedding(g["emb_lines"], tmp_path / "emb.txt")
    torch.manual_seed(seed)
    w = float(g["emb_weight"]) if weight is None else weight
    return _mod("src.plugin").EmbeddingRegularizer(tokenizer(g["chars"]), dec_dim, True, src, 'CosEmb', w,
                                                   **SETTINGS[tag])


def recorded_state(g, tag):
    pre = tag + ".param."
    return {k[len(pre):]: torch.from_numpy(v.copy()) for k, v in g.items() if k.startswith(pre)}


def digest(state_dict):
    h = hashlib.sha256()
    for k, v in state_dict.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v.detach().cpu().numpy().astype(np.float32)).tobytes())
    return h.hexdigest()
