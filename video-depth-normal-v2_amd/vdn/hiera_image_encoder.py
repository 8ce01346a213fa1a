"""Drop-in for models/hiera_image_encoder.py:5-61 (HieraImageEncoder): same constructor, methods and state-dict keys; the
forward pass runs on libvdn_hip.so (vdn/hiera_engine.py, csrc/hiera.hip), never on torch ops, and nothing is fetched.

The reference holds the torch.hub model as `self.model`, so its checkpoints carry `model.<hub key>`; the parameters here
sit under the same names. The hub names below are written from the published Hiera code as remembered and could not be
checked against it offline; they live in ONE table, RENAME, next to the names of the `transformers` port of
the same model, which tools/make_golden_hiera.py verifies by loading that port through it."""
from __future__ import annotations

import re

import torch
import torch.nn as nn

from . import modules
from .depth_anything_v2 import _EngineOwner
from .hiera_engine import EMBED_DIM, HEADS, TOKENS, HieraEngine

DEPTHS = {"hiera_tiny_224": (1, 2, 7, 2), "hiera_small_224": (1, 2, 11, 2), "hiera_base_224": (2, 3, 16, 3)}
# names models/hiera_image_encoder.py:22-29 accepts whose stage widths (112.. / 144.. / 256..) are not the head's 96..768
TOO_WIDE = ("hiera_base_plus_224", "hiera_large_224", "hiera_huge_224")
NUM_CLASSES = 1000

# (hub name, `transformers` HieraModel name): top-level parameters, then the members of a block. A correction of a hub name
# touches this table alone.
RENAME_TOP = (("patch_embed.proj", "embeddings.patch_embeddings.projection"), ("pos_embed", "embeddings.position_embeddings"))
RENAME_BLOCK = (("norm1", "layernorm_before"), ("attn.qkv", "attn.qkv"), ("attn.proj", "attn.proj"), ("norm2", "layernorm_after"),
                ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2"), ("proj", "proj"))
UNPORTED = ("norm", "head.projection")   # classifier end of the hub model: held for strict loading, never used


def transformers_key(key: str, depths) -> str | None:
    """The `transformers` HieraModel name of hub key `key` ('blocks.5.attn.qkv.weight' -> 'encoder.stages.2.layers.0.attn.qkv
    .weight'), or None for the classifier end, which that port's trunk does not have."""
    for hub, tf in RENAME_TOP:
        if key == hub or key.startswith(hub + "."):
            return tf + key[len(hub):]
    m = re.match(r"blocks\.(\d+)\.(.+)\.(weight|bias)$", key)
    if m:
        n, member = int(m.group(1)), m.group(2)
        for s, d in enumerate(depths):
            if n < d:
                break
            n -= d
        return f"encoder.stages.{s}.layers.{n}.{dict(RENAME_BLOCK)[member]}.{m.group(3)}"
    if key.startswith(UNPORTED):
        return None
    raise KeyError(key)


def _hub_model(depths) -> nn.Module:
    """Parameter holder with the hub model's module tree (zeros until a state dict is loaded)."""
    m = modules.Holder()
    m.patch_embed = modules.Holder()
    m.patch_embed.proj = modules.Conv(3, EMBED_DIM, 7)
    m.pos_embed = modules._param(1, TOKENS, EMBED_DIM)
    m.blocks = nn.ModuleList()
    cin = EMBED_DIM
    for s, depth in enumerate(depths):
        c = EMBED_DIM << s
        for i in range(depth):
            b = modules.Holder()
            b.norm1 = modules.Norm(cin)
            b.attn = modules.Holder()
            b.attn.qkv = modules.Lin(cin, 3 * c)
            b.attn.proj = modules.Lin(c, c)
            b.norm2 = modules.Norm(c)
            b.mlp = modules.Holder()
            b.mlp.fc1 = modules.Lin(c, 4 * c)
            b.mlp.fc2 = modules.Lin(4 * c, c)
            if cin != c:
                b.proj = modules.Lin(cin, c)
            m.blocks.append(b)
            cin = c
    m.norm = modules.Norm(cin)
    m.head = modules.Holder()
    m.head.projection = modules.Lin(cin, NUM_CLASSES)
    return m


class HieraImageEncoder(_EngineOwner):
    def __init__(self, model_name: str = "hiera_base_224", finetune: bool = True):
        super().__init__()
        if model_name in TOO_WIDE:
            raise NotImplementedError(
                f"{model_name}: its stage widths do not feed the depth + normal head, whose feature channels are "
                f"{[EMBED_DIM << s for s in range(4)]}; supported trunks: {sorted(DEPTHS)}")
        if model_name not in DEPTHS:
            raise ValueError(f"Unsupported model: {model_name}")
        self.model_name = model_name
        self.depths = DEPTHS[model_name]
        self.model = _hub_model(self.depths)
        self._rt_owner = ()   # (other trunk,) after share_runtime; a tuple, so that it is not registered as a submodule
        self.set_finetune(finetune)

    def set_finetune(self, finetune: bool):
        """Training is out of scope: only the requires_grad flags change."""
        self.finetune = finetune
        for p in self.parameters():
            p.requires_grad_(bool(finetune))

    def share_runtime(self, other: "HieraImageEncoder"):
        """Run on `other`'s Runtime (its precision and workspace arena) instead of one of its own: two trunks of one model run
        one after the other on the same stream, so one set of activation buffers serves both."""
        self._rt_owner, self._eng = (other,), None
        return self

    def _engines(self):
        rt = self._rt_owner[0]._engines()["rt"] if self._rt_owner else None
        if self._eng is None or (rt is not None and self._eng["rt"] is not rt):
            rt = rt or self._runtime()
            self._eng = dict(rt=rt, trunk=HieraEngine(rt, self.model, self.depths))
        return self._eng

    @torch.no_grad()
    def forward(self, x: torch.Tensor, taps: bool = False):
        """x f32 [N, 3, 224, 224] -> (None, [f32 NHWC [N, 56, 56, 96], [N, 28, 28, 192], [N, 14, 14, 384], [N, 7, 7, 768]]).
        The first element stands for the classifier output, which the model ignores (hiera_image_encoder.py:53)."""
        if x.dim() != 4 or x.shape[1] != 3 or tuple(x.shape[-2:]) != (224, 224):
            raise ValueError(f"expected [N, 3, 224, 224] (pos_embed holds {TOKENS} tokens: no other size), got {tuple(x.shape)}")
        e = self._engines()
        rt = e["rt"]
        x = x.to(device=rt.device, dtype=torch.float32).contiguous()
        N = x.shape[0]
        outs = [torch.empty((N, 56 >> s, 56 >> s, EMBED_DIM << s), dtype=torch.float32, device=rt.device) for s in range(len(HEADS))]
        e["trunk"].run(x, outs, taps=taps)
        self._taps = e["trunk"].taps
        return None, outs


__all__ = ["HieraImageEncoder", "DEPTHS", "transformers_key"]
