"""Launch sequence of the Hiera trunk (hiera_{tiny,small,base}_224 of the published Hiera code, as
models/hiera_image_encoder.py:35,60 runs it: inference, no masking, return_intermediates): every op between the input
frames and the four stage maps is a libvdn_hip.so launch, every buffer but the four results comes from the Runtime arena.

Token layout: one f32 residual stream [frames*T, C] per stage, a frame's T tokens in the model's unrolled order
(include/vdn.h, csrc/hiera.hip), so the 2 x 2 max-pools of the width-changing blocks are maxima over the 4 contiguous
quarters of a frame and the mask-unit windows are the rows t*W + w. Only the stage ends are put back in row-major order
(vdn_hiera_reroll), straight into the NHWC maps vdn_dn_prologue reads.
"""
from __future__ import annotations

from typing import List

import torch

from . import _abi as abi
from . import pack
from .runtime import Runtime

EMBED_DIM = 96
HEAD_DIM = 96
HEADS = (1, 2, 4, 8)
SIDE = 56                 # 224 / 4
TOKENS = SIDE * SIDE      # 3136
MASK_UNIT = 64            # 8 x 8 tokens: 49 windows
LN_EPS = 1e-6
K_PATCH = 147             # 3 * 7 * 7
LDK_PATCH = 192           # padded to the plane stride


def unroll_index(n: int = 3) -> torch.Tensor:
    """perm [T]: unrolled token u of a stage with n stride-2 levels left holds row-major token perm[u] of its
    (7 << n)-sided grid. The host-side statement of csrc/hiera.hip's index map."""
    side = 7 << n
    idx = torch.arange(side * side).reshape(1, side, side)
    for _ in range(n):   # one level: [b, h/2, 2, w/2, 2] -> [b, 2, 2, h/2, w/2], the 2 x 2 phase joins the leading digits
        b, h, w = idx.shape
        idx = idx.reshape(b, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3).reshape(b * 4, h // 2, w // 2)
    return idx.reshape(-1)


def attn_geometry(stage: int, first: bool):
    """(windows W, L_kv, q_stride) of a block: stages 0 and 1 attend inside the 49 mask units, the first block of stage 2
    inherits that windowing, everything after is global; the first block of stages 1..3 pools its queries 4 : 1."""
    tokens_in = TOKENS >> (2 * (stage - 1 if first and stage > 0 else stage))
    qs = 4 if first and stage > 0 else 1
    windowed = stage < 2 or (stage == 2 and first)
    W = TOKENS // MASK_UNIT if windowed else 1
    return W, tokens_in // W, qs


class HieraEngine:
    def __init__(self, rt: Runtime, model, depths):
        self.rt = rt
        h = rt.prec
        self.depths = tuple(int(d) for d in depths)
        pe = model.patch_embed.proj
        self.w_patch = pack.patch_embed(pe.weight, h)                    # [96, 147 -> 192]
        assert self.w_patch.hi.shape[1] == LDK_PATCH, self.w_patch.hi.shape
        self.b_patch = pack.f32(pe.bias)
        perm = unroll_index(3).to(model.pos_embed.device)
        self.pos = pack.f32(model.pos_embed.detach()[0][perm])           # pos_embed in unrolled order, once
        self.blocks = []
        n = 0
        for s, depth in enumerate(self.depths):
            for i in range(depth):
                b = model.blocks[n]
                first = i == 0
                k = dict(stage=s, first=first, geo=attn_geometry(s, first),
                         n1w=pack.f32(b.norm1.weight), n1b=pack.f32(b.norm1.bias), n2w=pack.f32(b.norm2.weight), n2b=pack.f32(b.norm2.bias),
                         wqkv=pack.linear(b.attn.qkv.weight, h), bqkv=pack.f32(b.attn.qkv.bias),
                         wo=pack.linear(b.attn.proj.weight, h), bo=pack.f32(b.attn.proj.bias),
                         w1=pack.linear(b.mlp.fc1.weight, h), b1=pack.f32(b.mlp.fc1.bias),
                         w2=pack.linear(b.mlp.fc2.weight, h), b2=pack.f32(b.mlp.fc2.bias))
                if first and s > 0:
                    k.update(wp=pack.linear(b.proj.weight, h), bp=pack.f32(b.proj.bias))
                self.blocks.append(k)
                n += 1
        self.taps = {}

    def _block(self, k: dict, x: torch.Tensor, F: int):
        """One block on the f32 stream x [F*T_in, C_in]; returns the stream it leaves ([F*T_out, C_out]; x itself unless
        the block changes width)."""
        rt = self.rt
        s = k["stage"]
        C = EMBED_DIM << s
        W, Lkv, qs = k["geo"]
        Tin = W * Lkv
        Tout = Tin // qs
        Cin = C // 2 if qs > 1 else C
        rin, rout = F * Tin, F * Tout
        n = rt.hbuf(f"hi_n{Cin}_{Tin}", (rin, Cin))
        rt.layernorm(x, rin, Cin, k["n1w"], k["n1b"], LN_EPS, out_h=n)
        if qs > 1:   # residual = max over the 4 token groups of proj(norm1(x))
            p = rt.fbuf(f"hi_p{s}", (rin, C))
            rt.gemm(n, k["wp"], rin, C, Cin, bias=k["bp"], out=p)
            x = rt.fbuf(f"hi_x{s}", (rout, C))
            rt.hiera_pool(p, x, F, Tout, C)
        qkv = rt.hbuf(f"hi_qkv{s}_{Tin}", (rin, 3 * C))
        rt.gemm(n, k["wqkv"], rin, 3 * C, Cin, bias=k["bqkv"], out=qkv)
        a = rt.hbuf(f"hi_a{s}", (rout, C))
        rt.hiera_attn(qkv, a, F, HEADS[s], W, Lkv, qs, HEAD_DIM ** -0.5)
        rt.gemm(a, k["wo"], rout, C, C, bias=k["bo"], res1=x, out=x)
        n2 = rt.hbuf(f"hi_n{C}_{Tout}", (rout, C))
        rt.layernorm(x, rout, C, k["n2w"], k["n2b"], LN_EPS, out_h=n2)
        hid = rt.hbuf(f"hi_h{s}", (rout, 4 * C))
        rt.gemm(n2, k["w1"], rout, 4 * C, C, bias=k["b1"], act=abi.ACT_GELU, out=hid)
        rt.gemm(hid, k["w2"], rout, C, 4 * C, bias=k["b2"], res1=x, out=x)
        return x

    def run(self, img: torch.Tensor, outs: List[torch.Tensor], taps: bool = False):
        """img f32 [F, 3, 224, 224] -> outs[s] f32 NHWC [F, 56 >> s, 56 >> s, 96 << s]. With `taps` the unrolled streams after
        the embedding ('embed') and after each stage's first block ('first{s}') are kept as clones (tests)."""
        rt = self.rt
        F = int(img.shape[0])
        rows = rt.hbuf("hi_rows", (F * TOKENS, LDK_PATCH))
        rt.hiera_embed(img, rows, F, LDK_PATCH)
        x = rt.fbuf("hi_x0", (F * TOKENS, EMBED_DIM))
        rt.gemm(rows, self.w_patch, F * TOKENS, EMBED_DIM, LDK_PATCH, bias=self.b_patch, tab=self.pos, tab_mod=TOKENS, out=x)
        self.taps = {}
        if taps:
            self.taps["embed"] = x.clone()
        for i, k in enumerate(self.blocks):
            x = self._block(k, x, F)
            if taps and k["first"]:
                self.taps[f"first{k['stage']}"] = x.clone()
            if i + 1 == len(self.blocks) or self.blocks[i + 1]["stage"] != k["stage"]:
                rt.hiera_reroll(x, outs[k["stage"]], F, k["stage"], EMBED_DIM << k["stage"])
