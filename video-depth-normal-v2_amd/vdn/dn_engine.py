"""Launch sequence of the depth + normal head (models/video_depth_head_v2_sangyu.py:187-317) and the tail of its wrapper
(models/video_depth_model.py:64-123): every op after the caller's trunks is a libvdn_hip.so launch, every buffer comes
from the Runtime arena (nothing allocated per call after warm-up).

Token layout: one [B*S*h*w, C] row matrix per level, frame-major and channel-last (csrc/dn_head.hip vdn_dn_prologue).
Spatial attention sequences are a frame's h*w consecutive rows, temporal ones the S rows h*w apart; the decoder's
convolutions read the same rows as NHWC maps, so no rearrange exists anywhere after the prologue.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from . import _abi as abi
from . import pack
from .runtime import Runtime

CHANNELS = [96, 192, 384, 768]   # video_depth_head_v2_sangyu.py:203
HEADS = 8
LN_EPS = 1e-5
BN_EPS = 1e-5
STACKS = ("temporal_layers_first", "spatial_layers_first", "temporal_layers_second", "spatial_layers_second")  # :281-284


def _fold(conv, bn):
    """Eval-mode BatchNorm2d after a bias-free conv: a per-channel affine map folded into the conv's weights."""
    w = conv.weight.detach().float()
    sc = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + BN_EPS)
    b = bn.bias.detach().float() - bn.running_mean.detach().float() * sc
    if conv.bias is not None:
        b = b + conv.bias.detach().float() * sc
    return w * sc[:, None, None, None], b.contiguous()


class DNHeadEngine:
    def __init__(self, rt: Runtime, head):
        self.rt = rt
        h = rt.prec
        self.levels = sorted(set(int(l) for l in head.attention_feature_levels))
        self.seq_len = None
        self.ape = [None] * 4
        if head.pos_embeds is not None:
            self.ape = [pack.f32(p) for p in head.pos_embeds]
            self.seq_len = int(head.pos_embeds[0].shape[0])
        self.blocks = {}
        for lvl in self.levels:
            stacks = []
            for name in STACKS:
                blks = []
                for b in getattr(head, name)[lvl].transformer_blocks:
                    m = b.multi_head_attention
                    blks.append(dict(
                        n1w=pack.f32(b.norm1.weight), n1b=pack.f32(b.norm1.bias), n2w=pack.f32(b.norm2.weight), n2b=pack.f32(b.norm2.bias),
                        win=pack.linear(m.in_proj_weight, h), bin=pack.f32(m.in_proj_bias),
                        wo=pack.linear(m.out_proj.weight, h), bo=pack.f32(m.out_proj.bias),
                        w1=pack.linear(b.ffn[0].weight, h), b1=pack.f32(b.ffn[0].bias),
                        w2=pack.linear(b.ffn[2].weight, h), b2=pack.f32(b.ffn[2].bias)))
                stacks.append((name.startswith("temporal"), blks))
            self.blocks[lvl] = stacks
        self.up = []
        for u in head.upscale_layers:
            w, b = _fold(u.conv[0], u.conv[1])
            self.up.append(dict(wc=pack.conv3x3(w, h), bc=b, wsk=pack.conv1x1(u.skip_proj.weight, h), bsk=pack.f32(u.skip_proj.bias)))
        f = head.final_upscale_layer
        w1, b1 = _fold(f[1], f[2])
        w2, b2 = _fold(f[5], f[6])
        self.fin = [(pack.conv3x3(w1, h), b1), (pack.conv3x3(w2, h), b2), (pack.conv3x3(f[8].weight, h), pack.f32(f[8].bias))]
        self.w_out, self.b_out = pack.f32(f[10].weight), pack.f32(f[10].bias)
        self.c_mid = int(f[8].weight.shape[0])   # 48

    # ------------------------------------------------------------------------------------------ transformer stacks
    def _stacks(self, lvl: int, x: torch.Tensor, B: int, S: int, hw: int):
        """_maybe_process (:267-285) after the position term: 4 stacks x 4 pre-LN TransformerBlocks (:58-75) on the f32
        residual stream x [B*S*hw, C], in place."""
        rt = self.rt
        C = CHANNELS[lvl]
        rows = B * S * hw
        scale = (C // HEADS) ** -0.5
        n = rt.hbuf(f"dn_n{lvl}", (rows, C))
        qkv = rt.hbuf(f"dn_qkv{lvl}", (rows, 3 * C))
        a = rt.hbuf(f"dn_a{lvl}", (rows, C))
        hid = rt.hbuf(f"dn_h{lvl}", (rows, 4 * C))
        for temporal, blks in self.blocks[lvl]:
            if temporal:   # "(b h w) s c": pixel p of clip b, its S frames h*w rows apart
                geo = dict(L=S, estride=hw, n0=hw, s0=1, n1=B, s1=S * hw)
            else:          # "(b s) (h w) c": one frame's h*w consecutive rows
                geo = dict(L=hw, estride=1, n0=1, s0=0, n1=B * S, s1=hw)
            for k in blks:
                rt.layernorm(x, rows, C, k["n1w"], k["n1b"], LN_EPS, out_h=n)
                rt.gemm(n, k["win"], rows, 3 * C, C, bias=k["bin"], out=qkv)
                rt.dn_attn(qkv, a, rows, C, HEADS, scale=scale, **geo)
                rt.gemm(a, k["wo"], rows, C, C, bias=k["bo"], res1=x, out=x)
                rt.layernorm(x, rows, C, k["n2w"], k["n2b"], LN_EPS, out_h=n)
                rt.gemm(n, k["w1"], rows, 4 * C, C, bias=k["b1"], act=abi.ACT_GELU, out=hid)
                rt.gemm(hid, k["w2"], rows, C, 4 * C, bias=k["b2"], res1=x, out=x)

    def tokens(self, a: Sequence[torch.Tensor], b: Optional[Sequence[torch.Tensor]], B: int, S: int, sizes):
        """Per level: prologue (+ the attention stacks on attention levels) -> half token planes [B*S*h*w, C]."""
        rt = self.rt
        if self.seq_len is not None and S > self.seq_len:
            raise ValueError(f"{S} frames exceed the head's sequence_length {self.seq_len} (pos_embeds)")
        F = B * S
        toks = []
        for lvl in range(4):
            C, (h, w) = CHANNELS[lvl], sizes[lvl]
            hw, rows = h * w, F * h * w
            bb = None if b is None else b[lvl]
            t = rt.hbuf(f"dn_tok{lvl}", (rows, C))
            if lvl in self.levels:
                x = rt.fbuf(f"dn_x{lvl}", (rows, C))
                rt.dn_prologue(a[lvl], bb, F, C, hw, ape=self.ape[lvl], S=S, out_f=x)
                self._stacks(lvl, x, B, S, hw)
                rt.addtab_cast(x, None, 1, 1, t, rows, C)
            else:
                rt.dn_prologue(a[lvl], bb, F, C, hw, out_h=t)
            toks.append(t)
        return toks

    # ------------------------------------------------------------------------------------------ decoder
    def _conv3(self, x, w, F: int, H: int, W: int, Cin: int, Cout: int, name: str, bias, act=abi.ACT_RELU, res1=None, f32_out=False):
        rt = self.rt
        out = (rt.fbuf if f32_out else rt.hbuf)(name, (F * H * W, Cout))
        rt.gemm(x, w, F * H * W, Cout, 9 * Cin, out=out, bias=bias, act=act, res1=res1,
                conv=dict(B=F, H=H, W=W, C=Cin, OH=H, OW=W, stride=1))
        return out

    def decode(self, toks: List, F: int, sizes):
        """upscale_layers (UpSampleAdd, :17-31) and final_upscale_layer up to its 48-channel ReLU (:242-249):
        f32 NHWC [F, 4 h0, 4 w0, 48]."""
        rt = self.rt
        x = toks[3]
        for i, (up, lo) in enumerate(zip(self.up, (2, 1, 0))):
            Cin, Co = CHANNELS[lo + 1], CHANNELS[lo]
            (h, w), (H, W) = sizes[lo + 1], sizes[lo]
            if (H, W) != (2 * h, 2 * w):
                raise ValueError(f"level {lo} is {H}x{W}, not twice level {lo + 1} ({h}x{w})")
            M = F * H * W
            u = rt.hbuf(f"dn_u{i}", (M, Cin))
            rt.upsample(x, u, F, h, w, H, W, Cin)
            sk = rt.fbuf(f"dn_sk{i}", (M, Co))
            rt.gemm(toks[lo], up["wsk"], M, Co, Co, bias=up["bsk"], out=sk)
            x = self._conv3(u, up["wc"], F, H, W, Cin, Co, f"dn_y{i}", up["bc"], res1=sk)
        h, w = sizes[0]
        C0 = CHANNELS[0]
        for j in range(2):
            u = rt.hbuf(f"dn_fu{j}", (F * 4 * h * w, C0))
            rt.upsample(x, u, F, h, w, 2 * h, 2 * w, C0)
            h, w = 2 * h, 2 * w
            x = self._conv3(u, self.fin[j][0], F, h, w, C0, C0, f"dn_fc{j}", self.fin[j][1])
        y = self._conv3(x, self.fin[2][0], F, h, w, C0, self.c_mid, "dn_fc2", self.fin[2][1], f32_out=True)
        return y, (h, w)

    def run_head(self, feats: Sequence[torch.Tensor], out: torch.Tensor):
        """VideoDepthAnythingHeadV2.forward: four f32 [B, S, C, h, w] maps -> out f32 [B, S, 3, 4 h0, 4 w0]."""
        B, S = feats[0].shape[:2]
        sizes = [tuple(f.shape[-2:]) for f in feats]
        toks = self.tokens(feats, None, B, S, sizes)
        y, (H, W) = self.decode(toks, B * S, sizes)
        self.rt.dn_tail(y, B * S, H, W, self.c_mid, self.w_out, self.b_out, H, W, raw=out)
        return toks

    def run_model(self, a, b, B: int, S: int, sizes, OH: int, OW: int, depth_in, relu: bool, depth, normal):
        """The wrapper after its trunks: features -> head -> resize / residual / ReLU / normal (video_depth_model.py:89-123).
        a, b: per level a contiguous f32 tensor of B*S frames, the trunk's own output or rows [start, start + S) of the clip
        driver's feature cache (VideoDepthEstimationModel.infer_video), which have the same layout."""
        toks = self.tokens(a, b, B, S, sizes)
        y, (H, W) = self.decode(toks, B * S, sizes)
        self.rt.dn_tail(y, B * S, H, W, self.c_mid, self.w_out, self.b_out, OH, OW, depth_in=depth_in, relu=relu, depth=depth,
                        normal=normal)
        return toks
