"""Executors: the reference's forward passes as sequences of libvdn_hip.so launches.

Data layout in HBM (everything channels-last, resident for the whole forward):
  residual streams (ViT tokens, memory-attention state, temporal hidden state)  f32 [rows, C]
  GEMM operands / activations between convs                                      half [rows, C]
  attention operands   Q,K  half [B*heads, tpad, 64];  V^T half [B*heads, 64, tpad]
  memory bank          per layer ring of projected+rotated K / V^T (6 slots), written once per frame
Every sequence is written once for both GEMM kernels. A linear that can take the 8-bit cross-term kernel (csrc/gemm_x8.hip;
DESIGN.md §3) holds its weight as a pack.Linear, and the activations around it come from Runtime.operand: split planes, or for
a call with enough rows (Runtime.x8_rows) the K-tile-major form (runtime.KT). layernorm, gemm and flash_attn read the form off
the operand.
Every function cites the reference code it stands for (paths relative to the reference root).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch

from . import _abi as abi
from . import pack
from .runtime import HL, Runtime, ceil_to

GELU, RELU = abi.ACT_GELU, abi.ACT_RELU
PATCH = 14


# =============================================================================================
class EncoderEngine:
    """DINOv2 ViT: depth_anything_v2/dinov2.py:212-231,271-321 + dinov2_layers/{block,attention,mlp}.py."""

    def __init__(self, rt: Runtime, mod, cfg: dict):
        self.rt, self.cfg = rt, cfg
        self.C, self.heads, self.depth, self.taps = cfg["dim"], cfg["heads"], cfg["depth"], cfg["taps"]
        h = rt.prec
        self.w_patch = pack.patch_embed(mod.patch_embed.proj.weight, h)
        self.b_patch = pack.f32(mod.patch_embed.proj.bias)
        self.cls = pack.f32(mod.cls_token).reshape(-1)
        self.pos = pack.f32(mod.pos_embed).reshape(-1, self.C)  # [1+37*37, C]
        self.blocks = []
        self.hidden = cfg.get("swiglu") or 4 * self.C   # FFN width: Mlp 4C, or the SwiGLU hidden size of ViT-g
        # 8-bit cross terms for the four linears of a block (csrc/gemm_x8.hip): K-tile-major weight planes made
        # once here, in the order of the kernel that writes each linear's input. SwiGLU has no cross-term path.
        self.x8 = rt.x8_capable(self.C) and not cfg.get("swiglu")

        def lin(w, order):
            return pack.Linear(pack.linear(w, h), order if self.x8 else None)

        for b in mod.blocks:
            blk = dict(
                n1w=pack.f32(b.norm1.weight), n1b=pack.f32(b.norm1.bias),
                wqkv=lin(b.attn.qkv.weight, pack.ORDER_NATURAL), bqkv=pack.f32(b.attn.qkv.bias),
                wproj=lin(b.attn.proj.weight, pack.ORDER_ATTN), bproj=pack.f32(b.attn.proj.bias),
                ls1=pack.f32(b.ls1.gamma),
                n2w=pack.f32(b.norm2.weight), n2b=pack.f32(b.norm2.bias),
                ls2=pack.f32(b.ls2.gamma))
            if cfg.get("swiglu"):
                # SwiGLU (swiglu_ffn.py:29-33): silu(x1) * x2 with [x1 ; x2] = w12 x. The gated epilogue computes
                # h * act(gate) from rows packed [h ; gate], so the halves are swapped: h = x2, gate = x1, act = SiLU.
                Hd = cfg["swiglu"]
                w12, b12 = b.mlp.w12.weight, b.mlp.w12.bias
                blk["wfc1"], blk["bfc1"] = pack.geglu(torch.cat([w12[Hd:], w12[:Hd]]), torch.cat([b12[Hd:], b12[:Hd]]), h)
                blk["wfc2"], blk["bfc2"] = pack.linear(b.mlp.w3.weight, h), pack.f32(b.mlp.w3.bias)
            else:
                blk["wfc1"], blk["bfc1"] = lin(b.mlp.fc1.weight, pack.ORDER_NATURAL), pack.f32(b.mlp.fc1.bias)
                blk["wfc2"], blk["bfc2"] = lin(b.mlp.fc2.weight, pack.ORDER_GEMM), pack.f32(b.mlp.fc2.bias)
            self.blocks.append(blk)
        self.nw, self.nb = pack.f32(mod.norm.weight), pack.f32(mod.norm.bias)
        self._pos_cache = {}
        # per-layer precision budget (include/vdn.h x8_terms; profiles/r03_precision_budget.md): VDN_X8_TERMS = "fc2=1,proj=1@12-23"
        # drops a cross term of the named linears (1: A_lo W_hi^T, 2: A_hi W_lo^T), optionally for blocks a..b only
        self.x8_terms = [dict(qkv=0, proj=0, fc1=0, fc2=0) for _ in self.blocks]
        for item in filter(None, os.environ.get("VDN_X8_TERMS", "").split(",")):
            name, val = item.split("=")
            val, _, rng = val.partition("@")
            a, b = (int(v) for v in rng.split("-")) if rng else (0, len(self.blocks) - 1)
            for L in range(a, b + 1):
                self.x8_terms[L][name] = int(val)

    def _pos_for(self, ph: int, pw: int):
        """interpolate_pos_encoding (dinov2.py:179-210): identity for the square 37x37 grid, else bicubic
        resample with scale ((ph+0.1)/37, (pw+0.1)/37). Returns (f32 [1+P, C] table, f32 [C] cls row)."""
        key = (ph, pw)
        if key not in self._pos_cache:
            rt, C = self.rt, self.C
            gs = int(math.sqrt(self.pos.shape[0] - 1))
            if ph * pw == gs * gs and ph == pw:
                table = self.pos
            else:
                table = torch.empty((1 + ph * pw, C), dtype=torch.float32, device=rt.device)
                table[0].copy_(self.pos[0])
                sx, sy = float(ph + 0.1) / gs, float(pw + 0.1) / gs
                rt.bicubic(self.pos[1:], table[1:], gs, gs, ph, pw, C, sx, sy)
            self._pos_cache[key] = (table, (self.cls + table[0]).contiguous())
        return self._pos_cache[key]

    def run(self, x: torch.Tensor, want_f32_last: bool = False, tap_out=None):
        """x f32 [Bf,3,H,W] -> 4 final-normed patch-token maps, half [Bf*P, C] each (cls dropped,
        dinov2.py:309-312); optionally also the last one in f32 (input of the memory block).
        `tap_out`: 4 caller-owned HL destinations [Bf*P, C] (the clip-level tap cache of the video driver)."""
        rt, C, Hh = self.rt, self.C, self.heads
        Bf, _, H, W = x.shape
        assert H % PATCH == 0 and W % PATCH == 0, "input sides must be multiples of 14 (patch_embed.py:73-74)"
        ph, pw = H // PATCH, W // PATCH
        P, N = ph * pw, ph * pw + 1
        M = Bf * N
        table, cls_row = self._pos_for(ph, pw)
        rows = rt.hbuf("patch_rows", (Bf * P, 640))
        rt.patchify(x, rows, Bf, H, W, 640)
        tok = rt.fbuf("tokens", (M, C))
        rt.fill_row(tok, cls_row, Bf, N, 0, C)
        rt.gemm(rows, self.w_patch, Bf * P, C, 640, out=tok, bias=self.b_patch, tab=table, tab_mod=P, tab_off=1,
                row_group=P, row_skip=1)
        npad = ceil_to(N, 64)
        q = rt.hbuf("enc_q", (Bf * Hh, npad, 64), zero=True)
        k = rt.hbuf("enc_k", (Bf * Hh, npad, 64), zero=True)
        vt = rt.hbuf("enc_vt", (Bf * Hh, 64, npad), zero=True)
        q8, k8 = rt.qk8("enc_q8", Bf * Hh, npad), rt.qk8("enc_k8", Bf * Hh, npad)  # e5m2 planes for the score cross terms
        Hd = self.hidden
        heads = rt.head_split([(q, q8), (k, k8)], vt, Hh, N, npad)
        outs, last_f32 = [], None
        readout = getattr(self, "readout", None)   # ReadoutEngine when the head was built with use_clstoken
        probe = getattr(self, "probe", None)   # tests only: callable(block index, fp32 token stream [M, C]); -1 = input of block 0
        if probe is not None:
            probe(-1, tok)
        # 8-bit cross-term path: large batches only, with the default attention (the only producer of the 8-bit output planes).
        # Its activations between the linears are K-tile-major planes: fp16 hi + the 6-bit rows of hi and remainder — no fp16 lo plane
        use8 = self.x8 and rt.x8_rows(M) and q8 is not None and rt.pv_products != 3
        hn, att, f1 = rt.operand("enc_ln", (M, C), use8), rt.operand("enc_att", (M, C), use8), rt.operand("enc_fc1", (M, Hd), use8)
        for i, b in enumerate(self.blocks):
            xt = self.x8_terms[i]
            rt.layernorm(tok, M, C, b["n1w"], b["n1b"], 1e-6, out_h=hn)
            rt.gemm(hn, b["wqkv"], M, 3 * C, C, bias=b["bqkv"], store=abi.ST_HEADS, heads=heads, tag="enc_linear", x8_terms=xt["qkv"])
            rt.flash_attn(q, k, vt, att, Bf, Hh, N, npad, N, npad, 64 ** -0.5, tag="enc_attn", q8=q8, k8=k8)
            rt.gemm(att, b["wproj"], M, C, C, bias=b["bproj"], gamma=b["ls1"], res1=tok, out=tok, tag="enc_linear", x8_terms=xt["proj"])
            rt.layernorm(tok, M, C, b["n2w"], b["n2b"], 1e-6, out_h=hn)
            if self.cfg.get("swiglu"):
                rt.gemm(hn, b["wfc1"], M, 2 * Hd, C, bias=b["bfc1"], store=abi.ST_GEGLU, act=abi.ACT_SILU, out=f1, tag="enc_linear")
            else:
                rt.gemm(hn, b["wfc1"], M, Hd, C, bias=b["bfc1"], act=GELU, out=f1, tag="enc_linear", x8_terms=xt["fc1"])
            rt.gemm(f1, b["wfc2"], M, C, Hd, bias=b["bfc2"], gamma=b["ls2"], res1=tok, out=tok, tag="enc_linear", x8_terms=xt["fc2"])
            if probe is not None:
                probe(i, tok)
            if i in self.taps:
                j = self.taps.index(i)
                t = tap_out[j] if tap_out is not None else rt.hbuf(f"tap{j}", (Bf * P, C))
                f = None
                if want_f32_last and j == len(self.taps) - 1:
                    f = last_f32 = rt.fbuf("tap_last_f32", (Bf * P, C))
                if readout is None:
                    rt.layernorm(tok, M, C, self.nw, self.nb, 1e-6, out_h=t, out_f=f, out_group=N)
                else:
                    # the final-normed cls row of every frame, then the readout projection on the normed patch tokens;
                    # with want_f32_last (path A) the last tap goes through the memory block first: its readout is the caller's
                    last = want_f32_last and j == len(self.taps) - 1
                    raw = t if last else rt.hbuf("tap_raw", (Bf * P, C))
                    rt.layernorm(tok, M, C, self.nw, self.nb, 1e-6, out_h=raw, out_f=f, out_group=N)
                    cls = rt.fbuf("cls_norm_last" if last else "cls_norm", (Bf, C))
                    rt.layernorm(tok.view(Bf, N, C)[:, 0].contiguous(), Bf, C, self.nw, self.nb, 1e-6, out_f=cls)
                    if last:
                        self.cls_last = cls
                    else:
                        readout.apply(j, raw, cls, Bf, P, t)
                outs.append(t)
        return outs, last_f32, (ph, pw)


# =============================================================================================
class ReadoutEngine:
    """use_clstoken (dpt.py:81-88,119-123): tap' = GELU(Linear_2C->C(cat(tap, cls expanded))). The cls half of the weight
    acts on ONE row per frame, so it becomes a per-frame bias: c_b = W[:, C:] cls_b + bias, tap'_b = GELU(tap_b W[:, :C]^T + c_b)
    — one small GEMM for the biases and one GEMM per frame. No shipped configuration enables the flag; this path is
    about the constructor contract, not speed."""

    def __init__(self, rt: Runtime, mods, C: int):
        self.rt, self.C = rt, C
        h = rt.prec
        self.w1 = [pack.linear(m[0].weight[:, :C].contiguous(), h) for m in mods]
        self.w2 = [pack.linear(m[0].weight[:, C:].contiguous(), h) for m in mods]
        self.b = [pack.f32(m[0].bias) for m in mods]

    def apply(self, j: int, x, cls_f32: torch.Tensor, Bf: int, P: int, out):
        rt, C = self.rt, self.C
        cb = rt.fbuf("ro_cb", (Bf, C))
        rt.gemm(rt.to_half(cls_f32), self.w2[j], Bf, C, C, bias=self.b[j], out=cb)
        for b in range(Bf):
            rt.gemm(x.narrow0(b * P, P), self.w1[j], P, C, C, bias=cb[b], act=GELU, out=out.narrow0(b * P, P))
        return out


# =============================================================================================
class TemporalEngine:
    """TemporalModule: video_depth_anything/motion_module/motion_module.py:102-136,174-192,245-326,
    attention.py:182-211 (softmax attention over frames), :296-384 (GEGLU feed-forward)."""

    def __init__(self, rt: Runtime, mod, c: int, idx: int):
        self.rt, self.c, self.idx = rt, c, idx
        h = rt.prec
        tt = mod.temporal_transformer
        blk = tt.transformer_blocks[0]
        self.gnw, self.gnb = pack.f32(tt.norm.weight), pack.f32(tt.norm.bias)
        self.w_in, self.b_in = pack.linear(tt.proj_in.weight, h), pack.f32(tt.proj_in.bias)
        # the LayerNorm-fed linears (q|k|v of both attention blocks, the gated feed-forward's first layer: 14 of the module's
        # 22 c^2 products per row) on the cross-term kernel when a window brings >= 4096 rows; the others take their input from
        # kernels that write no 6-bit rows (GroupNorm, the attention over frames, the gated epilogue)
        self.x8 = rt.x8_capable(c)
        x8_order = pack.ORDER_NATURAL if self.x8 else None
        self.att = []
        for i in range(2):
            a = blk.attention_blocks[i]
            wqkv, _ = pack.cat_proj([a.to_q.weight, a.to_k.weight, a.to_v.weight], [None, None, None], [0, 0, 0], h)
            wqkv = pack.Linear(wqkv, x8_order)
            rope = not hasattr(a, "pos_encoder")   # pe = 'rope' (motion_module.py:236-240): q / k rotated by frame index, no additive term
            if rope:
                Tm = a.max_len
                pe64 = torch.zeros((Tm, c), dtype=torch.float64, device=a.to_q.weight.device)
                fr = 1.0 / (10000.0 ** (torch.arange(0, c, 2, dtype=torch.float32)[: c // 2] / c))     # attention.py:403-408
                ang = torch.outer(torch.arange(Tm, dtype=torch.float32), fr)
                rope_cs = torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous().to(a.to_q.weight.device)   # [T, c/2, 2]
            else:
                pe64 = a.pos_encoder.pe.detach().double().reshape(-1, c)
                rope_cs = None
            self.att.append(dict(
                nw=pack.f32(blk.norms[i].weight), nb=pack.f32(blk.norms[i].bias), wqkv=wqkv,
                pe=None if rope else pack.f32(a.pos_encoder.pe).reshape(-1, c), rope_cs=rope_cs, max_len=pe64.shape[0],
                # (streaming with 'rope': the reference rotates by freqs_cis[:1] = position 0 = the identity
                # (motion_module.py:279-282 with a one-frame query), i.e. no position enters: the zero tables below)
                # streaming mode: W (x + pe[t]) = W x + W pe[t] -> the position term of each projection as a [T, c] table
                pe_q=(pe64 @ a.to_q.weight.detach().double().t()).float().contiguous(),
                pe_k=(pe64 @ a.to_k.weight.detach().double().t()).float().contiguous(),
                pe_v=(pe64 @ a.to_v.weight.detach().double().t()).float().contiguous(),
                wo=pack.linear(a.to_out[0].weight, h), bo=pack.f32(a.to_out[0].bias)))
        self.fnw, self.fnb = pack.f32(blk.ff_norm.weight), pack.f32(blk.ff_norm.bias)
        wg, self.bg = pack.geglu(blk.ff.net[0].proj.weight, blk.ff.net[0].proj.bias, h)
        self.wg = pack.Linear(wg, x8_order)
        self.wf2, self.bf2 = pack.linear(blk.ff.net[2].weight, h), pack.f32(blk.ff.net[2].bias)
        self.w_out, self.b_out = pack.linear(tt.proj_out.weight, h), pack.f32(tt.proj_out.bias)

    def gn(self, x, F: int, HW: int):
        """GroupNorm(32, eps 1e-6) per frame (motion_module.py:112): needs all pixels of a frame."""
        g = self.rt.hbuf("tm_gn", (F * HW, self.c))
        self.rt.groupnorm(x, g, F, HW, self.c, 32, self.gnw, self.gnb, 1e-6)
        return g

    def core(self, g, B: int, T: int, D: int):
        """proj_in -> 2 x (LN + PE, q/k/v, attention over frames, out) -> GEGLU FF (motion_module.py:116-192).
        Everything here is per pixel, so `D` may be any subset of a frame's pixels (vdn/dist.py)."""
        rt, c = self.rt, self.c
        M = B * T * D
        assert T <= self.att[0]["max_len"], "clip longer than temporal_max_len (motion_module.py:200-213)"
        hs = rt.fbuf("tm_h", (M, c))
        rt.gemm(g, self.w_in, M, c, c, bias=self.b_in, out=hs)
        # (the kernel takes launches of >= 2^20 outputs: narrow modules of small windows stay on the three-product kernels)
        n = rt.operand("tm_n", (M, c), self.x8 and rt.x8_rows(M) and M * 3 * c >= (1 << 20))
        qkv = rt.hbuf("tm_qkv", (M, 3 * c))
        a = rt.hbuf("tm_a", (M, c))
        for at in self.att:
            rt.layernorm(hs, M, c, at["nw"], at["nb"], 1e-5, out_h=n, addtab=at["pe"], tab_div=D, tab_mod=T)
            rt.gemm(n, at["wqkv"], M, 3 * c, c, out=qkv)
            rt.temporal_attn(qkv, a, B, T, D, c, 8, (c // 8) ** -0.5, rope_cs=at["rope_cs"])
            rt.gemm(a, at["wo"], M, c, c, bias=at["bo"], res1=hs, out=hs)
        gg = rt.hbuf("tm_gg", (M, 4 * c))
        rt.layernorm(hs, M, c, self.fnw, self.fnb, 1e-5, out_h=n)
        rt.gemm(n, self.wg, M, 8 * c, c, bias=self.bg, store=abi.ST_GEGLU, out=gg)
        hh = rt.hbuf("tm_hh", (M, c))
        rt.gemm(gg, self.wf2, M, c, 4 * c, bias=self.bf2, res1=hs, out=hh)
        return hh

    def out(self, hh, x, M: int):
        """proj_out + residual with the module input (motion_module.py:131-135)."""
        y = self.rt.hbuf(f"tm_out{self.idx}", (M, self.c))
        self.rt.gemm(hh, self.w_out, M, self.c, self.c, bias=self.b_out, res1=x, out=y)
        return y

    def run(self, x, B: int, T: int, HW: int):
        """x half [(b f) * HW, c] (NHWC frames) -> same shape."""
        return self.out(self.core(self.gn(x, B * T, HW), B, T, HW), x, B * T * HW)

    STREAM_SLOTS = 44  # the reference keeps at most 42 cached frames (video_depth_stream.py:155-158) + the new one

    def run_stream(self, x, HW: int, window_slots, new_slot: int):
        """Streaming step (video_depth_stream.py:76-160, motion_module.py:255-277): x is ONE frame [HW, c].
        `window_slots`: ring slots of the (up to 31) cached frames this step attends over, oldest first; the new frame's
        projections go to ring slot `new_slot` and it attends last.
        A slot holds the frame's q|k|v PROJECTION without the position term (f32 [HW, 3c]): the
        reference caches the LayerNorm output and re-projects all 32 frames with the sliding window's positions
        every step; here each frame is projected once and the positions enter as [T, c] tables inside
        `vdn_temporal_attn_last` (W(x + pe) = Wx + W pe), which also computes the newest frame's query only.
        The two attention blocks own one fixed ring each (nothing is allocated per step, no pointer table)."""
        rt, c = self.rt, self.c
        g = self.gn(x, 1, HW)
        hs = rt.fbuf("ts_h", (HW, c))
        rt.gemm(g, self.w_in, HW, c, c, bias=self.b_in, out=hs)
        nh = rt.hbuf("ts_nh", (HW, c))
        a = rt.hbuf("ts_a", (HW, c))
        slots = list(window_slots) + [new_slot]
        for j, at in enumerate(self.att):
            pool = rt.fbuf(f"ts_pool{self.idx}_{j}", (self.STREAM_SLOTS, HW, 3 * c))
            rt.layernorm(hs, HW, c, at["nw"], at["nb"], 1e-5, out_h=nh)
            rt.gemm(nh, at["wqkv"], HW, 3 * c, c, out=pool[new_slot])
            rt.temporal_attn_last(pool, slots, at["pe_q"], at["pe_k"], at["pe_v"], a, HW, c, (c // 8) ** -0.5)
            rt.gemm(a, at["wo"], HW, c, c, bias=at["bo"], res1=hs, out=hs)
        n = rt.hbuf("ts_n", (HW, c))
        rt.layernorm(hs, HW, c, self.fnw, self.fnb, 1e-5, out_h=n)
        gg = rt.hbuf("ts_gg", (HW, 4 * c))
        rt.gemm(n, self.wg, HW, 8 * c, c, bias=self.bg, store=abi.ST_GEGLU, out=gg)
        hh = rt.hbuf("ts_hh", (HW, c))
        rt.gemm(gg, self.wf2, HW, c, 4 * c, bias=self.bf2, res1=hs, out=hh)
        return self.out(hh, x, HW)

    def run_sharded(self, x, exch, HW: int):
        """Frame-sharded window (vdn/dist.py): x holds this rank's Tl frames. GroupNorm and proj_out run
        on the frame shard; the per-pixel core runs on all T frames of this rank's pixel shard, with one
        all-to-all before and one after per plane (staging: vdn.dist.shard_core, a pure function of tensors
        that tests/test_dist.py drives under gloo). Buffers are consumed in stream order, so plain local
        references keep them alive long enough."""
        from .dist import shard_core
        Tl = exch.Tl
        g = self.gn(x, Tl, HW)

        def core(planes, D):
            hh = self.core(HL(planes[0], planes[1] if len(planes) > 1 else None), 1, exch.T, D)
            return [hh.hi] + ([hh.lo] if hh.lo is not None else [])

        back = shard_core(exch, [g.hi] + ([g.lo] if g.lo is not None else []), HW, core)
        return self.out(HL(back[0], back[1] if len(back) > 1 else None), x, Tl * HW)


# =============================================================================================
class DPTEngine:
    """DPTHead / DPTHeadTemporal: depth_anything_v2/dpt.py:116-151, util/blocks.py:57-148,
    video_depth_anything/dpt_temporal.py:53-127."""

    def __init__(self, rt: Runtime, mod, in_ch: int, features: int, out_channels, temporal: bool):
        self.rt, self.C, self.F, self.oc = rt, in_ch, features, list(out_channels)
        h = rt.prec
        self.proj = [(pack.conv1x1(p.weight, h), pack.f32(p.bias)) for p in mod.projects]
        self.rt0 = pack.conv_transpose(mod.resize_layers[0].weight, mod.resize_layers[0].bias, h)
        self.rt1 = pack.conv_transpose(mod.resize_layers[1].weight, mod.resize_layers[1].bias, h)
        self.rs3 = (pack.conv3x3(mod.resize_layers[3].weight, h), pack.f32(mod.resize_layers[3].bias))
        s = mod.scratch
        self.rn = [pack.conv3x3(getattr(s, f"layer{i + 1}_rn").weight, h) for i in range(4)]

        def fold(conv, bn):
            """use_bn (util/blocks.py:49-51,71-77): eval-mode BatchNorm is a per-channel affine map, folded into the conv"""
            w, b = conv.weight.detach().float(), conv.bias.detach().float()
            if bn is None:
                return w, b
            sc = bn.weight.detach().float() / torch.sqrt(bn.running_var.detach().float() + 1e-5)
            return w * sc[:, None, None, None], (b - bn.running_mean.detach().float()) * sc + bn.bias.detach().float()

        # The RCU convolutions of the two high-resolution fusion blocks on the cross-term kernel (include/vdn.h pad_hi; DESIGN.md
        # §5 item 2c): their weights once more as that kernel's planes. VDN_RCU_X3 keeps the three-product launches (A/B switch)
        self.rcu_x8 = rt.x8_capable(features) and features % 256 == 0 and not os.environ.get("VDN_RCU_X3")
        self.rcu_path = {}     # fusion block -> "x8" | "x3": what its last _fusion call launched (tests, tools)
        self._rcu_x8_ok = True  # run(): off for the temporal head's sharded and streaming calls

        def rcu(r, x8):
            w1, b1 = fold(r.conv1, getattr(r, "bn1", None))
            w2, b2 = fold(r.conv2, getattr(r, "bn2", None))
            d = dict(w1=pack.conv3x3(w1, h), b1=pack.f32(b1), w2=pack.conv3x3(w2, h), b2=pack.f32(b2))
            if x8:
                d.update(x1=pack.conv3x3_x8(w1, h), x2=pack.conv3x3_x8(w2, h))
            return d

        self.ref = {}
        for i in range(1, 5):
            f = getattr(s, f"refinenet{i}")
            x8 = self.rcu_x8 and i in (1, 2)
            self.ref[i] = dict(r1=rcu(f.resConfUnit1, x8), r2=rcu(f.resConfUnit2, x8),
                               wo=pack.conv1x1(f.out_conv.weight, h), bo=pack.f32(f.out_conv.bias))
        self.oc1 = (pack.conv3x3(s.output_conv1.weight, h), pack.f32(s.output_conv1.bias))
        self.oc2 = (pack.conv3x3(s.output_conv2[0].weight, h), pack.f32(s.output_conv2[0].bias))
        # fused tail (csrc/tail.hip): needs split planes, 32 output channels and 32-channel input blocks
        w2 = s.output_conv2[0].weight
        fused = h.split and w2.shape[0] == 32 and w2.shape[1] % 32 == 0 and not os.environ.get("VDN_TAIL_UNFUSED")  # A/B switch
        self.oc2_taps = pack.conv3x3_taps(w2, h) if fused else None
        # output_conv1 in front of refinenet1's 2x resize (run()): the nine taps composed with out_conv, once per checkpoint.
        # Only the fused tail reads an fp32 out1; VDN_OC1_HIRES forces the materialised path1 (A/B switch)
        self.oc1_low = None
        if fused and (features // 2) % 16 == 0 and not os.environ.get("VDN_OC1_HIRES"):
            f1 = s.refinenet1.out_conv
            self.oc1_low = pack.lowres_oc1(s.output_conv1.weight, f1.weight, f1.bias, h)
        # layer{1,2}_rn folded into the ConvTranspose in front of them (run()): one sub-pixel convolution on the source map per
        # level, composed once per checkpoint. On wherever the kernel mode takes the widths (pack.subpixel_conv_ok; ViT-L);
        # VDN_RN_HIRES forces the materialised 4x / 2x maps (A/B switch)
        self.rn_low = [None, None]
        if not os.environ.get("VDN_RN_HIRES"):
            for i, k in enumerate((4, 2)):
                if pack.subpixel_conv_ok(self.oc[i], features, k, h):
                    rl = mod.resize_layers[i]
                    self.rn_low[i] = pack.subpixel_conv(rl.weight, rl.bias, getattr(s, f"layer{i + 1}_rn").weight, h)
        self.w_last = pack.f32(s.output_conv2[2].weight).reshape(-1)
        self.b_last = float(s.output_conv2[2].bias.detach().float().item())
        self.temporal = None
        if temporal:
            chans = [self.oc[2], self.oc[3], features, features]
            self.temporal = [TemporalEngine(rt, mod.motion_modules[i], chans[i], i) for i in range(4)]

    # -- helpers
    def _conv3(self, x, w, Bf, H, W, Cin, Cout, name, *, stride=1, bias=None, relu_a=False, act=0, res1=None, res2=None,
               f32_out=False):
        OH, OW = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        out = (self.rt.fbuf if f32_out else self.rt.hbuf)(name, (Bf * OH * OW, Cout))
        self.rt.gemm(x, w, Bf * OH * OW, Cout, 9 * Cin, out=out, bias=bias, act=act, relu_a=relu_a, res1=res1, res2=res2,
                     conv=dict(B=Bf, H=H, W=W, C=Cin, OH=OH, OW=OW, stride=stride))
        return out

    def _rcu(self, r, x, Bf, H, W, name, extra=None):
        """ResidualConvUnit (blocks.py:67-80): conv2(relu(conv1(relu(x)))) + x [+ extra]."""
        F = self.F
        t = self._conv3(x, r["w1"], Bf, H, W, F, F, "rcu_t", bias=r["b1"], relu_a=True, act=RELU)
        return self._conv3(t, r["w2"], Bf, H, W, F, F, name, bias=r["b2"], res1=x, res2=extra)

    def _fusion(self, i, Bf, size_in, size_out, prev, skip=None):
        """FeatureFusionBlock (blocks.py:123-148). The 1x1 out_conv commutes with the bilinear resize
        (both linear, interpolation weights sum to 1), so it runs at the LOW resolution: 4x fewer
        flops, same result up to rounding."""
        rt, F = self.rt, self.F
        H, W = size_in
        f = self.ref[i]
        x = prev
        M = Bf * H * W
        if self.rcu_x8 and self._rcu_x8_ok and i in (1, 2) and rt.x8_rows(Bf * (H + 2) * (W + 2)):
            # Four shifted-row cross-term GEMMs on padded operand planes that ping-pong between two buffers: one pack pass for
            # the block's first operand, every later one comes out of the convolution before it. The results land where the
            # three-product path writes them (ff{i}_s, ff{i}_u: unpadded split planes)
            self.rcu_path[i] = "x8"
            pa, pb = rt.pad_operand("rcu_pa", Bf, H, W, F), rt.pad_operand("rcu_pb", Bf, H, W, F)
            rt.pack_x8_relu_pad(skip if skip is not None else x, pa)
            if skip is not None:
                r = f["r1"]
                rt.conv3x3_pad(pa, r["x1"], F, r["b1"], out_pad=pb)
                x = rt.conv3x3_pad(pb, r["x2"], F, r["b2"], out=rt.hbuf(f"ff{i}_s", (M, F)), res1=skip, res2=prev, out_pad=pa)
            r = f["r2"]
            rt.conv3x3_pad(pa, r["x1"], F, r["b1"], out_pad=pb)
            u = rt.conv3x3_pad(pb, r["x2"], F, r["b2"], out=rt.hbuf(f"ff{i}_u", (M, F)), res1=x)
        else:
            self.rcu_path[i] = "x3"
            if skip is not None:
                x = self._rcu(f["r1"], skip, Bf, H, W, f"ff{i}_s", extra=prev)
            u = self._rcu(f["r2"], x, Bf, H, W, f"ff{i}_u")
        if size_out is None:  # run(): out_conv and the resize are taken over by the low-resolution output_conv1
            return u
        v = rt.hbuf(f"ff{i}_v", (Bf * H * W, F))
        rt.gemm(u, f["wo"], Bf * H * W, F, F, bias=f["bo"], out=v)
        OH, OW = size_out
        p = rt.hbuf(f"path{i}", (Bf * OH * OW, F))
        rt.upsample(v, p, Bf, H, W, OH, OW, F)
        return p

    def run(self, taps: List[torch.Tensor], Bf: int, ph: int, pw: int, T: Optional[int] = None, relu: bool = True,
            exch=None, stream=None, out: Optional[torch.Tensor] = None, act: Optional[int] = None, out_scale: float = 1.0):
        """`out` (f32 [Bf, 14 ph, 14 pw], contiguous): the caller's result tensor, written by the last kernel directly;
        without it the depth lands in this engine's arena (valid until the next run).
        `act` (abi.OUT_*; default: relu -> OUT_RELU / OUT_NONE) is the head's final activation and `out_scale` the factor of
        OUT_SIGMOID (the metric head, metric_depth/depth_anything_v2/dpt.py:112-113,183); both are launch arguments of the
        last kernel, whichever of the three endings below runs."""
        rt, C, F, oc = self.rt, self.C, self.F, self.oc
        self._rcu_x8_ok = exch is None and stream is None
        P = ph * pw
        pr = []
        for i in range(4):
            o = rt.hbuf(f"proj{i}", (Bf * P, oc[i]))
            rt.gemm(taps[i], self.proj[i][0], Bf * P, oc[i], C, bias=self.proj[i][1], out=o)
            pr.append(o)
        s1, s2, s3 = (4 * ph, 4 * pw), (2 * ph, 2 * pw), (ph, pw)
        s4 = ((ph + 2 - 3) // 2 + 1, (pw + 2 - 3) // 2 + 1)

        def level(i, k, size, wT, name):
            """resize_layers[i] (ConvTranspose k = s) then layer{i+1}_rn (3x3): as ONE sub-pixel convolution on the ph x pw map
            where the kernel takes the widths (no non-linearity in between: every output phase is a short 3x3-neighbourhood
            sum of the projected map; the k-times map is never written), else as written."""
            if self.rn_low[i] is not None:
                r = rt.hbuf(name + "_rn", (Bf * size[0] * size[1], F))
                return rt.gemm(pr[i], self.rn_low[i][0], Bf * P, k * k * F, 4 * oc[i], store=abi.ST_CONVT, out=r,
                               conv=dict(B=Bf, H=ph, W=pw, C=oc[i], OH=ph, OW=pw, stride=1, korder=1),
                               convt=dict(k=k, cout=F, B=Bf, H=ph, W=pw), subpix_bias=self.rn_low[i][1])
            l = rt.hbuf(name, (Bf * size[0] * size[1], oc[i]))
            rt.gemm(pr[i], wT[0], Bf * P, k * k * oc[i], oc[i], bias=wT[1], store=abi.ST_CONVT, out=l,
                    convt=dict(k=k, cout=oc[i], B=Bf, H=ph, W=pw))
            return self._conv3(l, self.rn[i], Bf, size[0], size[1], oc[i], F, name + "_rn")

        r1 = level(0, 4, s1, self.rt0, "l1")
        r2 = level(1, 2, s2, self.rt1, "l2")
        l3 = pr[2]
        l4 = self._conv3(pr[3], self.rs3[0], Bf, ph, pw, oc[3], oc[3], "l4", stride=2, bias=self.rs3[1])
        def tm(i, x, hw):
            if stream is not None:  # streaming: one new frame against the cached projections of up to 31 earlier ones
                return self.temporal[i].run_stream(x, hw, stream["window"], stream["new"])
            if exch is not None:  # frame-sharded window: Bf == this rank's frames of ONE clip
                return self.temporal[i].run_sharded(x, exch, hw)
            return self.temporal[i].run(x, Bf // T, T, hw)

        if self.temporal is not None:
            l3 = tm(0, l3, s3[0] * s3[1])
            l4 = tm(1, l4, s4[0] * s4[1])
        r3 = self._conv3(l3, self.rn[2], Bf, s3[0], s3[1], oc[2], F, "l3_rn")
        r4 = self._conv3(l4, self.rn[3], Bf, s4[0], s4[1], oc[3], F, "l4_rn")
        p4 = self._fusion(4, Bf, s4, s3, r4)
        if self.temporal is not None:
            p4 = tm(2, p4, s3[0] * s3[1])
        p3 = self._fusion(3, Bf, s3, s2, p4, r3)
        if self.temporal is not None:
            p3 = tm(3, p3, s2[0] * s2[1])
        p2 = self._fusion(2, Bf, s2, s1, p3, r2)
        s0 = (2 * s1[0], 2 * s1[1])
        H, W = ph * PATCH, pw * PATCH
        if out is not None:
            assert out.shape == (Bf, H, W) and out.dtype == torch.float32 and out.is_contiguous(), (out.shape, out.dtype)
        depth = out if out is not None else rt.fbuf("depth", (Bf, H, W))
        sy, sx = (s0[0] - 1) / max(H - 1, 1), (s0[1] - 1) / max(W - 1, 1)
        fused = self.oc2_taps is not None and int(17 * sy) + 3 <= 13 and int(17 * sx) + 3 <= 13
        if fused and self.oc1_low is not None and rt.lowres_oc1_rows(Bf * s0[0] * s0[1]):
            # output_conv1 o resize o out_conv has no non-linearity inside (dpt.py:145, blocks.py:144-146): a channel mixing
            # commutes with the resize tap by tap, so all nine taps' mixing (composed with out_conv) is ONE GEMM on the 4x
            # map, 4x fewer flops than the conv on the 8x map, and the combine kernel interpolates and adds the tap images.
            # path1 and ff1_v are never written. Small maps stay below (lowres_oc1_rows)
            u = self._fusion(1, Bf, s1, None, p2, r1)
            M1 = Bf * s1[0] * s1[1]
            z = rt.fbuf("oc1_z", (M1, 9 * (F // 2)))
            rt.gemm(u, self.oc1_low[0], M1, 9 * (F // 2), F, bias=self.oc1_low[1], out=z)
            o1 = rt.fbuf("out1_f32", (Bf * s0[0] * s0[1], F // 2))
            rt.oc1_combine(z, self.oc1[1], o1, Bf, s1[0], s1[1], s0[0], s0[1], F // 2)
            rt.depth_tail(o1, self.oc2_taps, self.oc2[1], self.w_last, self.b_last, depth, Bf, s0[0], s0[1], F // 2, H, W, relu, act, out_scale)
            return depth
        p1 = self._fusion(1, Bf, s1, s0, p2, r1)
        if fused:
            # resize -> conv3x3 + ReLU -> conv1x1 (+ ReLU) without leaving the chip (the scale is 8/14 for every DPT head);
            # output_conv1 then writes ONE fp32 plane, which is what the fused kernel interpolates from
            o1 = self._conv3(p1, self.oc1[0], Bf, s0[0], s0[1], F, F // 2, "out1_f32", bias=self.oc1[1], f32_out=True)
            rt.depth_tail(o1, self.oc2_taps, self.oc2[1], self.w_last, self.b_last, depth, Bf, s0[0], s0[1], F // 2, H, W, relu, act, out_scale)
            return depth
        o1 = self._conv3(p1, self.oc1[0], Bf, s0[0], s0[1], F, F // 2, "out1", bias=self.oc1[1])
        up = rt.hbuf("out_up", (Bf * H * W, F // 2))
        rt.upsample(o1, up, Bf, s0[0], s0[1], H, W, F // 2)
        o2 = self._conv3(up, self.oc2[0], Bf, H, W, F // 2, 32, "out2", bias=self.oc2[1], act=RELU)
        rt.head_out(o2, self.w_last, self.b_last, depth, Bf * H * W, 32, relu, act, out_scale)
        return depth


# =============================================================================================
class MemoryEngine:
    """MemoryBlock: depth_anything_v2/memory_block.py:83-125 over sam2/modeling/{memory_attention.py:58-169,
    sam/transformer.py:275-311, position_encoding.py:192-239, memory_encoder.py:158-181}.

    MI355X-first differences that leave the result unchanged:
      * the reference re-projects all S stored frames through k_proj/v_proj of every layer on every
        call; here each pushed frame's rotated K and V^T are written once into a per-layer 6-slot
        ring in HBM (keys are order-invariant under softmax, RoPE depends on t % P only), so the
        cross-attention reads them in place;
      * memory_pos_enc / maskmem_tpos_enc never reach the output under the flags MemoryBlock sets
        (pos_enc_at_cross_attn_keys=False, memory_block.py:39), so they are not computed.
    """

    def __init__(self, rt: Runtime, mod, C: int, max_len: int):
        self.rt, self.C, self.heads, self.max_len = rt, C, C // 64, max_len
        h = rt.prec
        ma = mod.memory_attention
        # 8-bit cross terms for the plain linears of the memory attention and the memory encoder (as in EncoderEngine)
        self.x8 = rt.x8_capable(C)

        def lin(w, order):
            return pack.Linear(w, order if self.x8 else None)

        NAT, GEMM, ATTN = pack.ORDER_NATURAL, pack.ORDER_GEMM, pack.ORDER_ATTN
        self.layers = []
        for l in ma.layers:
            sa, ca = l.self_attn, l.cross_attn_image
            wqkv, bqkv = pack.cat_proj([sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight],
                                       [sa.q_proj.bias, sa.k_proj.bias, sa.v_proj.bias], [1, 1, 0], h)
            wq, bq = pack.cat_proj([ca.q_proj.weight], [ca.q_proj.bias], [1], h)
            wkv, bkv = pack.cat_proj([ca.k_proj.weight, ca.v_proj.weight], [ca.k_proj.bias, ca.v_proj.bias], [1, 0], h)
            self.layers.append(dict(
                n1w=pack.f32(l.norm1.weight), n1b=pack.f32(l.norm1.bias),
                n2w=pack.f32(l.norm2.weight), n2b=pack.f32(l.norm2.bias),
                n3w=pack.f32(l.norm3.weight), n3b=pack.f32(l.norm3.bias),
                wqkv=lin(wqkv, NAT), bqkv=bqkv, wso=lin(pack.linear(sa.out_proj.weight, h), ATTN), bso=pack.f32(sa.out_proj.bias),
                wq=lin(wq, NAT), bq=bq, wkv=lin(wkv, NAT), bkv=bkv,
                wco=lin(pack.linear(ca.out_proj.weight, h), ATTN), bco=pack.f32(ca.out_proj.bias),
                w1=lin(pack.linear(l.linear1.weight, h), NAT), b1=pack.f32(l.linear1.bias),
                w2=lin(pack.linear(l.linear2.weight, h), GEMM), b2=pack.f32(l.linear2.bias)))
        self.nw, self.nb = pack.f32(ma.norm.weight), pack.f32(ma.norm.bias)
        self.curr_pos = pack.f32(mod.curr_pos_enc).reshape(-1)
        self.no_mem = mod.no_mem_embed.detach().float().reshape(1, -1)
        me = mod.memory_encoder

        def flat(*ts):
            return torch.cat([t.detach().float().reshape(-1) for t in ts]).contiguous()

        e0, e1 = me.mask_downsampler[0].encoder, me.mask_downsampler[1].encoder
        self.md1 = flat(e0[0].weight, e0[0].bias, e0[1].weight, e0[1].bias, e0[3].weight, e0[3].bias)
        self.md2 = flat(e1[0].weight, e1[0].bias, e1[1].weight, e1[1].bias, e1[3].weight, e1[3].bias)
        assert self.md1.numel() == 53 and self.md2.numel() == 2598
        self.wpix, self.bpix = pack.conv1x1(me.pix_feat_proj.weight, h), pack.f32(me.pix_feat_proj.bias)
        self.cx = []
        for b in me.fuser.layers:
            self.cx.append(dict(
                wdw=b.dwconv.weight.detach().float().reshape(C, 49).t().contiguous(), bdw=pack.f32(b.dwconv.bias),
                nw=pack.f32(b.norm.weight), nb=pack.f32(b.norm.bias),
                w1=lin(pack.linear(b.pwconv1.weight, h), NAT), b1=pack.f32(b.pwconv1.bias),
                w2=lin(pack.linear(b.pwconv2.weight, h), GEMM), b2=pack.f32(b.pwconv2.bias), g=pack.f32(b.gamma)))
        # Bank state shared by every lane copy of this engine (DepthAnythingV2._stream_lanes): ONE ring for the whole
        # batch, lane i of n works on batch rows [i B/n, (i+1) B/n) of it, so laned and single-lane calls see the
        # same memory and `count` advances once per forward (commit()).
        self.state = {"count": 0, "shape": None}
        self.lane = (0, 1)
        self.bank_rt = rt
        self._rope = {}
        self._nomem = {}

    def clear(self):
        self.state["count"] = 0
        self.state["shape"] = None

    @property
    def S(self):
        return min(self.state["count"], self.max_len)

    def _rope_for(self, side):
        if side not in self._rope:
            self._rope[side] = pack.rope_table(side, side, 64, device=self.rt.device)
        return self._rope[side]

    def prepare(self, B: int, P: int):
        """Called once per forward on the caller's stream BEFORE any lane forks: checks the bank against the batch
        (the reference asserts on a batch mismatch between the frame and its memories, memory_attention.py:135-137)
        and makes sure the ring and the RoPE table exist."""
        st = self.state
        if st["shape"] != (B, P):
            if st["count"] > 0:
                raise RuntimeError(f"memory bank holds {self.S} frame(s) of batch/grid {st['shape']} but the new frame is "
                                   f"{(B, P)}: call clear_memory() before changing the batch size or resolution")
            st["shape"] = (B, P)
        side = int(math.sqrt(P))
        assert side * side == P, "MemoryBlock assumes square inputs (memory_block.py:85)"
        self._rope_for(side)
        self._bank_full(B, P)

    def commit(self):
        self.state["count"] += 1

    def _bank_full(self, B, P):
        rt, Hh = self.bank_rt, self.heads
        tp = ceil_to(self.max_len * P, 64)
        ks = [rt.hbuf(f"mem_k{l}", (B * Hh, tp, 64), zero=True) for l in range(len(self.layers))]
        vs = [rt.hbuf(f"mem_vt{l}", (B * Hh, 64, tp), zero=True) for l in range(len(self.layers))]
        k8 = [rt.qk8(f"mem_k8{l}", B * Hh, tp) for l in range(len(self.layers))]  # e5m2 planes of the stored keys
        return ks, vs, k8, tp

    def _bank(self, B, P):
        """This lane's rows of the ring: B is the lane's batch."""
        i, n = self.lane
        ks, vs, k8, tp = self._bank_full(B * n, P)
        r0, nr = i * B * self.heads, B * self.heads
        return ([k.narrow0(r0, nr) for k in ks], [v.narrow0(r0, nr) for v in vs],
                [None if t is None else t.narrow(0, r0, nr) for t in k8], tp)

    def forward(self, feat_f32: torch.Tensor, B: int, P: int) -> torch.Tensor:
        """feat_f32 [B*P, C] (final-normed tap 4) -> half [B*P, C] (memory_block.py:92-125)."""
        rt, C, Hh = self.rt, self.C, self.heads
        assert self.state["shape"] == (B * self.lane[1], P), "MemoryEngine.prepare() not called for this batch"
        side = int(math.sqrt(P))
        M = B * P
        cs = self._rope_for(side)
        pp = ceil_to(P, 64)
        x = rt.fbuf("ma_x", (M, C))
        rt.add_vec(feat_f32, self.curr_pos, 0.1, x, M, C)  # memory_attention.py:140-141
        q = rt.hbuf("ma_q", (B * Hh, pp, 64), zero=True)
        k = rt.hbuf("ma_k", (B * Hh, pp, 64), zero=True)
        vt = rt.hbuf("ma_vt", (B * Hh, 64, pp), zero=True)
        q8, k8 = rt.qk8("ma_q8", B * Hh, pp), rt.qk8("ma_k8", B * Hh, pp)
        ks, vs, k8s, tp = self._bank(B, P)
        S = self.S
        if S == 0:
            # empty bank: keys/values come from no_mem_embed broadcast to P tokens (memory_block.py:115-123)
            nk, nk_pad = P, pp
            if M not in self._nomem:  # built once per (lane, batch): the broadcast no_mem_embed rows as half planes
                self._nomem[M] = rt.to_half(self.no_mem.expand(M, C).contiguous())
            a_nm = self._nomem[M]
            ks = [rt.hbuf(f"nomem_k{l}", (B * Hh, pp, 64), zero=True) for l in range(len(self.layers))]
            vs = [rt.hbuf(f"nomem_vt{l}", (B * Hh, 64, pp), zero=True) for l in range(len(self.layers))]
            k8s = [rt.qk8(f"nomem_k8{l}", B * Hh, pp) for l in range(len(self.layers))]
            for l, L in enumerate(self.layers):
                rt.gemm(a_nm, L["wkv"], M, 2 * C, C, bias=L["bkv"], store=abi.ST_HEADS,
                        heads=rt.head_split([(ks[l], k8s[l])], vs[l], Hh, P, pp, rope_cs=cs, rope_mod=P))
        else:
            nk, nk_pad = S * P, tp
        sh = rt.head_split([(q, q8), (k, k8)], vt, Hh, P, pp, rope_cs=cs, rope_mod=P)
        qh = rt.head_split([(q, q8)], None, Hh, P, pp, rope_cs=cs, rope_mod=P)
        # cross-term path: K-tile-major fp16 hi + planes of 6-bit rows between the linears (no fp16 lo plane), as in EncoderEngine.run
        use8 = self.x8 and rt.x8_rows(M) and q8 is not None and rt.pv_products != 3
        n, att, h2 = rt.operand("ma_n", (M, C), use8), rt.operand("ma_att", (M, C), use8), rt.operand("ma_h2", (M, 2 * C), use8)
        for l, L in enumerate(self.layers):
            rt.layernorm(x, M, C, L["n1w"], L["n1b"], 1e-5, out_h=n)
            rt.gemm(n, L["wqkv"], M, 3 * C, C, bias=L["bqkv"], store=abi.ST_HEADS, heads=sh)
            rt.flash_attn(q, k, vt, att, B, Hh, P, pp, P, pp, 0.125, q8=q8, k8=k8)
            rt.gemm(att, L["wso"], M, C, C, bias=L["bso"], res1=x, out=x)
            rt.layernorm(x, M, C, L["n2w"], L["n2b"], 1e-5, out_h=n, addvec=self.curr_pos, alpha=1.0)
            rt.gemm(n, L["wq"], M, C, C, bias=L["bq"], store=abi.ST_HEADS, heads=qh)
            rt.flash_attn(q, ks[l], vs[l], att, B, Hh, P, pp, nk, nk_pad, 0.125, q8=q8, k8=k8s[l])
            rt.gemm(att, L["wco"], M, C, C, bias=L["bco"], res1=x, out=x)
            rt.layernorm(x, M, C, L["n3w"], L["n3b"], 1e-5, out_h=n)
            rt.gemm(n, L["w1"], M, 2 * C, C, bias=L["b1"], act=GELU, out=h2)
            rt.gemm(h2, L["w2"], M, C, 2 * C, bias=L["b2"], res1=x, out=x)
        out = rt.hbuf("mem_out", (M, C))
        rt.layernorm(x, M, C, self.nw, self.nb, 1e-5, out_h=out)
        return out

    def update(self, mem_out: torch.Tensor, depth: torch.Tensor, B: int, ph: int, pw: int):
        """update_memory (memory_block.py:83-90): MemoryEncoder then push; here the push writes the
        frame's per-layer rotated K / V^T into ring slot count % max_len."""
        rt, C, Hh = self.rt, self.C, self.heads
        P, M = ph * pw, B * ph * pw
        H, W = depth.shape[-2], depth.shape[-1]
        h1, w1 = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
        h2, w2 = (h1 - 7) // 7 + 1, (w1 - 7) // 7 + 1
        assert (h2, w2) == (ph, pw), "mask downsampler output must match the feature grid (memory_encoder.py:173)"
        m1 = rt.fbuf("me_m1", (B, h1, w1))
        rt.mask_down1(depth, m1, B, H, W, h1, w1, self.md1)
        m2 = rt.fbuf("me_m2", (M,))
        rt.mask_down2(m1, m2, B, h1, w1, h2, w2, self.md2)
        x = rt.fbuf("me_x", (M, C))
        rt.gemm(mem_out, self.wpix, M, C, C, bias=self.bpix, rowadd=m2, out=x)
        d = rt.fbuf("me_dw", (M, C))
        # Cross-term path: every ConvNeXt block runs in place on the fp32 stream x, and one pass turns x into the A operand of the
        # pushed frame's key / value projections. Otherwise the last block writes that operand, the mem_feat split planes.
        use8 = self.x8 and rt.x8_rows(M)
        n, h4, feat = rt.operand("me_n", (M, C), use8), rt.operand("me_h4", (M, 4 * C), use8), rt.operand("mem_feat", (M, C), use8)
        for cx in self.cx:
            rt.dwconv7(x, d, B, ph, pw, C, cx["wdw"], cx["bdw"])
            rt.layernorm(d, M, C, cx["nw"], cx["nb"], 1e-6, out_h=n)
            rt.gemm(n, cx["w1"], M, 4 * C, C, bias=cx["b1"], act=GELU, out=h4)
            rt.gemm(h4, cx["w2"], M, C, 4 * C, bias=cx["b2"], gamma=cx["g"], res1=x,
                    out=(feat if cx is self.cx[-1] and not use8 else x))
        if use8:
            rt.pack_x8_f32(x, feat.hi, feat.p8)
        ks, vs, k8s, tp = self._bank(B, P)
        slot = self.state["count"] % self.max_len  # commit() advances the count once every lane has pushed
        cs = self._rope_for(int(math.sqrt(P)))
        for l, L in enumerate(self.layers):
            rt.gemm(feat, L["wkv"], M, 2 * C, C, bias=L["bkv"], store=abi.ST_HEADS,
                    heads=rt.head_split([(ks[l], k8s[l])], vs[l], Hh, P, tp, rope_cs=cs, rope_mod=P, tok_off=slot * P))
