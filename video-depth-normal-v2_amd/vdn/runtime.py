"""Device runtime: workspace arena and tensor-level wrappers over the C-ABI.

PyTorch is plumbing here (device memory, streams); every arithmetic op on the path is a launch of
libvdn_hip.so. Launches go to torch's current stream, so the caller's stream semantics (and
torch.cuda.CUDAGraph capture) apply unchanged. Workspace pointers are stable: buffers come from the
arena by (name, shape, dtype) and nothing is allocated per call after warm-up.
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _abi as abi
from ._abi import F16, BF16, F32
from .pack import Linear, Prec

_TDT = {torch.float16: F16, torch.bfloat16: BF16, torch.float32: F32}
_POISON = bool(int(__import__("os").environ.get("VDN_POISON", "0")))


def ceil_to(x: int, m: int) -> int:
    return (x + m - 1) // m * m


class HL:
    """A 16-bit tensor as (hi, lo) planes; lo is None in single-precision-pass mode. In split ("x3")
    mode value = float(hi) + float(lo) carries ~21 mantissa bits and every MFMA product is
    accumulated as hi*hi + hi*lo + lo*hi (include/vdn.h)."""
    __slots__ = ("hi", "lo")

    def __init__(self, hi: torch.Tensor, lo: Optional[torch.Tensor] = None):
        self.hi, self.lo = hi, lo

    @staticmethod
    def from_float(x: torch.Tensor, half: torch.dtype, split: bool) -> "HL":
        hi = x.to(half)
        if not split:
            return HL(hi.contiguous())
        lo = (x.float() - hi.float()).to(half)
        return HL(hi.contiguous(), lo.contiguous())

    def float(self) -> torch.Tensor:
        return self.hi.float() if self.lo is None else self.hi.float() + self.lo.float()

    @property
    def shape(self):
        return self.hi.shape

    def data_ptr(self):
        return self.hi.data_ptr()

    def narrow0(self, start: int, length: int) -> "HL":
        """Rows [start, start+length) of the leading dimension, both planes (a contiguous view)."""
        return HL(self.hi.narrow(0, start, length), None if self.lo is None else self.lo.narrow(0, start, length))

    def zero_(self):
        self.hi.zero_()
        if self.lo is not None:
            self.lo.zero_()
        return self


class KT:
    """An activation in the cross-term GEMM's operand form (include/vdn.h A8 / a_kt): `hi`, the fp16 hi plane
    K-tile-major, and `p8`, u8 [2, rows, K], the 6-bit rows of hi and of the remainder. There is no fp16 lo plane. Written by
    the LayerNorm, attention and GELU epilogues or by pack_x8 / pack_x8_f32; Runtime.operand hands it out."""
    __slots__ = ("hi", "p8")

    def __init__(self, hi: torch.Tensor, p8: torch.Tensor):
        self.hi, self.p8 = hi, p8


class PadKT:
    """A 3x3 convolution's operand map in the padded-row planes of the cross-term GEMM (include/vdn.h pad_hi): `hi` fp16
    [C/32, Mp, 32] and `p8` u8 [2, C/64, Mp, 64] with Mp = B (H+2) (W+2), views into `hi_store` / `p8_store`, which carry `guard` =
    W + 3 zero rows of 64 bytes in front and behind. Ring rows are zero bits. Written by Runtime.pack_x8_relu_pad and by the two
    epilogues of Runtime.conv3x3_pad; Runtime.pad_operand hands it out."""
    __slots__ = ("hi", "p8", "hi_store", "p8_store", "guard", "B", "H", "W", "C", "rows")

    def __init__(self, hi_store: torch.Tensor, p8_store: torch.Tensor, B: int, H: int, W: int, C: int):
        self.B, self.H, self.W, self.C = B, H, W, C
        self.rows, self.guard = B * (H + 2) * (W + 2), W + 3
        g, Mp = self.guard, self.rows
        self.hi_store, self.p8_store = hi_store, p8_store
        self.hi = hi_store[32 * g:32 * g + C * Mp].view(C // 32, Mp, 32)
        self.p8 = p8_store[64 * g:64 * g + 2 * C * Mp].view(2, C // 64, Mp, 64)


def _hl(t):
    """(hi tensor, lo pointer or None) of an HL, a KT or a plain tensor."""
    if isinstance(t, HL):
        return t.hi, (None if t.lo is None else t.lo.data_ptr())
    return (t.hi, None) if isinstance(t, KT) else (t, None)


_f32, _f64, _u8, _i64 = torch.float32, torch.float64, torch.uint8, torch.int64


def _fits(got, shape) -> bool:
    """Is `got` the `shape`, a None entry of which leaves that dimension free?"""
    if len(got) != len(shape):
        return False
    for w, g in zip(shape, got):
        if w is not None and w != g:
            return False
    return True


def checked_ptr(what: str, t, device: torch.device, dtype, shape=None, count=None, optional: bool = False) -> Optional[int]:
    """The contract of one tensor operand, stated where it becomes a pointer: `t` is a contiguous tensor on `device` of `dtype`
    (one dtype, or a tuple of admissible ones), with exactly `shape` (a None entry leaves that dimension free; an int is a rank,
    every dimension free) and / or `count` elements -> t.data_ptr(). None passes for an `optional` operand. Anything else raises
    VdnError before a pointer is taken; `what` names the wrapper and the operand. The C side sees only the pointer and the
    caller's counts, so this is the last check between a wrong tensor and an out-of-bounds access, and it raises rather than
    asserts: python -O keeps it."""
    if t is None and optional:
        return None
    if (isinstance(t, torch.Tensor) and (t.dtype == dtype or (type(dtype) is tuple and t.dtype in dtype)) and t.is_contiguous()
            and (t.device == device or (device.index is None and t.device.type == device.type))
            and (shape is None or (t.dim() == shape if type(shape) is int else t.shape == shape or _fits(t.shape, shape)))
            and (count is None or t.numel() == count)):
        return t.data_ptr()
    want = " or ".join(str(d) for d in (dtype if type(dtype) is tuple else (dtype,))) + " tensor"
    if shape is not None:
        want += " [" + ", ".join("*" if s is None else str(int(s)) for s in ((None,) * shape if type(shape) is int else shape)) + "]"
    if count is not None:
        want += f" of {int(count)} elements"
    if isinstance(t, torch.Tensor):
        got = f"{t.dtype} {list(t.shape)} on {t.device}" + ("" if t.is_contiguous() else ", not contiguous")
    else:
        got = type(t).__name__
    raise abi.VdnError(f"{what}: expected a contiguous {want} on {device}, got {got}")


class Runtime:
    def __init__(self, device: torch.device, half: torch.dtype = torch.float16, split: bool = False):
        if device.type != "cuda":
            raise abi.VdnError("vdn kernels run on an MI355X ('cuda' device under ROCm); there is no CPU path")
        self.device = device
        self.half = half
        self.split = split
        self.prec = Prec(half, split)
        self.dt = _TDT[half]
        self.zeros = torch.zeros(256, dtype=torch.uint8, device=device)
        self._bufs: Dict[tuple, torch.Tensor] = {}
        self.cu_hint = 0  # vdn_gemm_desc.cu_hint: 0 = whole chip; lanes that co-run set their share
        # MFMA products per P V term of vdn_flash_attn (include/vdn.h), per call: 1 (default) | 2 | 3. Decides which planes the
        # projections write (v_dst / qk_dst) and which kernel every attention launch of this runtime takes — one value per model.
        self.pv_products = int(os.environ.get("VDN_ATTN_PV", "1"))
        assert self.pv_products in (1, 2, 3), self.pv_products
        self.timing: Optional[list] = None  # bench.py: [(tag, start_event, end_event, flop)] for tagged launches

    # ------------------------------------------------------------------ memory
    def buf(self, name: str, shape: Sequence[int], dtype: torch.dtype, zero: bool = False) -> torch.Tensor:
        key = (name, tuple(int(s) for s in shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = (torch.zeros if zero else torch.empty)(key[1], dtype=dtype, device=self.device)
            if not zero and _POISON and t.is_floating_point():
                t.fill_(float("nan"))  # debug: any consumed-before-written element poisons the output
            self._bufs[key] = t
        return t

    def hbuf(self, name, shape, zero=False) -> HL:
        hi = self.buf(name, shape, self.half, zero)
        return HL(hi, self.buf(name + "#lo", shape, self.half, zero) if self.split else None)

    def operand(self, name: str, shape, x8: bool = False):
        """An activation between two linears, by name: the split planes of hbuf, or with `x8` (this call takes the cross-term
        kernel) the KT form, under the arena keys name_kt and name8."""
        if not x8:
            return self.hbuf(name, shape)
        return KT(self.buf(name + "_kt", shape, self.half), self.buf(name + "8", (2, *shape), torch.uint8))

    def pad_operand(self, name: str, B: int, H: int, W: int, C: int) -> PadKT:
        """The padded-row operand planes of a B x H x W x C map, by name (zero-initialised once: nothing ever writes the guard
        rows, and every producer rewrites the ring rows as zeros)."""
        assert C % 64 == 0 and self.half == torch.float16, (C, self.half)
        Mp, g = B * (H + 2) * (W + 2), W + 3
        return PadKT(self.buf(name + "_pkt", (C * Mp + 64 * g,), self.half, zero=True),
                     self.buf(name + "_p8", (2 * C * Mp + 128 * g,), torch.uint8, zero=True), B, H, W, C)

    def x8_capable(self, Cn: int) -> bool:
        """Can an engine whose linears are Cn wide use the cross-term kernel (csrc/gemm_x8.hip)? fp16 split planes only;
        VDN_X8=0 keeps the three-fp16-product kernels."""
        return self.split and self.half == torch.float16 and Cn % 64 == 0 and os.environ.get("VDN_X8", "1") != "0"

    @staticmethod
    def x8_rows(M: int) -> bool:
        """Does a call with M rows take it? Its tiles are 256 x 256: M >= 4096 keeps every launch near a round of the chip
        or more."""
        return M >= int(os.environ.get("VDN_X8_MIN_ROWS", "4096"))

    def to_half(self, x: torch.Tensor) -> HL:
        return HL.from_float(x, self.half, self.split)

    def qk8(self, name: str, bh: int, tpad: int) -> Optional[torch.Tensor]:
        """u8 [bh, tpad, 128] zero-initialised plane pair for the attention's 8-bit cross terms, or None when the
        mode has none (single-product or bf16 planes, or VDN_ATTN_QK8=0)."""
        if not (self.split and self.half == torch.float16) or os.environ.get("VDN_ATTN_QK8", "1") == "0":
            return None
        return self.buf(name, (bh, tpad, 128), torch.uint8, zero=True)

    def v_dst(self, vt: HL) -> HL:
        """Destination planes of a V^T head split: when the attention in use is the one-product P V kernel (fp16 split planes
        with the 8-bit Q / K planes, pv_products 1) nothing ever reads V^T's lo plane,
        so the projection does not write it — 2-byte scattered stores: 218 -> 210 us on the batch-8 QKV GEMM."""
        if (vt.lo is not None and self.half == torch.float16 and os.environ.get("VDN_ATTN_QK8", "1") != "0"
                and self.pv_products == 1):
            return HL(vt.hi, None)
        return vt

    def qk_dst(self, t: HL, t8) -> HL:
        """Destination planes of a Q / K head split: with the 8-bit planes (t8) the attention reads e5m2(lo 2^10) and never
        the fp16 lo plane, so the projection does not write it."""
        if self.pv_products == 3:
            return t   # the 3-product P V kernel (flash_attn_kernel<.., false, false>) takes its score cross terms from the fp16 lo planes
        return HL(t.hi, None) if (t8 is not None and t.lo is not None) else t

    def head_split(self, qk, vt, heads: int, tokens: int, tpad: int, rope_cs=None, rope_mod: int = 0, tok_off: int = 0) -> dict:
        """`heads=` of an ST_HEADS gemm: `qk`, the (planes, 8-bit planes) pairs of its Q / K-like splits in order, then `vt`,
        the V^T planes of the last split, or None. With a RoPE table the Q / K splits are rotated."""
        nv = int(vt is not None)
        return dict(dst=[self.qk_dst(t, t8) for t, t8 in qk] + [self.v_dst(vt) for _ in range(nv)], dst8=[t8 for _, t8 in qk] + [None] * nv,
                    transposed=[0] * len(qk) + [1] * nv, rope=[int(rope_cs is not None)] * len(qk) + [0] * nv, rope_cs=rope_cs,
                    rope_mod=rope_mod, heads=heads, tokens=tokens, tok_off=tok_off, tpad=tpad)

    def fbuf(self, name, shape, zero=False):
        return self.buf(name, shape, torch.float32, zero)

    def workspace_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self._bufs.values())

    def _ws(self, name: str, nbytes: int) -> torch.Tensor:
        """The arena's workspace `name`: at least nbytes, rounded up to whole 8-byte words."""
        return self.buf(name, ((nbytes + 7) // 8,), torch.float64)

    # ------------------------------------------------------------------ launch
    def _launch(self, fn, *args, tag: Optional[str] = None, flop: float = 0.0):
        if tag is not None and self.timing is not None:
            # HIP events on the launch stream (torch's current stream is the stream the kernel runs on)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rc = fn(*args, torch.cuda.current_stream(self.device).cuda_stream)
            e.record()
            self.timing.append((tag, s, e, flop))
        else:
            rc = fn(*args, torch.cuda.current_stream(self.device).cuda_stream)
        abi.check(rc, fn.__name__)

    # ------------------------------------------------------------------ ops
    @staticmethod
    def _p(t: Optional[torch.Tensor]):
        return None if t is None else t.data_ptr()

    def gemm(self, A: torch.Tensor, W: torch.Tensor, M: int, N: int, K: int, *, lda: Optional[int] = None,
             out: Optional[torch.Tensor] = None, ldc: Optional[int] = None, bias=None, act: int = 0, gamma=None,
             rowadd=None, tab=None, tab_mod: int = 0, tab_off: int = 0, res1=None, ldr1=None, res2=None, ldr2=None,
             conv: Optional[dict] = None, relu_a: bool = False, store: int = abi.ST_PLAIN, row_group: int = 0,
             row_skip: int = 0, heads: Optional[dict] = None, convt: Optional[dict] = None, tag: Optional[str] = None,
             a8: Optional[torch.Tensor] = None, w8: Optional[torch.Tensor] = None, out8: Optional[torch.Tensor] = None,
             a_kt: bool = False, w_kt: bool = False, out_kt: bool = False, x8_terms: int = 0,
             subpix_bias: Optional[torch.Tensor] = None, pad: Optional[PadKT] = None, pad_out: Optional[PadKT] = None):
        """A, W and out may be operand objects: a pack.Linear weight follows its activation, on the cross-term kernel for a KT
        (a8 / w8 / a_kt / w_kt filled from the two), else on its split planes, where x8_terms does not apply; a KT `out`
        fills out8 / out_kt. The keywords give the same planes by hand (tests and tools). subpix_bias (with conv= on the
        source map, convt= and store=ST_CONVT; W and the bias shares from pack.subpixel_conv, K = 4 C): the sub-pixel
        convolution mode of include/vdn.h."""
        if isinstance(W, Linear):
            if not isinstance(A, KT):
                W, x8_terms = W.hl, 0
            elif W.x8 is None:
                raise abi.VdnError("vdn_gemm: a cross-term (KT) activation needs a weight packed with X8 planes")
            else:
                a8, w8, a_kt, w_kt, W = A.p8, W.x8.p8, True, True, W.x8.hi
        elif isinstance(A, KT):
            raise abi.VdnError("vdn_gemm: a cross-term (KT) activation needs a pack.Linear weight")
        if isinstance(out, KT):
            out8, out_kt = out.p8, True
        d = abi.GemmDesc()
        d.dt = self.dt
        d.M, d.N, d.K = M, N, K
        A, d.A_lo = _hl(A)
        W, d.W_lo = _hl(W)
        d.A = A.data_ptr()
        d.relu_a = 1 if relu_a else 0
        if conv is not None:
            d.a_mode = abi.A_CONV3X3
            d.cB, d.cH, d.cW, d.cC = conv["B"], conv["H"], conv["W"], conv["C"]
            d.cOH, d.cOW, d.cstride = conv["OH"], conv["OW"], conv["stride"]
            d.lda = conv["C"]
            d.conv_korder = conv.get("korder", 1 if conv["C"] % 64 == 0 else 0)  # must match pack.conv3x3
        elif pad is not None:   # padded-row 3x3 mode (include/vdn.h pad_hi; conv3x3_pad below)
            d.a_mode = abi.A_PAD3X3
            d.cB, d.cH, d.cW, d.cC = pad.B, pad.H, pad.W, pad.C
        else:
            d.a_mode = abi.A_PLAIN
            d.lda = lda if lda is not None else K
        d.W = W.data_ptr()
        d.ldb = W.shape[1]
        assert W.shape[0] == N and W.dtype == self.half and A.dtype == self.half, (W.shape, N, W.dtype, A.dtype)
        assert W.is_contiguous()
        d.bias = self._p(bias)
        d.rowadd = self._p(rowadd)
        d.act = act
        d.gamma = self._p(gamma)
        d.tab = self._p(tab)
        d.tab_mod, d.tab_off = tab_mod, tab_off
        if res1 is not None:
            r1, d.res1_lo = _hl(res1)
            d.res1, d.res1_dt, d.ldr1 = r1.data_ptr(), _TDT[r1.dtype], (ldr1 if ldr1 is not None else N)
        if res2 is not None:
            r2, d.res2_lo = _hl(res2)
            d.res2, d.res2_dt, d.ldr2 = r2.data_ptr(), _TDT[r2.dtype], (ldr2 if ldr2 is not None else N)
        d.store = store
        if out is not None:
            oh, d.out_lo = _hl(out)
            d.out = oh.data_ptr()
            d.out_dt = _TDT[oh.dtype]
            d.ldc = ldc if ldc is not None else (N // 2 if store == abi.ST_GEGLU else N)
        d.row_group, d.row_skip = row_group, row_skip
        if heads is not None:
            dst = heads["dst"]
            d.nsplit = len(dst)
            for i, t in enumerate(dst):
                th, d.dst_lo[i] = _hl(t)
                d.dst[i] = th.data_ptr()
                d.transposed[i] = int(heads["transposed"][i])
                d.rope[i] = int(heads.get("rope", (0, 0, 0))[i])
                t8 = (heads.get("dst8") or (None, None, None))[i]
                if t8 is not None:
                    d.dst8[i] = t8.data_ptr()
            d.heads, d.tokens, d.tok_off, d.tpad = heads["heads"], heads["tokens"], heads.get("tok_off", 0), heads["tpad"]
            if heads.get("rope_cs") is not None:
                d.rope_cs, d.rope_mod = heads["rope_cs"].data_ptr(), heads["rope_mod"]
        if convt is not None:
            d.ck, d.cout = convt["k"], convt["cout"]
            d.cB, d.cH, d.cW = convt["B"], convt["H"], convt["W"]
        d.zeros = self.zeros.data_ptr()
        if a8 is not None and w8 is not None:  # 8-bit cross-term planes of both operands (include/vdn.h A8 / W8)
            d.A8, d.W8 = a8.data_ptr(), w8.data_ptr()
        if out8 is not None:
            d.out8 = out8.data_ptr()
        if pad_out is not None:   # relu of a residual-flavour result as the next convolution's padded operand planes
            d.pad_hi, d.out8 = pad_out.hi.data_ptr(), pad_out.p8.data_ptr()
        d.a_kt, d.w_kt, d.out_kt = int(a_kt), int(w_kt), int(out_kt)   # K-tile-major planes (include/vdn.h)
        d.x8_terms = int(x8_terms)
        if subpix_bias is not None:
            assert subpix_bias.dtype == torch.float32 and subpix_bias.is_contiguous() and subpix_bias.numel() == 4 * N, subpix_bias.shape
            d.subpix, d.subpix_bias = 1, subpix_bias.data_ptr()
        d.cu_hint = self.cu_hint
        if abi.OVERRIDE is not None:   # per-launch kernel-selection knobs (tests / tools); the library itself is stateless
            d.tuning = C.addressof(abi.OVERRIDE)
        if self.split:  # split-K scratch for launches whose tile grid covers a fraction of the chip (include/vdn.h)
            ws = self.buf("splitk_ws", (32 * 1024 * 1024,), torch.float32)
            d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
        self._launch(abi.lib.vdn_gemm, C.byref(d), tag=tag, flop=2.0 * M * N * K)  # the library copies the descriptor before it returns
        return out

    def layernorm(self, x: torch.Tensor, rows: int, Cn: int, w, b, eps: float, *, out_h=None, out_f=None, addvec=None,
                  alpha: float = 1.0, addtab=None, tab_div: int = 1, tab_mod: int = 1, out_group: int = 0, out8=None,
                  kt: bool = False):
        """out8: u8 [2, rows, C] planes of 6-bit rows of the output for the cross-term GEMM (include/vdn.h A8); kt: K-tile-major planes.
        A KT `out_h` gives both."""
        if isinstance(out_h, KT):
            out8, kt = out_h.p8, True
        oh, ol = _hl(out_h) if out_h is not None else (None, None)
        self._launch(abi.lib.vdn_layernorm, x.data_ptr(), _TDT[x.dtype], rows, Cn, w.data_ptr(), b.data_ptr(), eps,
                     self._p(addvec), alpha, self._p(addtab), tab_div, tab_mod, out_group, self._p(oh), ol, self.dt,
                     self._p(out_f), self._p(out8), int(kt))

    def flash_attn(self, Q, K, Vt, out, B: int, H: int, nq: int, nq_pad: int, nk: int, nk_pad: int, scale: float,
                   tag: Optional[str] = None, q8: Optional[torch.Tensor] = None, k8: Optional[torch.Tensor] = None,
                   out8: Optional[torch.Tensor] = None, out_kt: bool = False):
        """q8 / k8: the u8 [B*H, n_pad, 128] planes the projection wrote through heads['dst8'] (8-bit cross terms).
        out8 / out_kt: planes of 6-bit rows of the output and the K-tile-major layout for the cross-term GEMM that follows;
        a KT `out` gives both."""
        if isinstance(out, KT):
            out8, out_kt = out.p8, True
        (Q, ql), (K, kl), (Vt, vl), (out, ol) = _hl(Q), _hl(K), _hl(Vt), _hl(out)
        self._launch(abi.lib.vdn_flash_attn, self.dt, Q.data_ptr(), K.data_ptr(), Vt.data_ptr(), out.data_ptr(), ql, kl,
                     vl, ol, self._p(q8), self._p(k8), self._p(out8), int(out_kt), B, H, nq, nq_pad, nk, nk_pad, scale, self.pv_products, tag=tag,
                     flop=4.0 * B * H * nq * nk * 64)

    def temporal_attn(self, qkv, out, Bv: int, T: int, D: int, c: int, heads: int, scale: float, rope_cs=None):
        (qkv, ql), (out, ol) = _hl(qkv), _hl(out)
        self._launch(abi.lib.vdn_temporal_attn, self.dt, qkv.data_ptr(), out.data_ptr(), ql, ol, Bv, T, D, c, heads, scale,
                     self._p(rope_cs))

    def temporal_attn_last(self, pool: torch.Tensor, slots, pe_q, pe_k, pe_v, out, HW: int, c: int, scale: float):
        """Newest frame attends over the projected cache: `pool` f32 [ring slots, HW, 3c], `slots` the window's ring-slot
        indices, oldest first (host ints: they travel in the launch arguments)."""
        T = len(slots)
        tab = (C.c_int32 * T)(*slots)
        (out, ol) = _hl(out)
        self._launch(abi.lib.vdn_temporal_attn_last, self.dt, pool.data_ptr(), pool.stride(0), tab, T, HW, c, pe_q.data_ptr(),
                     pe_k.data_ptr(), pe_v.data_ptr(), scale, out.data_ptr(), ol)

    def groupnorm(self, x, y, F: int, HW: int, Cn: int, groups: int, w, b, eps: float):
        nsplit = 16 if HW >= 1024 else 4
        part = self.fbuf("gn_partial", (F, nsplit, groups, 2))
        (x, xl), (y, yl) = _hl(x), _hl(y)
        self._launch(abi.lib.vdn_groupnorm, self.dt, x.data_ptr(), xl, y.data_ptr(), yl, F, HW, Cn, groups, w.data_ptr(),
                     b.data_ptr(), eps, part.data_ptr(), nsplit)

    def upsample(self, x, y, B: int, IH: int, IW: int, OH: int, OW: int, Cn: int):
        (x, xl), (y, yl) = _hl(x), _hl(y)
        self._launch(abi.lib.vdn_upsample_bilinear, self.dt, x.data_ptr(), xl, y.data_ptr(), yl, B, IH, IW, OH, OW, Cn)

    def upsample_f32(self, x, y, B: int, IH: int, IW: int, OH: int, OW: int, relu: bool = False):
        dev = self.device
        self._launch(abi.lib.vdn_upsample_bilinear_f32, checked_ptr("upsample_f32: x", x, dev, _f32, count=B * IH * IW),
                     checked_ptr("upsample_f32: y", y, dev, _f32, count=B * OH * OW), B, IH, IW, OH, OW, int(relu))

    def stitch_fit(self, pred: torch.Tensor, target: torch.Tensor, coef: torch.Tensor):
        """coef[0:2] <- least-squares (scale, shift) of pred onto target (utils/util.py:40-62), on the device."""
        dev = self.device
        p = checked_ptr("stitch_fit: pred", pred, dev, _f32)
        n = pred.numel()
        self._launch(abi.lib.vdn_stitch_fit, p, checked_ptr("stitch_fit: target", target, dev, _f32, count=n), n,
                     self._ws("stitch_ws", abi.lib.vdn_stitch_workspace_bytes()).data_ptr(),
                     checked_ptr("stitch_fit: coef", coef, dev, _f32, count=2))

    def stitch_apply(self, window: torch.Tensor, coef: torch.Tensor, out_tail: torch.Tensor, out_new: torch.Tensor,
                     ref1: torch.Tensor, align_len: int, overlap: int, ref_frame: int):
        """window f32 [T, ...] -> out_tail [overlap - align_len, ...], out_new [T - overlap, ...] and ref1 [...], the frame
        `ref_frame` (include/vdn.h vdn_stitch_apply); coef f32 [2] is what stitch_fit wrote."""
        dev = self.device
        w = checked_ptr("stitch_apply: window", window, dev, _f32)
        T, frame = window.shape[0], tuple(window.shape[1:])
        self._launch(abi.lib.vdn_stitch_apply, w, checked_ptr("stitch_apply: coef", coef, dev, _f32, count=2),
                     checked_ptr("stitch_apply: out_tail", out_tail, dev, _f32, (overlap - align_len,) + frame),
                     checked_ptr("stitch_apply: out_new", out_new, dev, _f32, (T - overlap,) + frame),
                     checked_ptr("stitch_apply: ref1", ref1, dev, _f32, frame),
                     window[0].numel(), T, align_len, overlap, ref_frame)

    def dn_stitch_apply(self, depth: torch.Tensor, normal: torch.Tensor, coef: torch.Tensor, out_depth: torch.Tensor,
                        out_normal: torch.Tensor, overlap: int, keep: int, clamp0: bool):
        """One window of the depth + normal model, depth f32 [T, H, W] and normal f32 [T, 3, H, W], into the clip from the
        window's first frame on: out_depth f32 [>= keep, H, W] and out_normal f32 [>= keep, 3, H, W] are the clip's frames
        start .. (include/vdn.h vdn_dn_stitch_apply); coef f32 [2] is what stitch_fit wrote, or {1, 0}."""
        dev = self.device
        d = checked_ptr("dn_stitch_apply: depth", depth, dev, _f32, 3)
        T, H, W = depth.shape
        po = checked_ptr("dn_stitch_apply: out_depth", out_depth, dev, _f32, (None, H, W))
        if out_depth.shape[0] < keep:
            raise abi.VdnError(f"dn_stitch_apply: {keep} frames to write, the clip has {out_depth.shape[0]} left")
        self._launch(abi.lib.vdn_dn_stitch_apply, d, checked_ptr("dn_stitch_apply: normal", normal, dev, _f32, (T, 3, H, W)),
                     checked_ptr("dn_stitch_apply: coef", coef, dev, _f32, count=2), po,
                     checked_ptr("dn_stitch_apply: out_normal", out_normal, dev, _f32, (out_depth.shape[0], 3, H, W)),
                     H * W, T, overlap, keep, int(bool(clamp0)))

    def _eval_args(self, what: str, pred, gt, mask):
        """-> the pointers of f32 pred, gt [T, H, W], the u8 or bool mask [T, H, W] (or None) and the clip's workspace."""
        p = checked_ptr(what + ": pred", pred, self.device, _f32, 3)
        return (p, checked_ptr(what + ": gt", gt, self.device, _f32, pred.shape),
                checked_ptr(what + ": mask", mask, self.device, (_u8, torch.bool), pred.shape, optional=True),
                self._ws("eval_ws", abi.lib.vdn_eval_workspace_bytes(pred.shape[0])).data_ptr())

    def eval_fit(self, pred, gt, mask, dmin: float, dmax: float, domain: int, coef: torch.Tensor):
        """coef[0:2] (float64) <- masked least-squares (scale, shift) of the clip evaluation (include/vdn.h vdn_eval_fit)."""
        p, g, m, ws = self._eval_args("eval_fit", pred, gt, mask)
        self._launch(abi.lib.vdn_eval_fit, p, g, m, pred.shape[0], pred[0].numel(), dmin, dmax, domain, ws,
                     checked_ptr("eval_fit: coef", coef, self.device, _f64, count=2))

    def eval_metrics(self, pred, gt, mask, dmin: float, dmax: float, domain: int, tgm: int, coef: torch.Tensor,
                     out: torch.Tensor):
        """out[0:7] (float64) <- the seven clip metrics; follows eval_fit on the same arguments (vdn_eval_metrics)."""
        p, g, m, ws = self._eval_args("eval_metrics", pred, gt, mask)
        self._launch(abi.lib.vdn_eval_metrics, p, g, m, pred.shape[0], pred.shape[1], pred.shape[2], dmin, dmax, domain, tgm,
                     checked_ptr("eval_metrics: coef", coef, self.device, _f64, count=2), ws,
                     checked_ptr("eval_metrics: out", out, self.device, _f64, count=7))

    def resize_bilinear_hp(self, x: torch.Tensor, out: torch.Tensor):
        """out [T, OH, OW] <- half-pixel (align_corners=False) bilinear resize of f32 x [T, IH, IW]."""
        px = checked_ptr("resize_bilinear_hp: x", x, self.device, _f32, 3)
        po = checked_ptr("resize_bilinear_hp: out", out, self.device, _f32, (x.shape[0], None, None))
        self._launch(abi.lib.vdn_resize_bilinear_hp, px, po, x.shape[0], x.shape[1], x.shape[2], out.shape[1], out.shape[2])

    def sobel_ix_iy(self, depth: torch.Tensor, ix: torch.Tensor, iy: torch.Tensor, normalize_kernel: bool = True):
        """ix, iy f32 [F, H, W] <- Sobel (/ 8) of the reflect-padded f32 depth [F, H, W] (include/vdn.h vdn_sobel_ix_iy)."""
        dev = self.device
        d = checked_ptr("sobel_ix_iy: depth", depth, dev, _f32, 3)
        F, H, W = depth.shape
        self._launch(abi.lib.vdn_sobel_ix_iy, d, checked_ptr("sobel_ix_iy: ix", ix, dev, _f32, depth.shape),
                     checked_ptr("sobel_ix_iy: iy", iy, dev, _f32, depth.shape),
                     F, H, W, int(normalize_kernel))

    def normal_vector(self, depth: torch.Tensor, out: torch.Tensor, normalize_kernel: bool = True, scale_xy: float = 1.0,
                      scale_z: float = 1.0, eps: float = 1e-8):
        """out f32 [F, 3, H, W] <- unit normals of f32 depth [F, H, W] (vdn_normal_vector)."""
        d = checked_ptr("normal_vector: depth", depth, self.device, _f32, 3)
        F, H, W = depth.shape
        self._launch(abi.lib.vdn_normal_vector, d, checked_ptr("normal_vector: out", out, self.device, _f32, (F, 3, H, W)), F, H, W,
                     int(normalize_kernel), scale_xy, scale_z, eps)

    def erode_mask3(self, mask: torch.Tensor, out: torch.Tensor):
        """out u8 [F, H, W] <- 1 where u8 mask and its 3 x 3 neighbours inside the image are non-zero (vdn_erode_mask3)."""
        m = checked_ptr("erode_mask3: mask", mask, self.device, _u8, 3)
        F, H, W = mask.shape
        self._launch(abi.lib.vdn_erode_mask3, m, checked_ptr("erode_mask3: out", out, self.device, _u8, mask.shape), F, H, W)

    def _normal_args(self, what: str, pred, target, mask):
        """-> F, H, W and the pointers of f32 pred [F, 3, H, W], the f32 target, normals [F, 3, H, W] or a depth map [F, H, W],
        and the u8 mask [F, H, W] (or None)."""
        p = checked_ptr(what + ": pred", pred, self.device, _f32, (None, 3, None, None))
        F, _, H, W = pred.shape
        t = checked_ptr(what + ": target", target, self.device, _f32, (F, H, W) if getattr(target, "ndim", 4) == 3 else (F, 3, H, W))
        return F, H, W, p, t, checked_ptr(what + ": mask", mask, self.device, _u8, (F, H, W), optional=True)

    def normal_eval(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], out: torch.Tensor,
                    frame_sums: Optional[torch.Tensor] = None, frame_counts: Optional[torch.Tensor] = None):
        """out[0:2] (float64) <- (1 - masked mean cosine, kept pixels) of pred f32 [F, 3, H, W] against target: normals
        [F, 3, H, W] or a depth map [F, H, W], whose normals are made on the fly (vdn_normal_eval)."""
        dev = self.device
        F, H, W, p, t, m = self._normal_args("normal_eval", pred, target, mask)
        o = checked_ptr("normal_eval: out", out, dev, _f64, count=2)
        fs = checked_ptr("normal_eval: frame_sums", frame_sums, dev, _f64, count=F, optional=True)
        fc = checked_ptr("normal_eval: frame_counts", frame_counts, dev, _i64, count=F, optional=True)
        ws = self._ws("normal_eval_ws", abi.lib.vdn_normal_eval_workspace_bytes(F))
        self._launch(abi.lib.vdn_normal_eval, p, t, int(target.dim() == 3), m, F, H, W, ws.data_ptr(), fs, fc, o)

    def normal_angle_map(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], erode: bool, out: torch.Tensor):
        """out f32 [F, H, W] <- the angle in degrees between pred f32 [F, 3, H, W] and target, normals [F, 3, H, W] or a depth map
        [F, H, W]; NaN where the u8 mask (eroded first with `erode`) drops the pixel (vdn_normal_angle_map)."""
        F, H, W, p, t, m = self._normal_args("normal_angle_map", pred, target, mask)
        self._launch(abi.lib.vdn_normal_angle_map, p, t, int(target.dim() == 3), m, int(erode), F, H, W,
                     checked_ptr("normal_angle_map: out", out, self.device, _f32, (F, H, W)))

    def normal_angle_stats(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], erode: bool, B: int, T: int,
                           rows: torch.Tensor):
        """rows f64 [1 + B + B T, 9] <- n, mean, median, rmse and the five shares of the angles of pred f32 [B T, 3, H, W]
        against target, for the batch, each item and each frame (vdn_normal_angle_stats)."""
        F, H, W, p, t, m = self._normal_args("normal_angle_stats", pred, target, mask)
        if F != B * T:
            raise abi.VdnError(f"normal_angle_stats: {F} frames are not B * T = {B} * {T}")
        r = checked_ptr("normal_angle_stats: rows", rows, self.device, _f64, (1 + B + F, 9))
        nbytes = abi.lib.vdn_normal_angle_stats_workspace_bytes(B, T, H, W)
        if nbytes == 0:
            raise abi.VdnError(f"normal_angle_stats: unsupported shape B, T, H, W = {(B, T, H, W)} (B * T <= 65535)")
        ws = self._ws("normal_angle_ws", nbytes)
        self._launch(abi.lib.vdn_normal_angle_stats, p, t, int(target.dim() == 3), m, int(erode), B, T, H, W, ws.data_ptr(), r)

    def normal_colorize(self, x: torch.Tensor, out: torch.Tensor, bgr: bool = False):
        """out u8 [N, H, W, 3] <- the unit vector of f32 normals x [N, 3, H, W], or of the normals of a depth map x [N, H, W], as
        bytes (vdn_normal_colorize)."""
        from_depth = getattr(x, "ndim", 4) == 3
        px = checked_ptr("normal_colorize: x", x, self.device, _f32, 3 if from_depth else (None, 3, None, None))
        N, H, W = x.shape[0], x.shape[-2], x.shape[-1]
        self._launch(abi.lib.vdn_normal_colorize, px, int(from_depth), int(bgr),
                     checked_ptr("normal_colorize: out", out, self.device, _u8, (N, H, W, 3)), N, H, W)

    def normal_loss_backward(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], count: torch.Tensor,
                             coeff: torch.Tensor, grad: torch.Tensor):
        """grad f32 [F, 3, H, W] <- coeff * d normal_loss / d pred (vdn_normal_loss_backward). pred, target and mask as for
        normal_eval; count float64 [1] is the out[1] normal_eval wrote for them and coeff float64 [1], both on the device."""
        dev = self.device
        F, H, W, p, t, m = self._normal_args("normal_loss_backward", pred, target, mask)
        self._launch(abi.lib.vdn_normal_loss_backward, p, t, int(target.dim() == 3), m, F, H, W,
                     checked_ptr("normal_loss_backward: count", count, dev, _f64, count=1),
                     checked_ptr("normal_loss_backward: coeff", coeff, dev, _f64, count=1),
                     checked_ptr("normal_loss_backward: grad", grad, dev, _f32, pred.shape))

    def _depth_loss_args(self, what: str, keep: float, prediction, target, mask, out, scale_shift, frame_stats, frame_counts,
                         optional: bool):
        """-> B, T, H, W, whether keep < 1 selects the trimmed criterion, and the pointers of f32 prediction and target and the u8
        mask [B, T, H, W], out f64 [20] (trimmed: [40]), scale_shift f32 [B, 2], frame_stats f64 [B T, 4] and frame_counts
        i64 [B T]; `optional`: the last four may be None (the forward)."""
        dev = self.device
        p = checked_ptr(what + ": prediction", prediction, dev, _f32, 4)
        B, T, H, W = shape = prediction.shape
        trimmed = keep < 1.0
        return (B, T, H, W, trimmed, p, checked_ptr(what + ": target", target, dev, _f32, shape), checked_ptr(what + ": mask", mask, dev, _u8, shape),
                checked_ptr(what + ": out", out, dev, _f64, count=40 if trimmed else 20, optional=optional),
                checked_ptr(what + ": scale_shift", scale_shift, dev, _f32, count=2 * B, optional=optional),
                checked_ptr(what + ": frame_stats", frame_stats, dev, _f64, count=4 * B * T, optional=optional),
                checked_ptr(what + ": frame_counts", frame_counts, dev, _i64, count=B * T, optional=optional))

    def depth_loss(self, prediction: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, out: Optional[torch.Tensor],
                   alpha: float = 0.5, scales: int = 4, stable_scale: float = 10.0, scale_shift: Optional[torch.Tensor] = None,
                   frame_stats: Optional[torch.Tensor] = None, frame_counts: Optional[torch.Tensor] = None, keep: float = 1.0):
        """out[0:20] (float64) <- VideoDepthLoss of f32 prediction, target [B, T, H, W] under the u8 mask (vdn_depth_loss;
        include/vdn.h has the layout). out None: the fit alone, into scale_shift f32 [B, 2]. keep = 1 - trim in (0, 1): the
        trimmed criterion and its out[0:40] (vdn_depth_loss_trimmed)."""
        B, T, H, W, trimmed, p, t, m, o, ss, fs, fc = self._depth_loss_args("depth_loss", keep, prediction, target, mask, out,
                                                                            scale_shift, frame_stats, frame_counts, True)
        if out is None and (trimmed or scale_shift is None):
            raise abi.VdnError("depth_loss: out may be None only for the untrimmed fit alone, which writes scale_shift")
        if trimmed:
            ws = self._ws("depth_loss_trimmed_ws", abi.lib.vdn_depth_loss_trimmed_workspace_bytes(B, T))
            entry, extra = abi.lib.vdn_depth_loss_trimmed, (float(keep),)
        else:
            ws = self._ws("depth_loss_ws", abi.lib.vdn_depth_loss_workspace_bytes(B, T))
            entry, extra = abi.lib.vdn_depth_loss, ()
        self._launch(entry, p, t, m, B, T, H, W, float(alpha), int(scales), float(stable_scale), *extra, ws.data_ptr(), ss, fs, fc, o)

    def depth_loss_backward(self, prediction: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, alpha: float, scales: int,
                            stable_scale: float, scale_shift: torch.Tensor, frame_stats: torch.Tensor, frame_counts: torch.Tensor,
                            out: torch.Tensor, coeff: torch.Tensor, grad: torch.Tensor, keep: float = 1.0):
        """grad f32 [B, T, H, W] <- the gradient of c_sp * spatial + c_st * stable + c_ar * absRel with respect to the f32
        prediction (vdn_depth_loss_backward; keep < 1: vdn_depth_loss_trimmed_backward), coeff f32 [3] = {c_sp, c_st, c_ar} on
        the device. scale_shift, frame_stats, frame_counts and out are what depth_loss wrote for the same inputs and arguments."""
        B, T, H, W, trimmed, p, t, m, o, ss, fs, fc = self._depth_loss_args("depth_loss_backward", keep, prediction, target, mask, out,
                                                                            scale_shift, frame_stats, frame_counts, False)
        c = checked_ptr("depth_loss_backward: coeff", coeff, self.device, _f32, count=3)
        g = checked_ptr("depth_loss_backward: grad", grad, self.device, _f32, prediction.shape)
        size, entry = ((abi.lib.vdn_depth_loss_trimmed_backward_workspace_bytes, abi.lib.vdn_depth_loss_trimmed_backward) if trimmed
                       else (abi.lib.vdn_depth_loss_backward_workspace_bytes, abi.lib.vdn_depth_loss_backward))
        ws = self._ws("depth_loss_backward_ws", size(B, T, H, W))
        self._launch(entry, p, t, m, B, T, H, W, float(alpha), int(scales), float(stable_scale), ss, fs, fc, o, c, ws.data_ptr(), g)

    def _ssim_args(self, what: str, prediction, target, mask, scale_shift, out, frame_cs, item_max):
        """-> B, T, H, W and the pointers of f32 prediction and target and the u8 mask [B, T, H, W], scale_shift f32 [B, 2] or
        None, out f64 [4], frame_cs f64 [B T] and item_max f64 [B, 4] (include/vdn.h, vdn_ssim_loss)."""
        dev = self.device
        p = checked_ptr(what + ": prediction", prediction, dev, _f32, 4)
        B, T, H, W = shape = prediction.shape
        return (B, T, H, W, p, checked_ptr(what + ": target", target, dev, _f32, shape), checked_ptr(what + ": mask", mask, dev, _u8, shape),
                checked_ptr(what + ": scale_shift", scale_shift, dev, _f32, count=2 * B, optional=True),
                checked_ptr(what + ": out", out, dev, _f64, count=4), checked_ptr(what + ": frame_cs", frame_cs, dev, _f64, count=B * T),
                checked_ptr(what + ": item_max", item_max, dev, _f64, count=4 * B))

    def ssim_loss(self, prediction: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, scale_shift: Optional[torch.Tensor],
                  out: torch.Tensor, frame_cs: torch.Tensor, item_max: torch.Tensor):
        """out f64 [4], frame_cs f64 [B T], item_max f64 [B, 4] <- the SSIM term of f32 prediction, target [B, T, H, W] under the
        u8 mask (vdn_ssim_loss); scale_shift f32 [B, 2]: on the aligned prediction."""
        B, T, H, W, p, t, m, ss, o, fc, im = self._ssim_args("ssim_loss", prediction, target, mask, scale_shift, out, frame_cs, item_max)
        ws = self._ws("ssim_loss_ws", abi.lib.vdn_ssim_loss_workspace_bytes(B, T, H, W))
        self._launch(abi.lib.vdn_ssim_loss, p, t, m, ss, B, T, H, W, ws.data_ptr(), o, fc, im)

    def ssim_loss_backward(self, prediction: torch.Tensor, target: torch.Tensor, mask: torch.Tensor, scale_shift: Optional[torch.Tensor],
                           out: torch.Tensor, frame_cs: torch.Tensor, item_max: torch.Tensor, coeff: torch.Tensor, grad: torch.Tensor,
                           accumulate: bool = False):
        """grad f32 [B, T, H, W] <- (accumulate: +=, rounded once) the gradient of coeff * ssim_loss with respect to the f32
        prediction (vdn_ssim_loss_backward); coeff f32 [1] on the device; out, frame_cs and item_max are what ssim_loss wrote for
        the same inputs and scale_shift."""
        B, T, H, W, p, t, m, ss, o, fc, im = self._ssim_args("ssim_loss_backward", prediction, target, mask, scale_shift, out, frame_cs,
                                                             item_max)
        c = checked_ptr("ssim_loss_backward: coeff", coeff, self.device, _f32, count=1)
        g = checked_ptr("ssim_loss_backward: grad", grad, self.device, _f32, prediction.shape)
        ws = self._ws("ssim_loss_backward_ws", abi.lib.vdn_ssim_loss_backward_workspace_bytes(B, T, H, W))
        self._launch(abi.lib.vdn_ssim_loss_backward, p, t, m, ss, B, T, H, W, o, fc, im, c, int(bool(accumulate)), ws.data_ptr(), g)

    def prep_rgb(self, x: torch.Tensor, out: torch.Tensor, normalize: bool):
        """out f32 [F, 3, H, W] <- clamp(x, 0, 1), then the ImageNet mean / std when `normalize` (vdn_prep_rgb); out may be x."""
        px = checked_ptr("prep_rgb: x", x, self.device, _f32, (None, 3, None, None))
        F, _, H, W = x.shape
        self._launch(abi.lib.vdn_prep_rgb, px, checked_ptr("prep_rgb: out", out, self.device, _f32, x.shape), F, H, W, int(normalize))

    def prep_depth(self, x: torch.Tensor, mask: Optional[torch.Tensor], out: torch.Tensor, reciprocal: bool, clamp0: bool,
                   normalize: bool, minmax: Optional[torch.Tensor] = None):
        """out f32 [B, n] <- the stages of vdn_prep_depth on f32 x [B, n] under the u8 mask [B, n] (None: all kept);
        minmax f32 [B, 2] receives the (lo, hi) of the normalisation."""
        dev = self.device
        px = checked_ptr("prep_depth: x", x, dev, _f32, 2)
        B, n = x.shape
        ws = self._ws("prep_depth_ws", abi.lib.vdn_prep_depth_workspace_bytes(B)).data_ptr() if normalize else None
        self._launch(abi.lib.vdn_prep_depth, px, checked_ptr("prep_depth: mask", mask, dev, _u8, x.shape, optional=True),
                     checked_ptr("prep_depth: out", out, dev, _f32, x.shape), B, n, int(reciprocal), int(clamp0), int(normalize), ws,
                     checked_ptr("prep_depth: minmax", minmax, dev, _f32, count=2 * B, optional=True))

    @staticmethod
    def _bounds(bounds):
        return (0, 0.0, 0.0) if bounds is None else (1, float(bounds[0]), float(bounds[1]))

    def metric_eval(self, pred: torch.Tensor, depth: torch.Tensor, valid: Optional[torch.Tensor], out: torch.Tensor, bounds=None):
        """out f64 [B, 10] <- n and eval_depth's nine metrics of f32 pred [B, h, w] against f32 depth [B, H, W] under the u8
        mask [B, H, W] (byte == 1 keeps; None: all kept) and, with bounds = (min_depth, max_depth), those (vdn_metric_eval)."""
        dev = self.device
        d = checked_ptr("metric_eval: depth", depth, dev, _f32, 3)
        B, H, W = depth.shape
        p = checked_ptr("metric_eval: pred", pred, dev, _f32, (B, None, None))
        self._launch(abi.lib.vdn_metric_eval, p, d, checked_ptr("metric_eval: valid", valid, dev, _u8, depth.shape, optional=True), B, pred.shape[1],
                     pred.shape[2], H, W, *self._bounds(bounds), self._ws("metric_ws", abi.lib.vdn_metric_workspace_bytes(B)).data_ptr(),
                     checked_ptr("metric_eval: out", out, dev, _f64, (B, 10)))

    def _silog_args(self, what: str, pred, target, mask):
        """-> the element count and the pointers of f32 pred and target and the u8 mask (or None) of that many elements."""
        p = checked_ptr(what + ": pred", pred, self.device, _f32)
        n = pred.numel()
        return (n, p, checked_ptr(what + ": target", target, self.device, _f32, count=n),
                checked_ptr(what + ": mask", mask, self.device, _u8, count=n, optional=True))

    def silog_loss(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], out: torch.Tensor, lambd: float,
                   bounds=None):
        """out f64 [4] <- loss | n | sum dl | sum dl^2 of SiLogLoss over f32 pred, target and the u8 mask of equal size
        (vdn_silog_loss)."""
        n, p, t, m = self._silog_args("silog_loss", pred, target, mask)
        self._launch(abi.lib.vdn_silog_loss, p, t, m, n, float(lambd), *self._bounds(bounds),
                     self._ws("silog_ws", abi.lib.vdn_silog_loss_workspace_bytes()).data_ptr(),
                     checked_ptr("silog_loss: out", out, self.device, _f64, count=4))

    def silog_loss_backward(self, pred: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor], state: torch.Tensor,
                            coeff: torch.Tensor, grad: torch.Tensor, lambd: float, bounds=None):
        """grad f32 <- coeff * d loss / d pred (vdn_silog_loss_backward); state is what silog_loss wrote for the same inputs
        and arguments, coeff f32 [1] on the device."""
        dev = self.device
        n, p, t, m = self._silog_args("silog_loss_backward", pred, target, mask)
        self._launch(abi.lib.vdn_silog_loss_backward, p, t, m, n, float(lambd), *self._bounds(bounds),
                     checked_ptr("silog_loss_backward: state", state, dev, _f64, count=4),
                     checked_ptr("silog_loss_backward: coeff", coeff, dev, _f32, count=1),
                     checked_ptr("silog_loss_backward: grad", grad, dev, _f32, count=n))

    def minmax(self, x: torch.Tensor, groups: int, out: torch.Tensor):
        """out f32 [groups, 2] <- {min, max} of each of the `groups` equal runs of contiguous f32 x (vdn_minmax_f32)."""
        px = checked_ptr("minmax: x", x, self.device, _f32)
        if groups < 1 or x.numel() % groups:
            raise abi.VdnError(f"minmax: {x.numel()} elements are not {groups} equal runs")
        self._launch(abi.lib.vdn_minmax_f32, px, groups, x.numel() // groups,
                     self._ws("minmax_ws", abi.lib.vdn_minmax_workspace_bytes(groups)).data_ptr(),
                     checked_ptr("minmax: out", out, self.device, _f32, count=2 * groups))

    def colorize(self, depth: torch.Tensor, minmax: torch.Tensor, lut: torch.Tensor, out: torch.Tensor,
                 raw: Optional[torch.Tensor] = None, margin: int = 0):
        """out u8 <- palette pixels of f32 depth [N, H, W] (vdn_colorize): [N, H, W, ch], or with raw u8 [N, H, W, 3]
        [N, H, 2W + margin, 3]. minmax f32 [N, 2] (per frame) or [1, 2]; lut u8 [256, ch]."""
        dev = self.device
        d = checked_ptr("colorize: depth", depth, dev, _f32, 3)
        N, H, W = depth.shape
        table = checked_ptr("colorize: lut", lut, dev, _u8, (256, None))
        ch = lut.shape[1]
        per_frame = N > 1 and isinstance(minmax, torch.Tensor) and minmax.numel() == 2 * N
        self._launch(abi.lib.vdn_colorize, d, checked_ptr("colorize: minmax", minmax, dev, _f32, count=2 * N if per_frame else 2),
                     int(per_frame), table,
                     ch, checked_ptr("colorize: raw", raw, dev, _u8, (N, H, W, 3), optional=True), margin,
                     checked_ptr("colorize: out", out, dev, _u8, count=N * H * W * ch if raw is None else N * H * (2 * W + margin) * 3), N, H, W)

    def frame_median(self, x: torch.Tensor, median: torch.Tensor):
        """median[f] = torch.quantile(x[f], 0.5) for f32 x [F, ...] (exact radix select on the device)."""
        px = checked_ptr("frame_median: x", x, self.device, _f32)
        F = x.shape[0]
        self._launch(abi.lib.vdn_frame_median, px, F, x[0].numel(), checked_ptr("frame_median: median", median, self.device, _f32, count=F),
                     self._ws("median_ws", abi.lib.vdn_frame_median_workspace_bytes(F)).data_ptr())

    def refine_scale(self, x, median, w: float, b: float, max_log_scale: float, max_depth: float, out, scale_out=None):
        """out f32, of x's size <- x / max_depth * s_f for f32 x [F, ...] with s_f from median f32 [F] (vdn_refine_scale);
        scale_out f32 [F] receives s_f."""
        dev = self.device
        px = checked_ptr("refine_scale: x", x, dev, _f32)
        F = x.shape[0]
        self._launch(abi.lib.vdn_refine_scale, px, checked_ptr("refine_scale: median", median, dev, _f32, count=F), F, x[0].numel(), w, b,
                     max_log_scale, max_depth, checked_ptr("refine_scale: out", out, dev, _f32, count=x.numel()),
                     checked_ptr("refine_scale: scale_out", scale_out, dev, _f32, count=F, optional=True))

    def refine_pack(self, d, out, normals: bool = True):
        """out f32 [F, 3, H, W] <- (d, nx, ny) of f32 d [F, H, W], or d on all three planes without `normals` (vdn_refine_pack)."""
        pd = checked_ptr("refine_pack: d", d, self.device, _f32, 3)
        F, H, W = d.shape
        self._launch(abi.lib.vdn_refine_pack, pd, checked_ptr("refine_pack: out", out, self.device, _f32, (F, 3, H, W)), F, H, W, int(normals))

    def refine_finish(self, scaled, depth, w: float, b: float, max_depth: float, residual: bool, out):
        """out <- (scaled + (w * depth + b)) * max_depth, or depth * max_depth without `residual`, over f32 tensors of depth's size
        (vdn_refine_finish); scaled may be None where it is not read."""
        dev = self.device
        pd = checked_ptr("refine_finish: depth", depth, dev, _f32)
        n = depth.numel()
        self._launch(abi.lib.vdn_refine_finish, checked_ptr("refine_finish: scaled", scaled, dev, _f32, count=n, optional=not residual), pd, w, b,
                     max_depth, int(residual), checked_ptr("refine_finish: out", out, dev, _f32, count=n), n)

    def refine_normalize(self, x, max_depth: float, out):
        """out = x / max_depth (true fp32 division) for contiguous f32 tensors of equal size."""
        px = checked_ptr("refine_normalize: x", x, self.device, _f32)
        self._launch(abi.lib.vdn_refine_normalize, px, max_depth,
                     checked_ptr("refine_normalize: out", out, self.device, _f32, count=x.numel()), x.numel())

    def refine_mix(self, depth, x, a0: float, a1: float, c0: float, a2: float, c1: float, out):
        """out = relu(a2 * relu(a0 * depth + a1 * x + c0) + c1): the v2 refiner's final_res, BatchNorms folded (refiner.fold_final_res)."""
        dev = self.device
        pd = checked_ptr("refine_mix: depth", depth, dev, _f32)
        n = depth.numel()
        self._launch(abi.lib.vdn_refine_mix, pd, checked_ptr("refine_mix: x", x, dev, _f32, count=n), a0, a1, c0, a2, c1,
                     checked_ptr("refine_mix: out", out, dev, _f32, count=n), n)

    def refine_window_tail(self, net, scaled, slots, kind: int, residual: bool, coef, out):
        """out f32 [T, OH, OW] <- the finish of one window (vdn_refine_window_tail): net f32 [T, IH, IW] is the head's rectified
        map (sampled at the output pixels where the sizes differ), scaled f32 [frames, OH, OW] the clip's scaled input, slots
        int32 [T] the clip frame each slot shows (range-checked by the caller before the upload), coef five floats: (w, b, unit,
        0, 0) for abi.TAIL_SHIFT, refiner.fold_final_res's for abi.TAIL_MIX. scaled may be None where it is not read."""
        dev = self.device
        po = checked_ptr("refine_window_tail: out", out, dev, _f32, 3)
        T, OH, OW = out.shape
        pn = checked_ptr("refine_window_tail: net", net, dev, _f32, (T, None, None))
        reads = kind == abi.TAIL_MIX or bool(residual)
        ps = checked_ptr("refine_window_tail: scaled", scaled, dev, _f32, (None, OH, OW), optional=not reads)
        if kind not in (abi.TAIL_SHIFT, abi.TAIL_MIX) or len(coef) != 5:
            raise abi.VdnError(f"refine_window_tail: kind {kind} with {len(coef)} coefficients")
        frames = scaled.shape[0] if scaled is not None else 1 << 30   # nothing of `scaled` is indexed then
        self._launch(abi.lib.vdn_refine_window_tail, pn, net.shape[1], net.shape[2], ps, frames,
                     C.cast(checked_ptr("refine_window_tail: slots", slots, dev, torch.int32, (T,)), C.POINTER(C.c_int32)), T, OH, OW, int(kind), int(bool(residual)),
                     *(float(c) for c in coef), po)

    def dn_attn(self, qkv, out, rows: int, Cn: int, heads: int, L: int, estride: int, n0: int, s0: int, n1: int, s1: int,
                scale: float):
        """Grouped self-attention of the depth + normal head (include/vdn.h vdn_dn_attn): qkv [rows, 3C], out [rows, C]."""
        (qh, ql), (oh, ol) = _hl(qkv), _hl(out)
        self._launch(abi.lib.vdn_dn_attn, self.dt, qh.data_ptr(), ql, oh.data_ptr(), ol, rows, Cn, heads, L, estride, n0, s0,
                     n1, s1, scale, tag="dn_attn", flop=4.0 * n0 * n1 * L * L * Cn)

    def dn_prologue(self, a: torch.Tensor, b: Optional[torch.Tensor], frames: int, Cn: int, hw: int, ape=None, S: int = 1,
                    out_f=None, out_h=None):
        """Trunk features (f32, per frame a flat [C*hw] array) -> token rows [frames*hw, C] (include/vdn.h vdn_dn_prologue)."""
        for t in (a, b):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == frames * Cn * hw), t
        oh, ol = _hl(out_h) if out_h is not None else (None, None)
        self._launch(abi.lib.vdn_dn_prologue, self.dt, a.data_ptr(), self._p(b), frames, Cn, hw, self._p(ape), S,
                     self._p(out_f), self._p(oh), ol)

    def dn_tail(self, x, F: int, IH: int, IW: int, Cn: int, w, bias, OH: int, OW: int, depth_in=None, relu: bool = False,
                raw=None, depth=None, normal=None):
        """conv3x3 Cin->3 + bias [-> resize] -> raw and / or (depth, normal) (include/vdn.h vdn_dn_tail)."""
        assert x.dtype == torch.float32 and x.is_contiguous()
        self._launch(abi.lib.vdn_dn_tail, x.data_ptr(), F, IH, IW, Cn, w.data_ptr(), bias.data_ptr(), OH, OW, self._p(depth_in),
                     int(relu), self._p(raw), self._p(depth), self._p(normal))

    def hiera_embed(self, img: torch.Tensor, rows, frames: int, ldk: int):
        """f32 [frames, 3, 224, 224] -> the 7 x 7 patch rows [frames*3136, ldk] in unrolled token order (include/vdn.h)."""
        assert img.dtype == torch.float32 and img.is_contiguous() and tuple(img.shape) == (frames, 3, 224, 224), img.shape
        rows, rl = _hl(rows)
        self._launch(abi.lib.vdn_hiera_embed, self.dt, img.data_ptr(), rows.data_ptr(), rl, frames, ldk)

    def hiera_attn(self, qkv, out, frames: int, heads: int, W: int, Lkv: int, q_stride: int, scale: float):
        """Mask-unit / global attention of the Hiera trunk (include/vdn.h vdn_hiera_attn): qkv [frames*W*Lkv, 3*heads*96]."""
        (qh, ql), (oh, ol) = _hl(qkv), _hl(out)
        assert qh.numel() == frames * W * Lkv * 3 * heads * 96 and oh.numel() * q_stride == frames * W * Lkv * heads * 96
        self._launch(abi.lib.vdn_hiera_attn, self.dt, qh.data_ptr(), ql, oh.data_ptr(), ol, frames, heads, W, Lkv, q_stride, scale,
                     tag="hiera_attn", flop=4.0 * frames * W * heads * (Lkv // q_stride) * Lkv * 96)

    def hiera_pool(self, x: torch.Tensor, y: torch.Tensor, frames: int, n: int, Cn: int):
        assert x.dtype == y.dtype == torch.float32 and x.numel() == frames * 4 * n * Cn and y.numel() == frames * n * Cn
        self._launch(abi.lib.vdn_hiera_pool, x.data_ptr(), y.data_ptr(), frames, n, Cn)

    def hiera_reroll(self, tokens: torch.Tensor, out: torch.Tensor, frames: int, stage: int, Cn: int):
        side = 56 >> stage
        assert tokens.dtype == out.dtype == torch.float32 and tokens.numel() == out.numel() == frames * side * side * Cn
        assert out.is_contiguous()
        self._launch(abi.lib.vdn_hiera_reroll, tokens.data_ptr(), out.data_ptr(), frames, stage, Cn)

    def patchify(self, img, rows, B: int, H: int, W: int, ldk: int):
        rows, rl = _hl(rows)
        self._launch(abi.lib.vdn_patchify, self.dt, img.data_ptr(), rows.data_ptr(), rl, B, H, W, ldk)

    def fill_row(self, x, vec, B: int, rows_per_b: int, row: int, Cn: int):
        self._launch(abi.lib.vdn_fill_row, x.data_ptr(), vec.data_ptr(), B, rows_per_b, row, Cn)

    def bicubic(self, src, dst, ih: int, iw: int, oh: int, ow: int, Cn: int, scale_rows: float, scale_cols: float):
        self._launch(abi.lib.vdn_bicubic, src.data_ptr(), dst.data_ptr(), ih, iw, oh, ow, Cn, scale_rows, scale_cols)

    def preprocess_u8(self, frames_u8: torch.Tensor, H: int, W: int, mean, std, swap_rb: bool = False,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """u8 [n,h,w,3] on the device -> normalised f32 [n,3,H,W] (cubic resize + /255 + mean / std), one launch.
        `out`: a contiguous f32 [n,3,H,W] to write instead of a fresh tensor."""
        src = checked_ptr("preprocess_u8: frames_u8", frames_u8, self.device, _u8, (None, None, None, 3))
        n, h, w, _ = frames_u8.shape
        if out is None:
            out = torch.empty((n, 3, H, W), dtype=torch.float32, device=self.device)
        m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        self._launch(abi.lib.vdn_preprocess, src, n, h, w, int(swap_rb),
                     checked_ptr("preprocess_u8: out", out, self.device, _f32, (n, 3, H, W)), H, W, m3, s3)
        return out

    def add_vec(self, x, vec, alpha: float, y, rows: int, Cn: int):
        self._launch(abi.lib.vdn_add_vec, x.data_ptr(), vec.data_ptr(), alpha, y.data_ptr(), rows, Cn)

    @staticmethod
    def _out_act(relu: bool, act: Optional[int]) -> int:
        """Final activation of a DPT head (include/vdn.h VDN_OUT_*): `act` where given, else the older relu flag."""
        if act is None:
            return abi.OUT_RELU if relu else abi.OUT_NONE
        if act not in (abi.OUT_NONE, abi.OUT_RELU, abi.OUT_SIGMOID):
            raise ValueError(f"act must be one of OUT_NONE, OUT_RELU, OUT_SIGMOID (0, 1, 2), got {act!r}")
        return act

    def depth_tail(self, x: torch.Tensor, w: HL, bias2, w1, b1: float, depth, B: int, IH: int, IW: int, Cn: int, OH: int,
                   OW: int, relu: bool = False, act: Optional[int] = None, out_scale: float = 1.0):
        """resize(align_corners) -> conv3x3 + ReLU -> conv1x1 -> final activation in one launch; x f32 NHWC (split-plane modes
        only). act (abi.OUT_*) overrides relu; OUT_SIGMOID writes out_scale * sigmoid (include/vdn.h vdn_depth_tail_act)."""
        assert x.dtype == torch.float32 and x.is_contiguous() and w.lo is not None and w.hi.shape[0] == 32
        self._launch(abi.lib.vdn_depth_tail_act, self.dt, x.data_ptr(), B, IH, IW, Cn, w.hi.data_ptr(), w.lo.data_ptr(),
                     w.hi.shape[1], bias2.data_ptr(), w1.data_ptr(), b1, depth.data_ptr(), OH, OW, self._out_act(relu, act),
                     float(out_scale))

    @staticmethod
    def lowres_oc1_rows(M: int) -> bool:
        """Does a DPT head whose 8x map has M rows run output_conv1 at the low resolution (DPTEngine.run)? Small maps keep
        the materialised path1."""
        return M >= int(os.environ.get("VDN_OC1_LOWRES_MIN_ROWS", "65536"))

    def oc1_combine(self, z: torch.Tensor, bias, out: torch.Tensor, B: int, IH: int, IW: int, OH: int, OW: int, Cn: int):
        """z f32 [B*IH*IW, 9*Cn] (nine tap images per source pixel) -> out f32 [B*OH*OW, Cn] (include/vdn.h vdn_oc1_combine)."""
        assert z.dtype == torch.float32 and z.is_contiguous() and z.numel() == B * IH * IW * 9 * Cn, (z.shape, z.dtype)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * OH * OW * Cn, (out.shape, out.dtype)
        self._launch(abi.lib.vdn_oc1_combine, z.data_ptr(), bias.data_ptr(), out.data_ptr(), B, IH, IW, OH, OW, Cn)

    def head_out(self, feat, w, bias: float, depth, M: int, Cn: int, relu: bool = False, act: Optional[int] = None,
                 out_scale: float = 1.0):
        """The closing 1x1 convolution and its final activation, as depth_tail takes it (include/vdn.h vdn_head_out_act)."""
        feat, fl = _hl(feat)
        self._launch(abi.lib.vdn_head_out_act, self.dt, feat.data_ptr(), fl, w.data_ptr(), bias, depth.data_ptr(), M, Cn,
                     self._out_act(relu, act), float(out_scale))

    def depth_to_points(self, depth: torch.Tensor, rgb: torch.Tensor, fx: float, fy: float, points: torch.Tensor,
                        colors: torch.Tensor):
        """points, colors f64 [h*w, 3] <- the point cloud of depth f32 [h, w] and rgb u8 [h, w, 3] (vdn_depth_to_points)."""
        dev = self.device
        d = checked_ptr("depth_to_points: depth", depth, dev, _f32, 2)
        h, w = depth.shape
        self._launch(abi.lib.vdn_depth_to_points, d, checked_ptr("depth_to_points: rgb", rgb, dev, _u8, (h, w, 3)), h, w, float(fx), float(fy),
                     checked_ptr("depth_to_points: points", points, dev, _f64, (h * w, 3)),
                     checked_ptr("depth_to_points: colors", colors, dev, _f64, (h * w, 3)))

    def mask_down1(self, depth, out, B, H, W, OH, OW, w):
        self._launch(abi.lib.vdn_mask_down1, depth.data_ptr(), out.data_ptr(), B, H, W, OH, OW, w.data_ptr())

    def mask_down2(self, x, out, B, H, W, OH, OW, w):
        self._launch(abi.lib.vdn_mask_down2, x.data_ptr(), out.data_ptr(), B, H, W, OH, OW, w.data_ptr())

    def dwconv7(self, x, y, B, H, W, Cn, w, bias):
        self._launch(abi.lib.vdn_dwconv7, x.data_ptr(), y.data_ptr(), B, H, W, Cn, w.data_ptr(), bias.data_ptr())

    def addtab_cast(self, x, tab, tab_div: int, tab_mod: int, y, rows: int, Cn: int):
        yh, yl = _hl(y)
        self._launch(abi.lib.vdn_addtab_cast, self.dt, x.data_ptr(), self._p(tab), tab_div, tab_mod, yh.data_ptr(), yl, rows, Cn)

    def pack_x8(self, t: HL, hi_kt: torch.Tensor, planes8: torch.Tensor, order: int = 0):
        """Split planes [rows, ld] -> the K-tile-major hi plane and the two planes of 6-bit rows of the cross-term GEMM's A operand
        (include/vdn.h vdn_pack_x8), for activations whose producer writes plain split planes."""
        rows, ld = t.hi.shape
        self._launch(abi.lib.vdn_pack_x8, t.hi.data_ptr(), t.lo.data_ptr(), rows, ld, hi_kt.data_ptr(), planes8.data_ptr(), 1, order)

    def pack_x8_relu_pad(self, x: HL, out: PadKT):
        """relu(x), split planes [B H W, C] row-major -> the padded-row operand planes `out` (include/vdn.h vdn_pack_x8_relu_pad)."""
        assert x.lo is not None and tuple(x.hi.shape) == (out.B * out.H * out.W, out.C) and x.hi.dtype == torch.float16, x.hi.shape
        self._launch(abi.lib.vdn_pack_x8_relu_pad, x.hi.data_ptr(), x.lo.data_ptr(), out.B, out.H, out.W, out.C, out.hi.data_ptr(),
                     out.p8.data_ptr())

    def conv3x3_pad(self, a: PadKT, w, N: int, bias: torch.Tensor, *, out_pad: Optional[PadKT] = None, out: Optional[HL] = None,
                    res1: Optional[HL] = None, res2: Optional[HL] = None, tag: Optional[str] = None):
        """3x3, stride 1, pad 1 convolution of the padded-row operand `a` with `w` (pack.conv3x3_x8) on the cross-term kernel.
        Without `out`: relu(conv + bias) -> `out_pad`, the next convolution's operand. With `out` (unpadded split planes
        [B H W, N]): conv + bias + res1 [+ res2] -> out, and relu of it -> `out_pad` if given."""
        kw = dict(a8=a.p8, w8=w.p8, a_kt=True, w_kt=True, bias=bias, pad=a, tag=tag)
        if out is None:
            assert out_pad is not None and res1 is None and res2 is None and (out_pad.B, out_pad.H, out_pad.W, out_pad.C) == (a.B, a.H, a.W, N)
            self.gemm(HL(a.hi), HL(w.hi), a.rows, N, 9 * a.C, out=HL(out_pad.hi.view(-1, N)), out8=out_pad.p8, out_kt=True, act=abi.ACT_RELU, **kw)
            return out_pad
        assert res1 is not None and tuple(out.hi.shape) == (a.B * a.H * a.W, N)
        assert out_pad is None or (out_pad.B, out_pad.H, out_pad.W, out_pad.C) == (a.B, a.H, a.W, N)
        self.gemm(HL(a.hi), HL(w.hi), a.rows, N, 9 * a.C, out=out, res1=res1, res2=res2, pad_out=out_pad, **kw)
        return out

    def pack_x8_f32(self, x: torch.Tensor, hi_kt: torch.Tensor, planes8: torch.Tensor):
        """fp32 [rows, ld] -> the cross-term GEMM's A operand (include/vdn.h vdn_pack_x8_f32)."""
        rows, ld = x.shape
        self._launch(abi.lib.vdn_pack_x8_f32, x.data_ptr(), rows, ld, hi_kt.data_ptr(), planes8.data_ptr())

    def cast(self, x, y):
        self._launch(abi.lib.vdn_cast, x.data_ptr(), _TDT[x.dtype], y.data_ptr(), _TDT[y.dtype], x.numel())
