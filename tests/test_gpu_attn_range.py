"""The five attention kernels at logit ranges where softmax goes wrong: every score pattern of tests/attn_cases.py (offsets of
+-120, ramps that cross the lazy-rescale threshold every tile or every second tile, one-hot rows, flat rows, a query tile that
mixes rows of maximum -40 and +120) against plain fp64 attention on the values the operand planes hold. The bar of a run is
the bar the kernel's own randn test holds, raised to 4x the error of plain fp32 torch attention on the same inputs where that
is larger (attn_cases.bars). tests/test_attn_cases_host.py shows that these patterns catch an unstable softmax; each run here
prints one table row (profiles/attn_range.md), asserts a finite output under the bars and a bitwise equal second call."""
import pytest
import torch

import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16 = torch.float16
NAN = float("nan")
PV_DEFAULT = 1   # default pv_products of vdn_flash_attn (include/vdn.h)


@pytest.fixture(scope="module")
def rts():
    """{split: Runtime}"""
    from vdn import _abi
    from vdn.runtime import Runtime
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    assert _abi.lib.vdn_arch_ok() == 1, "not a gfx950 device"
    return {split: Runtime(DEV, F16, split=split) for split in (False, True)}


def _planes(x, split):
    """fp32 CPU tensor -> (HL on the device, the values its planes hold as fp32 on the CPU)."""
    from vdn.runtime import HL
    p = HL.from_float(x, F16, split)
    return HL(p.hi.to(DEV), None if p.lo is None else p.lo.to(DEV)), p.float()


def _out(rt, name, shape):
    out = rt.hbuf(name, shape)
    out.hi.fill_(NAN)   # an element the kernel does not write fails the finite check
    return out


def _twice(launch, out):
    """Runs the launch twice: the output of the first as fp32 on the CPU, and the second must equal it bit for bit."""
    launch()
    first = (out.hi.clone(), None if out.lo is None else out.lo.clone())
    got = out.float().cpu()
    launch()
    assert torch.equal(out.hi.view(torch.int16), first[0].view(torch.int16))
    if out.lo is not None:
        assert torch.equal(out.lo.view(torch.int16), first[1].view(torch.int16))
    return got


# ------------------------------------------------------------------------------------------------------ vdn_flash_attn
def _flash(rt, case, nq, nk, mode, B, pv=None, qk8=False):
    from vdn.runtime import HL, ceil_to
    H, dh, scale = 2, 64, 0.125
    split = rt.split
    q, k, v = AC.make_batch(case, H, nq, nk, dh, scale, seed=nk + 7 * int(split))
    qp, kp = ceil_to(nq, 64), ceil_to(nk, 64)

    def padded(x, rows, fill):   # [H, n, 64] -> planes [H, rows, 64], pad rows `fill`
        P = HL.from_float(x, F16, split)
        hi = torch.full((H, rows, dh), fill, dtype=F16)
        hi[:, :x.shape[1]] = P.hi
        lo = None
        if split:
            lo = torch.full((H, rows, dh), fill, dtype=F16)
            lo[:, :x.shape[1]] = P.lo
        return HL(hi.to(DEV), None if lo is None else lo.to(DEV)), P

    qd, Q = padded(q, qp, 0.0)
    kd, K = padded(k, kp, NAN)   # pad keys must not matter: the ragged last tile is masked
    V = HL.from_float(v, F16, split)
    vt = torch.zeros(H, dh, kp, dtype=F16)
    vt[:, :, :nk] = V.hi.transpose(1, 2)
    vd = HL(vt.to(DEV))
    if split:
        vl = torch.zeros(H, dh, kp, dtype=F16)
        vl[:, :, :nk] = V.lo.transpose(1, 2)
        vd = HL(vt.to(DEV), vl.to(DEV))
    extra = (0.0, 0.0)
    q8 = k8 = None
    if qk8:
        def planes8(t):  # HL [H, pad, 64] -> u8 [H, pad, 128]: e5m2(value) | e5m2(remainder * 2^10), as the projection epilogue writes them
            return torch.cat([t.float().to(torch.float8_e5m2).view(torch.uint8),
                              (t.lo.float() * 1024.0).to(torch.float8_e5m2).view(torch.uint8)], dim=-1).contiguous()
        q8, k8 = planes8(qd), planes8(kd)
        extra = AC.qk8_movement(Q.hi.float(), Q.lo.float(), K.hi.float(), K.lo.float(), V.float(), scale)
    ref, e32, bar, bar_px = AC.bars(Q.float(), K.float(), V.float(), scale, B, 8, extra)
    out = _out(rt, "ar_flash", (nq, H * dh))
    if pv is not None:
        rt.pv_products = pv
    try:
        got = _twice(lambda: rt.flash_attn(qd, kd, vd, out, 1, H, nq, qp, nk, kp, scale, q8=q8, k8=k8), out)
    finally:
        rt.pv_products = PV_DEFAULT
    AC.check("flash_attn", case, f"{nq}x{nk}", mode, got, ref.transpose(0, 1).reshape(nq, H * dh), e32, bar, bar_px)


@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("nk", [64, 130, 321])
def test_flash_single_plane(rts, nk, case):
    _flash(rts[False], case, 130, nk, "fp16", 2e-3)


@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("nk,pv,B,qk8", [(321, 3, 1e-5, False), (321, 2, 3e-4, False), (321, 2, 3e-4, True), (321, 1, 4e-4, True),
                                         (64, 2, 3e-4, True)])
def test_flash_split(rts, nk, pv, B, qk8, case):
    """The four (pv, qk8) rows of test_x3_flash_attention; with the 8-bit planes the kernel is flash_attn2_kernel, whose 6 key
    tiles at nk = 321 are the first, even, odd and last instantiation of the generated stream, and 1 tile at nk = 64."""
    _flash(rts[True], case, 130, nk, f"split pv={pv}" + (" qk8" if qk8 else ""), B, pv, qk8)


# ------------------------------------------------------------------------------------------------------ packed qkv rows
class Rows:
    """Packed qkv [rows, 3C] (columns q | k | v, each [heads][dh]) of sequences x heads problems; `order` is the permutation
    that takes [nseq.., heads, L, dh] to the row-major [.., heads, dh] layout of the rows."""

    def __init__(self, lead, heads, order):
        self.lead, self.heads, self.order = tuple(lead), heads, order
        self.back = [order.index(i) for i in range(len(order))]

    def pack(self, x):       # [*lead, heads, L, dh] -> [rows, heads * dh]
        y = x.permute(*self.order)
        return y.reshape(-1, self.heads * x.shape[-1])

    def unpack(self, y, L):  # [rows, heads * dh] -> [*lead, heads, L, dh]
        dims = list(self.lead) + [self.heads, L, y.shape[-1] // self.heads]
        return y.reshape(*[dims[i] for i in self.order]).permute(*self.back)


def _problems(case, lead, heads, nq, nk, dh, scale, seed, tile=64):
    n = heads
    for d in lead:
        n *= d
    q, k, v = AC.make_batch(case, n, nq, nk, dh, scale, seed, tile)
    return tuple(t.reshape(*lead, heads, t.shape[1], dh) for t in (q, k, v))


def _self_attn(rt, kernel, case, rows, L, dh, scale, shape, B, ratio, launch, tile=64):
    """q, k and v of every (sequence, head) from the case, packed, rounded to the planes; reference on what the planes hold."""
    C = rows.heads * dh
    q, k, v = _problems(case, rows.lead, rows.heads, L, L, dh, scale, seed=L + dh, tile=tile)
    qkv, vals = _planes(torch.cat([rows.pack(t) for t in (q, k, v)], dim=1).contiguous(), rt.split)
    qv, kv, vv = (rows.unpack(vals[:, i * C:(i + 1) * C], L) for i in range(3))
    ref, e32, bar, bar_px = AC.bars(qv, kv, vv, scale, B, ratio)
    out = _out(rt, "ar_rows", (vals.shape[0], C))
    got = _twice(lambda: launch(qkv, out, vals.shape[0], C), out)
    AC.check(kernel, case, shape, "split" if rt.split else "fp16", got, rows.pack(ref), e32, bar, bar_px)


# ------------------------------------------------------------------------------------------------------ vdn_dn_attn
@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("dh,heads", [(12, 8), (96, 2)])
def test_dn_attn_spatial(rts, dh, heads, split, case):
    """2 sequences of L = 196 consecutive rows: four key tiles, the last ragged; a partial last query tile."""
    rt, L, nseq = rts[split], 196, 2
    rows = Rows((nseq,), heads, (0, 2, 1, 3))   # row = seq * L + t
    _self_attn(rt, "dn_attn", case, rows, L, dh, dh ** -0.5, f"spatial L={L} dh={dh}", 1e-5 if split else 2e-3, 10,
               lambda qkv, out, n, C: rt.dn_attn(qkv, out, n, C, heads, L=L, estride=1, n0=1, s0=0, n1=nseq, s1=L, scale=dh ** -0.5))


@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("dh,heads", [(12, 8), (96, 2)])
def test_dn_attn_temporal(rts, dh, heads, split, case):
    """5 interleaved sequences of L = 33 rows at stride hw = 5: one ragged key tile; the ramps gain their bits per 16 keys."""
    rt, L, hw = rts[split], 33, 5
    rows = Rows((hw,), heads, (2, 0, 1, 3))     # row = t * hw + pixel
    _self_attn(rt, "dn_attn", case, rows, L, dh, dh ** -0.5, f"temporal L={L} hw={hw} dh={dh}", 1e-5 if split else 2e-3, 10,
               lambda qkv, out, n, C: rt.dn_attn(qkv, out, n, C, heads, L=L, estride=hw, n0=hw, s0=1, n1=1, s1=L * hw, scale=dh ** -0.5),
               tile=16)


# ------------------------------------------------------------------------------------------------------ vdn_hiera_attn
@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("heads,W,Lkv,qs", [(2, 2, 64, 4), (1, 1, 196, 1)])
def test_hiera_attn(rts, heads, W, Lkv, qs, case):
    """Token t of window w of frame f is row f*W*Lkv + t*W + w, query j of it output row f*W*Lq + j*W + w. With a query stride
    the case's query is the max over its qs elements t = g*Lq + j: element g = j % qs holds it, the others something smaller."""
    rt, F, dh = rts[True], 2, 96
    scale, Lq, C = dh ** -0.5, Lkv // qs, heads * dh
    rows = Rows((F, W), heads, (0, 3, 1, 2, 4))
    q, k, v = _problems(case, (F, W), heads, Lq, Lkv, dh, scale, seed=Lkv + qs)
    g = torch.Generator().manual_seed(Lkv)
    qe = q[..., None, :, :] - torch.rand(F, W, heads, qs, Lq, dh, generator=g)   # [.., g, j, dh], all below the pooled value
    j = torch.arange(Lq)
    qe[:, :, :, j % qs, j] = q
    qkv, vals = _planes(torch.cat([rows.pack(t) for t in (qe.reshape(F, W, heads, Lkv, dh), k, v)], dim=1).contiguous(), True)
    qv, kv, vv = (rows.unpack(vals[:, i * C:(i + 1) * C], Lkv) for i in range(3))
    qv = qv.reshape(F, W, heads, qs, Lq, dh).max(dim=3).values
    assert torch.equal(qv, rows.unpack(_planes(rows.pack(q), True)[1], Lq))     # the pooled query is the case's, to the bit
    ref, e32, bar, bar_px = AC.bars(qv, kv, vv, scale, 1e-5, 10)
    out = _out(rt, "ar_hiera", (vals.shape[0] // qs, C))
    got = _twice(lambda: rt.hiera_attn(qkv, out, F, heads, W, Lkv, qs, scale), out)
    AC.check("hiera_attn", case, f"heads={heads} W={W} Lkv={Lkv} qs={qs}", "split", got, rows.pack(ref), e32, bar, bar_px)


# ------------------------------------------------------------------------------------------------------ vdn_temporal_attn
@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("T", [7, 33, 64])
@pytest.mark.parametrize("c", [64, 192])
def test_temporal_attn(rts, c, T, split, case):
    """qkv [T, D, 3c]: sequence (d, head) over the T frames, a single key tile (two 32-frame blocks from T = 33 on); the ramps
    gain their bits per 16 frames."""
    rt, D, heads = rts[split], 3, 8
    dh = c // heads
    rows = Rows((D,), heads, (2, 0, 1, 3))      # row = t * D + d
    _self_attn(rt, "temporal_attn", case, rows, T, dh, dh ** -0.5, f"T={T} D={D} c={c}", 1e-5 if split else 2e-3, 8,
               lambda qkv, out, n, C: rt.temporal_attn(qkv, out, 1, T, D, c, heads, dh ** -0.5), tile=16)


# ------------------------------------------------------------------------------------------------------ vdn_temporal_attn_last
def _last(rt, case, T, in_pe_k):
    HW, c, heads = 31, 64, 8
    dh = c // heads
    scale = dh ** -0.5
    # head h: HW queries (one per pixel, the newest frame's) over T keys; the keys are the case's for every pixel, the values
    # differ per pixel
    q, k, v = _problems(case, (), heads, HW, T, dh, scale, seed=T, tile=16)       # [heads, HW | T, dh]
    g = torch.Generator().manual_seed(700 + T)
    vpx = v[:, None] + 0.5 * torch.randn(heads, HW, T, dh, generator=g)           # [heads, HW, T, dh]
    ref, e32, bar, bar_px = AC.bars(q[:, :, None], k[:, None], vpx, scale, 5e-6, 8)
    entries = torch.randn(T, HW, 3, heads, dh, generator=g)                       # the q of the older frames is never read
    entries[T - 1, :, 0] = q.transpose(0, 1)
    entries[:, :, 1] = 0.0 if in_pe_k else k.permute(1, 0, 2)[:, None]
    entries[:, :, 2] = vpx.permute(2, 1, 0, 3)
    tabs = [torch.zeros(T, c) for _ in range(3)]
    if in_pe_k:
        tabs[1] = k.permute(1, 0, 2).reshape(T, c).contiguous()
    nslots = T + 5
    slots = torch.randperm(nslots, generator=g)[:T].tolist()                       # scattered ring slots, oldest first
    pool = torch.full((nslots, HW, 3 * c), NAN, device=DEV)                        # unused slots must not be read
    for t in range(T):
        pool[slots[t]] = entries[t].reshape(HW, 3 * c).to(DEV)
    tabs = [t.to(DEV) for t in tabs]
    out = _out(rt, "ar_last", (HW, c))
    got = _twice(lambda: rt.temporal_attn_last(pool, slots, tabs[0], tabs[1], tabs[2], out, HW, c, scale), out)
    AC.check("temporal_attn_last", case, f"T={T} HW={HW} c={c}", "keys in pe_k" if in_pe_k else "f32 cache", got,
             ref[:, :, 0].transpose(0, 1).reshape(HW, c), e32, bar, bar_px)


@pytest.mark.parametrize("case", AC.CASES)
@pytest.mark.parametrize("T", [9, 32])
def test_temporal_attn_last(rts, T, case):
    _last(rts[True], case, T, False)


@pytest.mark.parametrize("case", AC.CASES)
def test_temporal_attn_last_keys_in_position_table(rts, case):
    """The same scores with the cached keys zero and the pattern in the pe_k table (added on load)."""
    _last(rts[True], case, 9, True)
