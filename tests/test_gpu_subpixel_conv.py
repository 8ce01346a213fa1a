"""layer{1,2}_rn folded into the ConvTranspose in front of it, on the MI355X: vdn_gemm's sub-pixel mode against the fp64
evaluation of the reference formula and against the materialised launch pair on the same inputs, and DPTEngine.run with
the path on and off.

Rule for every comparison (the one tests/test_gpu_lowres_oc1.py uses): both paths are three-product chains and the new one
rounds one intermediate fewer (the k-times map is never split into planes), so its error against fp64 may be at most 2x
the materialised pair's (the factor absorbs sampling noise), and both stay under the project's 1e-3, in rel-L2 and on the
worst element. The border ring (rows and columns 0 and k h - 1 / k w - 1) is measured apart from the interior: a wrong
bias share of a neighbour outside the map shows there and nowhere else.

Figures of the run that accompanied the change are in profiles/subpixel_rn.md."""
import pytest
import torch

from common import rel_l2, synth_sd, worst_px
from subpix_ref import reference_nhwc, ring_mask

pytestmark = pytest.mark.gpu
TOL = 1e-3
LEVELS = {1: (256, 4), 2: (512, 2)}   # ViT-L: out_channels[level - 1], ConvTranspose kernel == stride; features 256
F_VITL = 256


def _params(Ci, k, F, seed):
    g = torch.Generator().manual_seed(seed)
    wt = (torch.randn(Ci, Ci, k, k, generator=g) / Ci ** 0.5).cuda()
    bt = torch.randn(Ci, generator=g).cuda()
    wr = (torch.randn(F, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).cuda()
    return wt, bt, wr


def _subpix(rt, p, packed, B, h, w, Ci, k, F, name):
    out = rt.hbuf(name, (B * k * h * k * w, F))
    out.hi.fill_(float("nan"))
    out.lo.fill_(float("nan"))
    from vdn import _abi as abi
    return rt.gemm(p, packed[0], B * h * w, k * k * F, 4 * Ci, store=abi.ST_CONVT, out=out,
                   conv=dict(B=B, H=h, W=w, C=Ci, OH=h, OW=w, stride=1, korder=1), convt=dict(k=k, cout=F, B=B, H=h, W=w),
                   subpix_bias=packed[1])


def _materialised(rt, p, wt, bt, wr, B, h, w, Ci, k, F):
    from vdn import _abi as abi, pack
    wT, wR = pack.conv_transpose(wt, bt, rt.prec), pack.conv3x3(wr, rt.prec)
    l = rt.hbuf("mat_l", (B * k * h * k * w, Ci))
    rt.gemm(p, wT[0], B * h * w, k * k * Ci, Ci, bias=wT[1], store=abi.ST_CONVT, out=l, convt=dict(k=k, cout=Ci, B=B, H=h, W=w))
    out = rt.hbuf("mat_rn", (B * k * h * k * w, F))
    return rt.gemm(l, wR, B * k * h * k * w, F, 9 * Ci, out=out, conv=dict(B=B, H=k * h, W=k * w, C=Ci, OH=k * h, OW=k * w, stride=1))


def _errs(got, ref, ring):
    """(rel-L2, worst element) on the interior and on the border ring; `ring` is None for maps that are all ring."""
    g, r = got.double(), ref
    if ring is None:
        return None, (rel_l2(g, r), worst_px(g, r))
    scale = float(r.abs().max())
    inner = (rel_l2(g[~ring], r[~ring]), float((g[~ring] - r[~ring]).abs().max()) / scale) if (~ring).any() else None
    return inner, (rel_l2(g[ring], r[ring]), float((g[ring] - r[ring]).abs().max()) / scale)


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("B,h,w", [(4, 37, 37), (1, 28, 37), (1, 5, 7), (2, 1, 9)])
def test_subpixel_gemm_against_fp64_and_materialised_pair(level, B, h, w):
    """ViT-L's two levels at the bench lane's map (4 x 37 x 37), a non-square one (28 x 37), maps smaller than one M tile
    (5 x 7 and a 1-pixel-high 2 x 1 x 9, which is all border ring), random p / Wt / bT / Wr. Ten repeats bit-identical.
    Measured (rel-L2 / worst element, interior; the ring is the same size or smaller): level 1 at 4 x 37 x 37 3.6e-7 / 7.7e-7
    against 1.0e-6 / 1.7e-6 materialised, level 2 6.5e-7 / 1.0e-6 against 1.4e-6 / 2.1e-6; the small maps alike."""
    from vdn import pack
    from vdn.runtime import Runtime
    Ci, k = LEVELS[level]
    F = F_VITL
    rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
    assert pack.subpixel_conv_ok(Ci, F, k, rt.prec)
    wt, bt, wr = _params(Ci, k, F, 100 * level + h + w)
    g = torch.Generator().manual_seed(B * 1000 + h * 10 + w)
    p = rt.to_half(torch.randn(B * h * w, Ci, generator=g).cuda())
    packed = pack.subpixel_conv(wt, bt, wr, rt.prec)
    ref = reference_nhwc(p.float().double().reshape(B, h, w, Ci), wt.double(), bt.double(), wr.double())
    new = _subpix(rt, p, packed, B, h, w, Ci, k, F, "new").float().reshape(B, k * h, k * w, F)
    assert torch.isfinite(new).all(), "an output element was never written"
    mat = _materialised(rt, p, wt, bt, wr, B, h, w, Ci, k, F).float().reshape(B, k * h, k * w, F)
    ring = ring_mask(B, k * h, k * w, device="cuda") if min(h, w) * k > 2 else None
    en, em = _errs(new, ref, ring), _errs(mat, ref, ring)
    for where, a, b in zip(("interior", "ring"), en, em):
        if a is None:
            continue
        print(f"level {level} B={B} {h}x{w} {where}: sub-pixel rel-L2 {a[0]:.3e} worst {a[1]:.3e}; materialised rel-L2 {b[0]:.3e} worst {b[1]:.3e}")
    for where, a, b in zip(("interior", "ring"), en, em):
        if a is None:
            continue
        for name, x, y in zip(("rel-L2", "worst element"), a, b):
            assert x < TOL and y < TOL, (where, name, x, y)
            assert x <= 2 * y, (where, name, x, y)
    first = rt.hbuf("new", (B * k * h * k * w, F))
    hi0, lo0 = first.hi.clone(), first.lo.clone()
    for _ in range(10):
        again = _subpix(rt, p, packed, B, h, w, Ci, k, F, "again")
        assert torch.equal(again.hi, hi0) and torch.equal(again.lo, lo0)


@pytest.mark.parametrize("Ci,F,k", [(48, 64, 4), (96, 128, 4), (96, 64, 2), (192, 128, 2), (1536, 384, 4), (1536, 384, 2), (256, 64, 4)])
def test_kernel_rejects_what_the_gate_excludes(Ci, F, k):
    """ViT-S / ViT-B / ViT-g widths (and a 64-channel-block input with a narrow output): the gate says no, and a launch that
    asks for the mode anyway is refused by vdn_gemm instead of computing something else."""
    from vdn import _abi as abi, pack
    from vdn.runtime import HL, Runtime
    rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
    assert not pack.subpixel_conv_ok(Ci, F, k, rt.prec)
    B, h, w = 1, 3, 4
    p = rt.to_half(torch.randn(B * h * w, Ci).cuda())
    W = HL(torch.zeros(k * k * F, 4 * Ci, dtype=torch.float16, device="cuda"), torch.zeros(k * k * F, 4 * Ci, dtype=torch.float16, device="cuda"))
    with pytest.raises(abi.VdnError):
        _subpix(rt, p, (W, torch.zeros(k * k, 4, F, device="cuda")), B, h, w, Ci, k, F, "rej")


def _head(enc):
    import vdn
    from vdn import modules
    cfg = vdn.MODEL_CONFIGS[enc]
    head = modules.dpt_head(modules.ENCODERS[enc]["dim"], cfg["features"], cfg["out_channels"], False, False)
    sd = {k[len("depth_head."):]: v for k, v in synth_sd("A", enc).items() if k.startswith("depth_head.")}
    head.load_state_dict(sd, strict=True)
    return head.to("cuda").eval(), modules.ENCODERS[enc]["dim"], cfg["features"], cfg["out_channels"]


@pytest.mark.parametrize("enc,Bf,ph,pw", [("vitl", 4, 37, 37), ("vits", 2, 28, 37), ("vitb", 1, 19, 26)])
def test_engine_with_and_without_the_switch(enc, Bf, ph, pw, monkeypatch):
    """DPTEngine.run on the same taps with the sub-pixel path and, with VDN_RN_HIRES, with the materialised 4x / 2x maps.
    l1_rn / l2_rn of each run against the fp64 formula on that run's own projected maps follow the rule above, the two depth
    maps agree within 1e-3, and the path under test must have run: on ViT-L l1 / l2 are absent from the arena, on the
    widths the gate excludes (ViT-S, ViT-B) the engine must have taken the materialised path without the switch.
    Measured on ViT-L: l1_rn 5.0e-7 / 9.1e-7 against 1.0e-6 / 1.6e-6, l2_rn 9.3e-7 / 1.3e-6 against 1.5e-6 / 2.0e-6 (rel-L2 /
    worst element, interior); depth against depth rel-L2 8.0e-7, worst pixel 1.4e-6."""
    from vdn.engine import DPTEngine
    from vdn.runtime import Runtime
    head, dim, F, oc = _head(enc)
    g = torch.Generator().manual_seed(13)
    taps_f = [torch.randn(Bf * ph * pw, dim, generator=g).cuda() for _ in range(4)]
    admitted = enc == "vitl"
    errs, depths = {}, {}
    for mode in ("subpix", "hires"):
        if mode == "hires":
            monkeypatch.setenv("VDN_RN_HIRES", "1")
        else:
            monkeypatch.delenv("VDN_RN_HIRES", raising=False)
        rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
        eng = DPTEngine(rt, head, dim, F, oc, temporal=False)
        took = mode == "subpix" and admitted
        assert [r is not None for r in eng.rn_low] == [took, took]
        depths[mode] = eng.run([rt.to_half(t) for t in taps_f], Bf, ph, pw).clone()
        names = {key[0] for key in rt._bufs}
        assert ("l1" in names) == (not took) and ("l2" in names) == (not took), "the path under test did not run"
        assert "l1_rn" in names and "l2_rn" in names
        errs[mode] = []
        for i, k in enumerate((4, 2)):
            pr = rt.hbuf(f"proj{i}", (Bf * ph * pw, oc[i])).float().double().reshape(Bf, ph, pw, oc[i])
            rl, rn = head.resize_layers[i], getattr(head.scratch, f"layer{i + 1}_rn")
            ref = reference_nhwc(pr, rl.weight.double(), rl.bias.double(), rn.weight.double())
            got = rt.hbuf(f"l{i + 1}_rn", (Bf * k * ph * k * pw, F)).float().reshape(Bf, k * ph, k * pw, F)
            inner, ring = _errs(got, ref, ring_mask(Bf, k * ph, k * pw, device="cuda"))
            errs[mode] += [*inner, *ring]
            print(f"[{enc} Bf={Bf} {ph}x{pw}] {mode} l{i + 1}_rn: interior rel-L2 {inner[0]:.3e} worst {inner[1]:.3e}; "
                  f"ring rel-L2 {ring[0]:.3e} worst {ring[1]:.3e}")
            del pr, ref, got
        del rt, eng
        torch.cuda.empty_cache()
    dd = (rel_l2(depths["subpix"], depths["hires"]), worst_px(depths["subpix"], depths["hires"]))
    print(f"[{enc}] depth, sub-pixel against materialised: rel-L2 {dd[0]:.3e} worst pixel {dd[1]:.3e}")
    for new, mat in zip(errs["subpix"], errs["hires"]):
        assert new < TOL and mat < TOL, (new, mat)
        assert new <= 2 * mat, (new, mat)
    assert dd[0] < TOL and dd[1] < TOL, dd
    if not admitted:
        assert torch.equal(depths["subpix"], depths["hires"])
