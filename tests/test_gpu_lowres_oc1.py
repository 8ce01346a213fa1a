"""output_conv1 at the low resolution on the MI355X: the combine kernel alone against its torch restatement, and
DPTEngine.run with the path on and off against the fp64 evaluation of the reference formula on the same input.

Figures of the run that accompanied the change are in profiles/lowres_oc1.md."""
import pytest
import torch
import torch.nn.functional as Fn

from common import rel_l2, synth_sd, worst_px
from oc1_ref import combine_ref, conv3x3_nhwc, oc1_reference

pytestmark = pytest.mark.gpu
TOL = 1e-3


@pytest.mark.parametrize("B,h,w,Co", [(2, 19, 26, 32), (1, 37, 28, 128), (1, 9, 5, 16), (3, 17, 33, 64), (1, 1, 8, 16), (1, 40, 3, 48)])
def test_combine_kernel_against_restatement(B, h, w, Co):
    """vdn_oc1_combine on random tap images (non-square maps, tiles cut by both borders, several channel counts) against the
    same sum in fp64 with the kernel's float32 sample positions. Bound from the number format: an output value is a bias
    plus at most 9 taps x 4 corners products, well under 64 fp32 roundings (2^-24 each) of partial sums that never exceed
    9 max|z| + max|b1|. Repeats must agree bit for bit (no atomics)."""
    from vdn.runtime import Runtime
    rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
    g = torch.Generator().manual_seed(B * 1000 + h * 10 + w)
    z = torch.randn(B * h * w, 9 * Co, generator=g).cuda()
    b1 = torch.randn(Co, generator=g).cuda()
    OH, OW = 2 * h, 2 * w
    out = torch.full((B * OH * OW, Co), float("nan"), device="cuda")
    rt.oc1_combine(z, b1, out, B, h, w, OH, OW, Co)
    ref = combine_ref(z.double().reshape(B, h, w, 9, Co), b1.double(), OH, OW, coord=torch.float32).reshape(B * OH * OW, Co)
    assert torch.isfinite(out).all()
    err = float((out.double() - ref).abs().max())
    bound = 64 * 2.0 ** -24 * (9 * float(z.abs().max()) + float(b1.abs().max()))
    print(f"combine B={B} {h}x{w} Co={Co}: max abs error {err:.2e} (bound {bound:.2e}), rel-L2 {rel_l2(out, ref):.2e}")
    assert err <= bound, (err, bound)
    again = torch.empty_like(out)
    rt.oc1_combine(z, b1, again, B, h, w, OH, OW, Co)
    assert torch.equal(out, again)


def _head(enc):
    import vdn
    from vdn import modules
    cfg = vdn.MODEL_CONFIGS[enc]
    head = modules.dpt_head(modules.ENCODERS[enc]["dim"], cfg["features"], cfg["out_channels"], False, False)
    sd = {k[len("depth_head."):]: v for k, v in synth_sd("A", enc).items() if k.startswith("depth_head.")}
    head.load_state_dict(sd, strict=True)
    return head.to("cuda").eval(), modules.ENCODERS[enc]["dim"], cfg["features"], cfg["out_channels"]


def _tail_fp64(o1, s, H, W):
    """dpt.py:146-151 from output_conv1's result on: resize to (H, W), conv3x3 + ReLU, conv1x1 + ReLU."""
    up = Fn.interpolate(o1.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    c2, c3 = s.output_conv2[0], s.output_conv2[2]
    t = torch.relu(conv3x3_nhwc(up, c2.weight.double(), c2.bias.double()))
    return torch.relu(t @ c3.weight.double().reshape(1, -1).t() + c3.bias.double())[..., 0]


@pytest.mark.parametrize("enc,Bf,ph,pw", [("vitl", 4, 37, 37), ("vits", 2, 28, 37)])
def test_engine_lowres_against_fp64_and_materialised(enc, Bf, ph, pw, monkeypatch):
    """The bench lane's head shape (ViT-L, 4 frames of 518 x 518) and a non-square ViT-S 392 x 518: out1_f32 and the depth of
    DPTEngine.run on the low-resolution path and, with VDN_OC1_HIRES, on the materialised path1, each against the fp64
    evaluation of the reference formula on the u (refinenet1.resConfUnit2 output) of its own run. Both are three-product
    chains and the new one rounds one intermediate fewer, so its error may be at most 2x the materialised path's (the
    factor absorbs sampling noise), and both stay under the project's 1e-3.
    Measured (rel-L2 / worst pixel): ViT-L out1 1.0e-6 / 1.2e-6 against 3.1e-6 / 6.8e-6 materialised, depth 8.7e-7 / 1.3e-6
    against 2.1e-6 / 7.3e-6; ViT-S out1 7.8e-7 / 1.0e-6 against 2.6e-6 / 6.1e-6, depth 8.2e-7 / 1.9e-6 against 1.9e-6 / 4.9e-6."""
    from vdn.engine import DPTEngine
    from vdn.runtime import Runtime
    head, dim, F, oc = _head(enc)
    s = head.scratch
    g = torch.Generator().manual_seed(11)
    taps_f = [torch.randn(Bf * ph * pw, dim, generator=g).cuda() for _ in range(4)]
    h, w, OH, OW, H, W = 4 * ph, 4 * pw, 8 * ph, 8 * pw, 14 * ph, 14 * pw
    errs = {}
    for mode in ("lowres", "hires"):
        if mode == "hires":
            monkeypatch.setenv("VDN_OC1_HIRES", "1")
        else:
            monkeypatch.delenv("VDN_OC1_HIRES", raising=False)
        rt = Runtime(torch.device("cuda:0"), torch.float16, split=True)
        eng = DPTEngine(rt, head, dim, F, oc, temporal=False)
        assert (eng.oc1_low is not None) == (mode == "lowres") and eng.oc2_taps is not None
        depth = eng.run([rt.to_half(t) for t in taps_f], Bf, ph, pw).clone()
        took_lowres = ("oc1_z", (Bf * h * w, 9 * (F // 2)), torch.float32) in rt._bufs
        assert took_lowres == (mode == "lowres"), "the path under test did not run"
        assert (("path1", (Bf * OH * OW, F), torch.float16) in rt._bufs) == (mode == "hires")
        u = rt.hbuf("ff1_u", (Bf * h * w, F)).float().double().reshape(Bf, h, w, F)
        o1 = rt.fbuf("out1_f32", (Bf * OH * OW, F // 2)).reshape(Bf, OH, OW, F // 2)
        f1 = s.refinenet1.out_conv
        ref1 = oc1_reference(u, f1.weight.double(), f1.bias.double(), s.output_conv1.weight.double(), s.output_conv1.bias.double(), OH, OW)
        refd = _tail_fp64(ref1, s, H, W)
        errs[mode] = (rel_l2(o1, ref1), worst_px(o1, ref1), rel_l2(depth, refd), worst_px(depth, refd))
        print(f"[{enc} Bf={Bf} {14 * ph}x{14 * pw}] {mode}: out1_f32 rel-L2 {errs[mode][0]:.3e} worst pixel {errs[mode][1]:.3e}; "
              f"depth rel-L2 {errs[mode][2]:.3e} worst pixel {errs[mode][3]:.3e}")
        del rt, eng, u, o1, ref1, refd
        torch.cuda.empty_cache()
    for name, lo, hi in zip(("out1 rel-L2", "out1 worst pixel", "depth rel-L2", "depth worst pixel"), errs["lowres"], errs["hires"]):
        assert lo < TOL and hi < TOL, (name, lo, hi)
        assert lo <= 2 * hi, (name, lo, hi)
