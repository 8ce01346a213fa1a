"""layer{1,2}_rn folded into the ConvTranspose in front of it (DPTEngine.run, pack.subpixel_conv_compose, vdn_gemm's subpix
mode): the identity itself, in fp64 on the CPU. A 3x3 window on the k-times map reaches only the 3x3 neighbourhood of the
source pixel, each output phase through a short list of neighbours, and a neighbour outside the map stands for pixels in the
convolution's zero padding, so it drops out together with its share of the transposed convolution's bias."""
import pytest
import torch

from subpix_ref import block_sum, reference, reference_nhwc


@pytest.mark.parametrize("B,h,w", [(2, 5, 7), (1, 3, 9), (2, 1, 3), (1, 4, 1), (3, 1, 1), (1, 2, 1)])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("Ci,Cm,Co", [(8, 8, 8), (6, 10, 4)])
def test_block_sum_equals_conv_of_conv_transpose(B, h, w, k, Ci, Cm, Co):
    from vdn import pack
    g = torch.Generator().manual_seed(1000 * h + 10 * w + k + Ci)
    p = torch.randn(B, h, w, Ci, dtype=torch.float64, generator=g)
    wt, bt = torch.randn(Ci, Cm, k, k, dtype=torch.float64, generator=g), torch.randn(Cm, dtype=torch.float64, generator=g)
    wr = torch.randn(Co, Cm, 3, 3, dtype=torch.float64, generator=g)
    ref = reference(p, wt, bt, wr)
    wc, beta, slots = pack.subpixel_conv_compose(wt, bt, wr)
    assert wc.shape == (k * k, 4, Co, Ci) and beta.shape == (k * k, 4, Co) and wc.dtype == torch.float64
    got = block_sum(p, wc, beta, slots, k)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"B={B} {h}x{w} k={k} {Ci}->{Cm}->{Co}: max |block sum - reference| / max |reference| = {err:.2e}")
    assert err < 1e-10, err
    # the matrix-product restatement the GPU tests use says the same as torch's conv_transpose2d / conv2d
    assert float((reference_nhwc(p, wt, bt, wr) - ref).abs().max() / ref.abs().max()) < 1e-10
    # the bias share of a neighbour outside the map must drop out: keeping it is wrong on the border ring
    if h > 1 or w > 1:
        whole = beta.sum(1).reshape(k, k, Co)[None, None, :, None].expand(B, h, k, w, k, Co).reshape(B, h * k, w * k, Co)
        keep = block_sum(p, wc, torch.zeros_like(beta), slots, k) + whole
        assert float((keep - ref).abs().max() / ref.abs().max()) > 1e-3


@pytest.mark.parametrize("k", [2, 4])
def test_documented_row_and_neighbour_order(k):
    """phase = a*k + b; its slots list (sy, sx) with sy ascending, then sx ascending; {-1, 0} for phase 0, {0, 1} for phase
    k - 1, {0} in between: 16 blocks for k = 2, 36 for k = 4. Block (phase, slot) is the sum over the taps that land in that
    neighbour of Wr[dy, dx] Wt[(a + dy) mod k, (b + dx) mod k]^T, its bias share the same taps' Wr[dy, dx] bT; unused slots are 0."""
    from vdn import pack
    g = torch.Generator().manual_seed(5 + k)
    Ci, Cm, Co = 8, 6, 4
    wt, bt, wr = torch.randn(Ci, Cm, k, k, generator=g), torch.randn(Cm, generator=g), torch.randn(Co, Cm, 3, 3, generator=g)
    wc, beta, slots = pack.subpixel_conv_compose(wt, bt, wr)
    assert [pack.subpixel_neighbours(k, a) for a in range(k)] == ([(-1, 0), (0, 1)] if k == 2 else [(-1, 0), (0,), (0,), (0, 1)])
    assert sum(len(s) for s in slots) == (16 if k == 2 else 36)
    for a in range(k):
        for b in range(k):
            ph = a * k + b
            want = [(sy, sx) for sy in pack.subpixel_neighbours(k, a) for sx in pack.subpixel_neighbours(k, b)]
            assert slots[ph] == want == sorted(want)
            for s, (sy, sx) in enumerate(want):
                blk, bs = torch.zeros(Co, Ci, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if (a + dy) // k == sy and (b + dx) // k == sx:
                            blk += wr[:, :, dy + 1, dx + 1].double() @ wt[:, :, (a + dy) % k, (b + dx) % k].double().t()
                            bs += wr[:, :, dy + 1, dx + 1].double() @ bt.double()
                assert torch.allclose(wc[ph, s], blk, rtol=1e-12, atol=1e-12) and torch.allclose(beta[ph, s], bs, rtol=1e-12, atol=1e-12)
            assert not wc[ph, len(want):].any() and not beta[ph, len(want):].any()


def test_gate_admits_vitl_widths_only():
    """An N tile of the kernel (256 columns) must lie inside one phase and K runs in 64-channel blocks: ViT-L's head
    (features 256, out_channels 256 / 512) qualifies, the ViT-S / ViT-B / ViT-g heads keep the two-launch path."""
    from vdn import MODEL_CONFIGS, pack
    split = pack.Prec(torch.float16, True)
    for enc, cfg in MODEL_CONFIGS.items():
        for i, k in enumerate((4, 2)):
            assert pack.subpixel_conv_ok(cfg["out_channels"][i], cfg["features"], k, split) == (enc == "vitl"), (enc, i)
    assert not pack.subpixel_conv_ok(256, 256, 4, pack.Prec(torch.float16, False))  # one-product mode has no such kernel
