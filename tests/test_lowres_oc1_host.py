"""output_conv1 in front of refinenet1's 2x resize (DPTEngine.run, pack.lowres_oc1_compose, vdn_oc1_combine): the identity
itself, in fp64 on the CPU. conv3x3(pad 1) o bilinear x2 (align_corners) o conv1x1 has no non-linearity inside, a channel
mixing commutes with every spatial operator, and the interpolation weights sum to one, so the nine taps' mixing can run at
the low resolution and what is left is an interpolate-and-add pass. Both sides are fp64: agreement to rounding."""
import pytest
import torch
import torch.nn.functional as Fn

from oc1_ref import combine_ref, oc1_reference, upsample_nhwc


@pytest.mark.parametrize("h,w", [(5, 7), (3, 9), (1, 3), (7, 2), (11, 17)])
@pytest.mark.parametrize("F", [8, 16])
def test_composite_weight_and_combine_equal_the_reference_formula(h, w, F):
    from vdn import pack
    g = torch.Generator().manual_seed(100 * h + w + F)
    Co = F // 2
    u = torch.randn(2, F, h, w, dtype=torch.float64, generator=g)
    wo, bo = torch.randn(F, F, 1, 1, dtype=torch.float64, generator=g), torch.randn(F, dtype=torch.float64, generator=g)
    W, b1 = torch.randn(Co, F, 3, 3, dtype=torch.float64, generator=g), torch.randn(Co, dtype=torch.float64, generator=g)
    OH, OW = 2 * h, 2 * w
    ref = Fn.conv2d(Fn.interpolate(Fn.conv2d(u, wo, bo), size=(OH, OW), mode="bilinear", align_corners=True), W, b1, padding=1)
    wc, bc = pack.lowres_oc1_compose(W, wo, bo)
    assert wc.shape == (9 * Co, F) and bc.shape == (9 * Co,) and wc.dtype == torch.float64
    rows = u.permute(0, 2, 3, 1).reshape(-1, F)                       # NHWC rows, as the engine holds them
    z = (rows @ wc.t() + bc).reshape(2, h, w, 9, Co)                   # the one low-resolution GEMM
    got = combine_ref(z, b1, OH, OW, coord=torch.float64).permute(0, 3, 1, 2)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"{h}x{w} F={F}: max |lowres - reference| / max |reference| = {err:.2e} (values up to {float(ref.abs().max()):.1f})")
    assert err < 1e-10, err
    # the NHWC restatement the GPU tests use says the same as torch's conv2d / interpolate
    ref2 = oc1_reference(u.permute(0, 2, 3, 1), wo, bo, W, b1, OH, OW).permute(0, 3, 1, 2)
    assert float((ref2 - ref).abs().max() / ref.abs().max()) < 1e-10


def test_composite_rows_are_tap_major():
    """Row t*Co + c of the composite weight is (W_t Wo)[c] with t = 3 ky + kx, its bias W_t bo."""
    from vdn import pack
    g = torch.Generator().manual_seed(7)
    F, Co = 8, 4
    W, wo, bo = torch.randn(Co, F, 3, 3, generator=g), torch.randn(F, F, generator=g), torch.randn(F, generator=g)
    wc, bc = pack.lowres_oc1_compose(W, wo, bo)
    for ky in range(3):
        for kx in range(3):
            t = 3 * ky + kx
            assert torch.allclose(wc[t * Co:(t + 1) * Co], W[:, :, ky, kx].double() @ wo.double(), rtol=1e-12, atol=1e-12)
            assert torch.allclose(bc[t * Co:(t + 1) * Co], W[:, :, ky, kx].double() @ bo.double(), rtol=1e-12, atol=1e-12)


def test_float32_sample_positions_match_torch():
    """upsample_nhwc with float32 coordinates (the kernels' expression) against torch's float32 interpolate."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 9, 7, generator=g)
    got = upsample_nhwc(x.permute(0, 2, 3, 1), 10, 18).permute(0, 3, 1, 2)
    ref = Fn.interpolate(x, size=(10, 18), mode="bilinear", align_corners=True)
    assert float((got - ref).abs().max()) < 1e-5
