"""Plain torch restatements for the low-resolution output_conv1 tests (no kernels): the reference formula
conv3x3(bilinear x2(conv1x1(u))) evaluated in the tensors' own precision, and the combine pass of vdn_oc1_combine
(include/vdn.h) on the nine tap images."""
import torch
import torch.nn.functional as Fn


def ac_coords(O, I, dtype, device="cpu", weight="rounded"):
    """align_corners=True source index of every destination index: scale = (I-1)/(O-1), src = scale * dst, evaluated in
    `dtype` (float32 = the expression of the kernels, float64 = torch's for fp64 tensors). `weight` is the flavour of
    csrc/resample.hpp's ac_coord: "rounded" = fl(fl(scale * dst) - i0), "fused" (float32 only) = fl(scale * dst - i0) with one
    rounding, emulated exactly: the product of two float32 fits a float64, and so does its distance to the integer below."""
    scale = (torch.tensor(I - 1, dtype=dtype) / torch.tensor(O - 1, dtype=dtype)) if O > 1 else torch.tensor(0, dtype=dtype)
    src = scale.to(device) * torch.arange(O, dtype=dtype, device=device)
    i0 = src.to(torch.int64).clamp(max=I - 1)
    i1 = (i0 + 1).clamp(max=I - 1)
    if weight == "fused":
        assert dtype == torch.float32
        exact = scale.double().to(device) * torch.arange(O, dtype=torch.float64, device=device) - i0.double()
        return i0, i1, exact.float()
    assert weight == "rounded", weight
    return i0, i1, src - i0.to(dtype)


def upsample_nhwc(x, OH, OW, coord=torch.float32, weight="rounded"):
    """Bilinear align_corners resize of x [B, h, w, C] with the sample positions computed in `coord` (weights of flavour
    `weight`), arithmetic in x.dtype."""
    _, h, w, _ = x.shape
    y0, y1, ly = ac_coords(OH, h, coord, x.device, weight)
    x0, x1, lx = ac_coords(OW, w, coord, x.device, weight)
    ly, lx = ly.to(x.dtype)[None, :, None, None], lx.to(x.dtype)[None, None, :, None]
    r0, r1 = x[:, y0], x[:, y1]
    top = (1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]
    bot = (1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1]
    return (1 - ly) * top + ly * bot


def combine_ref(z, b1, OH, OW, coord=torch.float32):
    """z [B, h, w, 9, Co] (tap images, tap = 3 ky + kx), b1 [Co] -> [B, OH, OW, Co]: every tap image sampled at the tap's
    position, taps in the zero padding dropped."""
    B, h, w, _, Co = z.shape
    out = b1.to(z.dtype).expand(B, OH, OW, Co).clone()
    for ky in range(3):
        for kx in range(3):
            up = upsample_nhwc(z[:, :, :, 3 * ky + kx], OH, OW, coord)
            ya, yb = max(0, 1 - ky), OH - max(0, ky - 1)   # destination rows y with y + ky - 1 inside the map
            xa, xb = max(0, 1 - kx), OW - max(0, kx - 1)
            out[:, ya:yb, xa:xb] += up[:, ya + ky - 1:yb + ky - 1, xa + kx - 1:xb + kx - 1]
    return out


def conv3x3_nhwc(x, w, b):
    """nn.Conv2d(3x3, pad 1) on x [B, H, W, Ci] with w [Co, Ci, 3, 3] as shifted matrix products (any dtype, any device)."""
    B, H, W, _ = x.shape
    xp = Fn.pad(x, (0, 0, 1, 1, 1, 1))
    out = b.to(x.dtype).expand(B, H, W, w.shape[0]).clone()
    for ky in range(3):
        for kx in range(3):
            out += xp[:, ky:ky + H, kx:kx + W] @ w[:, :, ky, kx].to(x.dtype).t()
    return out


def oc1_reference(u, wo, bo, w, b1, OH, OW):
    """The reference formula on u [B, h, w, F] in u.dtype (fp64 in the tests): out_conv (1x1), bilinear resize with
    align_corners=True (torch's own), output_conv1 (3x3, pad 1). Returns [B, OH, OW, Co]."""
    v = u @ wo.reshape(wo.shape[0], -1).to(u.dtype).t() + bo.to(u.dtype)
    up = Fn.interpolate(v.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return conv3x3_nhwc(up, w, b1)
