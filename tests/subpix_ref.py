"""fp64 restatements for the sub-pixel convolution tests (pack.subpixel_conv_compose, vdn_gemm's subpix mode): the reference
formula layer_rn(resize_layer(p)) and the block sum the kernel evaluates, both on NHWC maps."""
import torch
import torch.nn.functional as Fn


def reference(p, wt, bt, wr):
    """conv2d(conv_transpose2d(p, wt, bt, stride = k), wr, padding = 1) (dpt.py:129 then :135-136) on p [B, h, w, Ci]
    -> [B, k h, k w, Co]."""
    k = wt.shape[-1]
    y = Fn.conv2d(Fn.conv_transpose2d(p.permute(0, 3, 1, 2), wt, bt, stride=k), wr, padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def block_sum(p, wc, beta, slots, k):
    """Output pixel (k y + a, k x + b) = sum over the phase's neighbour slots (sy, sx) with (y + sy, x + sx) inside the map of
    wc[phase, slot] @ p[y + sy, x + sx] + beta[phase, slot]; a neighbour outside drops out whole, its bias share included."""
    B, h, w, _ = p.shape
    co = wc.shape[2]
    pp = Fn.pad(p, (0, 0, 1, 1, 1, 1))
    inside = Fn.pad(torch.ones(h, w, dtype=p.dtype, device=p.device), (1, 1, 1, 1))
    out = torch.zeros(B, h, k, w, k, co, dtype=p.dtype, device=p.device)
    for a in range(k):
        for b in range(k):
            ph = a * k + b
            for s, (sy, sx) in enumerate(slots[ph]):
                q = pp[:, 1 + sy:1 + sy + h, 1 + sx:1 + sx + w]
                m = inside[1 + sy:1 + sy + h, 1 + sx:1 + sx + w]
                out[:, :, a, :, b] += (q @ wc[ph, s].t() + beta[ph, s]) * m[None, :, :, None]
    return out.reshape(B, h * k, w * k, co)


def ring_mask(B, H, W, device=None):
    """True on the border ring (rows and columns 0 and H - 1 / W - 1) of [B, H, W] maps."""
    m = torch.zeros(B, H, W, dtype=torch.bool, device=device)
    m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True
    return m


def reference_nhwc(p, wt, bt, wr):
    """The same formula as shifted matrix products (any device; the GPU tests evaluate it in fp64 on the device): the
    transposed convolution with kernel == stride is one matrix product per phase, the 3x3 convolution nine shifted ones."""
    B, h, w, _ = p.shape
    cm, k = wt.shape[1], wt.shape[-1]
    up = torch.empty(B, h, k, w, k, cm, dtype=p.dtype, device=p.device)
    for a in range(k):
        for b in range(k):
            up[:, :, a, :, b] = p @ wt[:, :, a, b].to(p.dtype) + bt.to(p.dtype)
    up = Fn.pad(up.reshape(B, h * k, w * k, cm), (0, 0, 1, 1, 1, 1))
    out = torch.zeros(B, h * k, w * k, wr.shape[0], dtype=p.dtype, device=p.device)
    for ky in range(3):
        for kx in range(3):
            out += up[:, ky:ky + h * k, kx:kx + w * k] @ wr[:, :, ky, kx].to(p.dtype).t()
    return out
