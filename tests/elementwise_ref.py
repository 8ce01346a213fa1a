"""Plain float64 restatements of the normalisation, elementwise and spatial kernels (csrc/norm.hip, csrc/spatial.hip), the
inputs of their edge tests and the one comparison those tests use; torch on the CPU, no kernels and no vdn import.

Every restatement takes the values the kernel sees (already rounded to the operand type) and evaluates the operation in
float64, so that what a test measures is the kernel's own arithmetic and the rounding of its output type:
  1e-5   a float32 output, 1e-3 an fp16 output (2^-11 per value), 1.5e-2 a bf16 output (2^-8 per value)
(the rules of tests/test_gpu_ops.py). Inputs are value = f(row, channel) + noise: a kernel that reads the wrong row or channel
past its first grid round returns values that are off by the step of f, far outside every bar, which noise alone would show
only as noise."""
import torch

from oc1_ref import upsample_nhwc

NOISE_ROWS = 4099   # prime: the noise block repeats with a period that no grid stride or row length divides


def close64(got, ref, tol, what=""):
    """rel-L2 < tol and worst element (relative to the largest reference value) < 8 tol, as `close` of test_gpu_ops.py, with
    the difference taken in float64 on the device `got` lives on. Returns (rel-L2, worst) for the tests that print them."""
    ref = ref.to(got.device)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    d = got.double() - ref.double()
    err = float(d.norm() / (ref.double().norm() + 1e-30))
    mx = float(d.abs().max() / (ref.double().abs().max() + 1e-30))
    assert err < tol and mx < 8 * tol, (what, err, mx, tol)
    return err, mx


def errors64(got, ref):
    """(rel-L2, worst element) of close64 without a bar."""
    d = got.double().cpu() - ref.double()
    return float(d.norm() / (ref.double().norm() + 1e-30)), float(d.abs().max() / (ref.double().abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------ inputs
def noise(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tagged(rows, C, seed=0, dtype=torch.float32, amp=0.5):
    """f32 [rows, C] holding values of `dtype`: 0.01 (row % 251) + 0.02 (c % 127) + amp * noise, the noise block repeating every
    NOISE_ROWS rows (a 2 M-row input costs one gather, not 100 M normal deviates)."""
    base = noise(min(rows, NOISE_ROWS), C, seed=seed, scale=amp)
    r = torch.arange(rows)
    x = base[r % NOISE_ROWS] if rows > NOISE_ROWS else base
    x = x + (0.01 * (r % 251).float())[:, None] + (0.02 * (torch.arange(C) % 127).float())[None, :]
    return x.to(dtype).float()


def gn_input(F, HW, C, k, seed=0):
    """GroupNorm input of mean / std ratio k as fp16 planes: x ~ N(k, 1) in f32, hi = fp16(x), lo = fp16(x - hi) (hi + lo holds
    x to 2^-22 and is exact in f32). Returns (hi, lo, value) with value = hi + lo in f32."""
    x = noise(F, HW, C, seed=seed) + float(k)
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi, lo, hi.float() + lo.float()


def cast_input(n, seed=0):
    """f32 [n] for the cast kernel: normal deviates over 40 binades, then every edge of the 16-bit targets: subnormals of fp16
    (and the tie at half its smallest), f32 subnormals (subnormal for bf16 too), the first values that round to inf in fp16 and
    in bf16, round-to-nearest-even ties of both, +-inf, +-0 and NaN; the edges are repeated through the array so that every
    grid round meets them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-30, 10, (n,), generator=g).float())
    edge = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), float("nan"), 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                         3 * 2.0 ** -24, 1e-7, -6e-8, 6.1e-5, 2.0 ** -14, 1e-40, -1e-40, 2.0 ** -133, 3 * 2.0 ** -134, 2.0 ** -149,
                         65504.0, 65519.9, 65520.0, -65520.0, 7e4, 1e5, 3.38e38, 3.3961775292304e38, 3.4e38, -3.4e38,
                         1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 - 2.0 ** -12])
    idx = torch.arange(0, n - len(edge), 50021)
    for j, e in enumerate(edge):
        x[idx + j] = e
    x[n - len(edge):] = edge
    return x


# ------------------------------------------------------------------------------------------------ normalisation
def layer_norm(x, w, b, eps, addvec=None, alpha=1.0, tab=None, tab_div=1, tab_mod=1, out_group=0):
    """vdn_layernorm: rows of x [rows, C] normalised (biased variance), * w + b + alpha * addvec + tab[(row // tab_div) % tab_mod];
    out_group > 0 drops the first row of every group of out_group rows (the cls token) and compacts the rest."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * w.double() + b.double()
    if addvec is not None:
        y = y + alpha * addvec.double()
    if tab is not None:
        y = y + tab.double()[(torch.arange(x.shape[0]) // tab_div) % tab_mod]
    if out_group > 0:
        y = y[torch.arange(x.shape[0]) % out_group != 0]
    return y


def group_norm(x, groups, w, b, eps):
    """vdn_groupnorm on x [F, HW, C]: statistics per (frame, group of C / groups adjacent channels) over HW and the group."""
    F, HW, C = x.shape
    g = x.double().reshape(F, HW, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    return ((g - mean) / torch.sqrt(var + eps)).reshape(F, HW, C) * w.double() + b.double()


# ------------------------------------------------------------------------------------------------ elementwise
def add_vec(x, vec, alpha):
    return x.double() + alpha * vec.double()


def addtab_cast(x, tab=None, tab_div=1, tab_mod=1):
    y = x.double()
    if tab is not None:
        y = y + tab.double()[(torch.arange(x.shape[0]) // tab_div) % tab_mod]
    return y


# ------------------------------------------------------------------------------------------------ spatial
def bilinear_ac(x, OH, OW):
    """align_corners bilinear resize of x [B, h, w, C] (or [B, h, w]): sample positions by the kernels' float32 expression
    (csrc/resample.hpp, "rounded" weights), the blend in float64."""
    if x.dim() == 3:
        return upsample_nhwc(x.double()[..., None], OH, OW)[..., 0]
    return upsample_nhwc(x.double(), OH, OW)


def patchify(img):
    """img [B, 3, H, W] -> [B * H/14 * W/14, 588]: the 14 x 14 patches as rows in (channel, ky, kx) order, the order of the
    patch-embedding convolution's weight."""
    B, Cc, H, W = img.shape
    ph, pw = H // 14, W // 14
    return img.reshape(B, Cc, ph, 14, pw, 14).permute(0, 2, 4, 1, 3, 5).reshape(B * ph * pw, Cc * 196)


def head_out(feat, w, bias, relu):
    y = feat.double() @ w.double() + bias
    return y.clamp(min=0) if relu else y


def dwconv7(x, w, b):
    """Depthwise 7 x 7, zero padding 3, on x [B, H, W, C]; w [49, C] (tap = 7 ky + kx), b [C]."""
    B, H, W, C = x.shape
    xp = torch.zeros(B, H + 6, W + 6, C, dtype=torch.float64)
    xp[:, 3:H + 3, 3:W + 3] = x.double()
    y = b.double().expand(B, H, W, C).clone()
    for ky in range(7):
        for kx in range(7):
            y += xp[:, ky:ky + H, kx:kx + W] * w[ky * 7 + kx].double()
    return y
