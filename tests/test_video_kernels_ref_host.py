"""tests/video_kernels_ref.py against what it restates, at small sizes on the CPU: the references that
tests/test_gpu_video_kernel_edges.py compares the kernels with must themselves be right."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import hiera_ref as HR
import video_kernels_ref as V

NAN, INF, NEG_NAN, FMAX, SUB, MEDIAN_ROWS = V.NAN, V.INF, V.NEG_NAN, V.FMAX, V.SUB, V.MEDIAN_ROWS


def _same(a, b):
    """bit for bit, but any NaN equals any NaN and -0 equals +0 (torch.equal's zeros)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------------------------------------ median
@pytest.mark.parametrize("row", MEDIAN_ROWS, ids=[str(i) for i in range(len(MEDIAN_ROWS))])
def test_median_is_torch_quantile_on_special_values(row):
    x = np.array([row], dtype=np.float32)
    want = torch.quantile(torch.from_numpy(x), 0.5, dim=-1).numpy()
    got = V.frame_median(x)
    assert _same(got, want), (row, got, want)
    if np.isnan(x).any():
        assert np.isnan(got).all()


def test_median_without_the_nan_rule_ignores_a_nan():
    """What the select alone makes of a NaN (select.hpp orders keys by bit pattern): the figures of the issue that
    asked for the rule. frame_median differs from select_lerp on exactly these frames."""
    pos = np.array([[1, 2, NAN, 4, 5]], dtype=np.float32)
    neg = np.array([[1, 2, NEG_NAN, 4, 5]], dtype=np.float32)
    assert V.select_lerp(pos)[0] == 4.0 and V.select_lerp(neg)[0] == 2.0
    assert np.isnan(V.frame_median(pos)[0]) and np.isnan(V.frame_median(neg)[0])
    for x in (pos, neg):
        assert bool(torch.isnan(torch.quantile(torch.from_numpy(x), 0.5, dim=-1)[0]))


@pytest.mark.parametrize("F_,n", [(1, 1), (3, 2), (4, 33), (4, 34), (2, 1001), (3, 4096)])
def test_median_is_torch_quantile_on_random_frames(F_, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(F_, n, generator=g) * 3.0
    x[0, : n // 3] = x[0, 0]
    if F_ > 1:
        x[1] = torch.round(x[1])
    assert _same(V.frame_median(x.numpy()), torch.quantile(x, 0.5, dim=-1).numpy())


def test_keys_are_ordered_and_invertible():
    v = np.array([-INF, -FMAX, -1.0, -SUB, -0.0, 0.0, SUB, 1.0, 1.75, 2.0, FMAX, INF], dtype=np.float32)
    k = V.ordered_keys(v)
    assert np.all(k[1:] > k[:-1])
    assert np.array_equal(V.key_values(k).view(np.uint32), v.view(np.uint32))
    assert V.ordered_keys(np.array([NAN], dtype=np.float32))[0] > k[-1] and V.ordered_keys(np.array([NEG_NAN]))[0] < k[0]
    # pass 0 of a positive float: 1024 + 4 * exponent + the top two mantissa bits
    assert V.pass_bins(1.75)[0] == 1024 + 4 * 127 + 3 and V.pass_bins(2.0)[0] == 1024 + 4 * 128
    assert V.pass_bins(1.0 + 2.0 ** -23) == (1024 + 4 * 127, 0, 1)


# ------------------------------------------------------------------------------------------------ stitch
def test_stitch_fit_and_apply_compose_to_util_stitch():
    """Two windows through the restated fit and apply equal vdn.util.stitch within the bar the device stitcher is held to
    against it (2e-6 rel-L2, test_gpu_ops.py), and the fit alone equals util's float32 closed form to float32 sums' accuracy."""
    from vdn import util
    fh, fw, T = 20, 24, util.INFER_LEN
    g = torch.Generator().manual_seed(401)
    wins = [(torch.randn(T, fh, fw, generator=g).abs() * (1.0 + 0.3 * k) + 0.1 * k).numpy() for k in range(2)]
    n = T + 22 - 5
    ref = util.stitch([w[i] for w in wins for i in range(T)], n)
    align, overlap = util.OVERLAP - util.INTERP_LEN, util.OVERLAP
    kf = [wins[0][k] for k in util.KEYFRAMES[:align]]
    scale, shift, det, s0, s2 = V.stitch_fit(wins[1][:align], np.stack(kf))
    us, ush = util.compute_scale_and_shift(np.concatenate(list(wins[1][:align])), np.concatenate(kf), np.ones((align * fh, fw)))
    assert det > 0 and abs(us - scale) <= 1e-4 * abs(scale) and abs(ush - shift) <= 1e-4 * max(abs(shift), abs(scale))
    out = wins[0].copy()
    tail, new, ref1 = V.stitch_apply(wins[1].reshape(T, -1), np.float32(scale), np.float32(shift), out[-util.INTERP_LEN:].reshape(util.INTERP_LEN, -1),
                                     align, overlap, util.KEYFRAMES[1])
    out[-util.INTERP_LEN:] = tail.reshape(-1, fh, fw)
    got = np.concatenate([out, new.reshape(-1, fh, fw)])[:n]
    assert got.shape == ref.shape
    err = np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref)
    assert err < 2e-6, err
    assert np.array_equal(ref1, np.maximum(wins[1][util.KEYFRAMES[1]].reshape(-1) * np.float32(scale) + np.float32(shift), 0))


def test_stitch_fit_singular_and_exact():
    assert V.stitch_fit(np.full(8, 3.0), np.full(8, 3.0))[:2] == (1.0, 0.0)
    p = np.array([1.0, 2.0, 3.0, 5.0], dtype=np.float32)
    s, b = V.stitch_fit(p, 2.0 * p + 0.5)[:2]
    assert abs(s - 2.0) < 1e-14 and abs(b - 0.5) < 1e-14


def test_stitch_apply_weights_and_clamp():
    win = np.arange(5 * 3, dtype=np.float32).reshape(5, 3) - 4.0
    tail, new, ref1 = V.stitch_apply(win, 2.0, -3.0, np.full((2, 3), 10.0, dtype=np.float32), 1, 3, 4)   # interp 2: weights 0, 1
    fit = np.maximum(win * 2.0 - 3.0, 0)
    assert np.array_equal(tail[0], np.full(3, 10.0)) and np.array_equal(tail[1], fit[2])
    assert np.array_equal(new, fit[3:]) and np.array_equal(ref1, fit[4]) and (fit == 0).any()


# ------------------------------------------------------------------------------------------------ refiner
@pytest.mark.parametrize("H,W", [(2, 2), (2, 7), (7, 2), (19, 23)])
def test_sobel_pack_is_the_oracles_normals(H, W):
    from oracle import ref_cpu as O
    d = torch.rand(3, H, W, generator=torch.Generator().manual_seed(H * W)) * 2.0
    want = torch.cat([d[:, None], O.sobel_normals(d[:, None])[:, :2]], dim=1).double().numpy()
    got = V.sobel_pack(d.numpy())
    assert got.shape == want.shape
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 2e-6 and np.abs(got - want).max() < 2e-6


def test_refine_scale_and_finish_are_the_torch_statement():
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(2, 35, generator=g) * 60000.0 + 100.0).double()
    med = torch.quantile(x, 0.5, dim=-1)
    out, s = V.refine_scale(x.numpy(), med.numpy(), 0.7, -0.2, 1.0, 65535.0)
    s_ref = torch.exp(torch.tanh(med / 65535.0 * 0.7 - 0.2))
    assert np.allclose(s, s_ref.numpy(), rtol=1e-14) and np.allclose(out, (x / 65535.0 * s_ref[:, None]).numpy(), rtol=1e-14)
    d = torch.rand(2, 35, generator=g).double()
    assert np.allclose(V.refine_finish(out, d.numpy(), 1.3, 0.05, 65535.0, True), ((torch.from_numpy(out) + (d * 1.3 + 0.05)) * 65535.0).numpy(), rtol=1e-14)
    assert np.array_equal(V.refine_finish(None, d.numpy(), 1.3, 0.05, 65535.0, False), (d * 65535.0).numpy())


# ------------------------------------------------------------------------------------------------ Hiera
@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_unrolled_index_is_hiera_refs(n):
    side = 7 << n
    perm = HR.unroll_index(n).numpy()                       # unrolled u -> row-major token
    yy, xx = np.divmod(perm, side)
    assert np.array_equal(V.unrolled_of_yx(yy, xx, n), np.arange(side * side))


def test_embed_rows_are_unfold_in_unrolled_order():
    img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(2))
    want = Fn.unfold(img, 7, padding=3, stride=4).transpose(1, 2)[:, HR.unroll_index(3)].reshape(2 * 3136, 147)
    assert np.array_equal(V.hiera_embed_rows(img.numpy()), want.numpy())


@pytest.mark.parametrize("stage", [0, 1, 2, 3])
def test_reroll_is_hiera_refs(stage):
    side = 56 >> stage
    x = torch.randn(2, side * side, 4, generator=torch.Generator().manual_seed(stage))
    assert np.array_equal(V.hiera_reroll(x.numpy(), stage), HR.reroll(x, stage).numpy())


def test_pool_is_torch_max_except_for_nan():
    x = torch.randn(2, 4 * 5, 8, generator=torch.Generator().manual_seed(3))
    assert np.array_equal(V.hiera_pool(x.numpy(), 5), x.reshape(2, 4, 5, 8).max(1).values.numpy())
    x[1, 2 * 5 + 3, 6] = NAN                                 # group 2 of token 3
    got, tmax = V.hiera_pool(x.numpy(), 5), x.reshape(2, 4, 5, 8).max(1).values.numpy()
    assert np.isnan(tmax[1, 3, 6]) and got[1, 3, 6] == np.nanmax(x.reshape(2, 4, 5, 8)[1, :, 3, 6].numpy())
    tmax[1, 3, 6] = got[1, 3, 6]
    assert np.array_equal(got, tmax)
    x[1, :, 6] = NAN                                         # all four groups: nothing left but the NaN
    assert np.isnan(V.hiera_pool(x.numpy(), 5)[1, :, 6]).all()


# ------------------------------------------------------------------------------------------------ head
def test_prologue_is_the_view_add_ape_composition():
    B, S, h, w, C = 2, 3, 3, 5, 8
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(B * S, h, w, C, generator=g), torch.randn(B * S, h, w, C, generator=g)
    ape = torch.randn(8, C, generator=g)
    ref = ((a + b).view(B, S, C, h, w) + ape[:S][None, :, :, None, None]).permute(0, 1, 3, 4, 2).reshape(-1, C)
    assert torch.equal(V.dn_prologue(a, b, B * S, C, h * w, ape, S), ref)
    assert torch.equal(V.dn_prologue(a, None, B * S, C, h * w), a.view(B, S, C, h, w).permute(0, 1, 3, 4, 2).reshape(-1, C))


@pytest.mark.parametrize("IH,IW,OH,OW", [(6, 7, 6, 7), (6, 7, 11, 13), (1, 5, 3, 9), (5, 1, 4, 1), (4, 5, 1, 1), (5, 6, 5, 9), (7, 6, 3, 4)])
def test_tail_is_conv_and_interpolate(IH, IW, OH, OW):
    g = torch.Generator().manual_seed(IH * 100 + OW)
    x = torch.randn(2, IH, IW, 5, generator=g).double()
    w, bias = torch.randn(3, 5, 3, 3, generator=g).double(), torch.randn(3, generator=g).double()
    din = torch.randn(2, OH, OW, generator=g).double()
    y = Fn.conv2d(x.permute(0, 3, 1, 2), w, bias, padding=1)
    if (OH, OW) != (IH, IW):
        y = Fn.interpolate(y, size=(OH, OW), mode="bilinear", align_corners=True)
    raw, d, nrm = V.dn_tail(x.numpy(), w.numpy(), bias.numpy(), OH, OW, din.numpy(), True)
    assert np.allclose(raw, y.numpy(), rtol=0, atol=1e-12)
    assert np.allclose(d, torch.relu(y[:, 0] + din).numpy(), rtol=0, atol=1e-12)
    assert np.allclose(nrm[:, :2], -y[:, 1:].numpy(), rtol=0, atol=1e-12) and np.all(nrm[:, 2] == 1)
    assert np.allclose(V.dn_tail(x.numpy(), w.numpy(), bias.numpy(), OH, OW)[1], y[:, 0].numpy(), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ points
@pytest.mark.parametrize("hw", [(3, 5), (23, 37)])
def test_points_are_the_scripts_expression(hw):
    height, width = hw
    rs = np.random.RandomState(width)
    pred = (rs.rand(height, width) * 20.0).astype(np.float32)
    color_image = rs.randint(0, 256, (height, width, 3)).astype(np.uint8)
    focal_length_x, focal_length_y = 470.4, 431.7
    x, y = np.meshgrid(np.arange(width), np.arange(height))       # depth_to_pointcloud.py:99-104
    x = (x - width / 2) / focal_length_x
    y = (y - height / 2) / focal_length_y
    z = np.array(pred)
    points = np.stack((np.multiply(x, z), np.multiply(y, z), z), axis=-1).reshape(-1, 3)
    colors = np.array(color_image).reshape(-1, 3) / 255.0
    gp, gc = V.depth_to_points(pred, color_image, focal_length_x, focal_length_y)
    assert gp.dtype == np.float64 and np.array_equal(gp, points) and np.array_equal(gc, colors)
