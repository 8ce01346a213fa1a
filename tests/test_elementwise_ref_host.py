"""The float64 restatements of tests/elementwise_ref.py against torch's own operators in float64, and the GroupNorm accuracy
inputs against torch's float32 group_norm: the bars of tests/test_gpu_elementwise_edges.py rest on both. No GPU."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as E

# shapes and ratios of the GPU accuracy test (test_groupnorm_accuracy_against_torch_fp32)
GN_ACC_SHAPES = [(361, 256), (1369, 256), (361, 1024)]
GN_ACC_K = [0.25, 4, 16, 64, 256]


def _same(a, b, tol=1e-12):
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float64
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_layer_norm_restatement():
    rows, C = 23, 36
    x, w, b = E.noise(rows, C, seed=1) * 3 + 1, E.noise(C, seed=2), E.noise(C, seed=3)
    vec, tab = E.noise(C, seed=4), E.noise(5, C, seed=5)
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), 1e-6)
    _same(E.layer_norm(x, w, b, 1e-6), ref)
    idx = (torch.arange(rows) // 7) % 5
    _same(E.layer_norm(x, w, b, 1e-6, addvec=vec, alpha=0.5, tab=tab, tab_div=7, tab_mod=5), ref + 0.5 * vec.double() + tab.double()[idx])
    keep = [r for r in range(rows) if r % 11 != 0]
    got = E.layer_norm(x, w, b, 1e-6, out_group=11)
    assert got.shape[0] == rows - -(-rows // 11)
    _same(got, ref[keep])


@pytest.mark.parametrize("F_,HW,C,groups", [(2, 50, 8, 1), (1, 3, 64, 32), (1, 1, 64, 32), (2, 10, 264, 33), (1, 13, 128, 64)])
def test_group_norm_restatement(F_, HW, C, groups):
    x, w, b = E.noise(F_, HW, C, seed=6) * 2 + 0.5, E.noise(C, seed=7), E.noise(C, seed=8)
    ref = F.group_norm(x.double().permute(0, 2, 1), groups, w.double(), b.double(), 1e-6).permute(0, 2, 1)
    _same(E.group_norm(x, groups, w, b, 1e-6), ref)


def test_elementwise_restatements():
    x, vec, tab = E.noise(37, 36, seed=9), E.noise(36, seed=10), E.noise(3, 36, seed=11)
    _same(E.add_vec(x, vec, 0.1), torch.add(x.double(), vec.double(), alpha=0.1))
    _same(E.addtab_cast(x), x.double())
    rows = torch.arange(37)
    _same(E.addtab_cast(x, tab, 5, 3), x.double() + tab.double()[torch.div(rows, 5, rounding_mode="floor") % 3])


def test_bilinear_restatement():
    """float32 sample positions against torch's float64 ones: the weights differ by half an ulp of the coordinate at most."""
    x = E.noise(2, 9, 7, 8, seed=12)
    ref = F.interpolate(x.double().permute(0, 3, 1, 2), (20, 13), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    _same(E.bilinear_ac(x, 20, 13), ref, tol=2.0 ** -24 * 20 * 4)
    _same(E.bilinear_ac(x[..., 0], 20, 13), ref[..., 0], tol=2.0 ** -24 * 20 * 4)


def test_patchify_head_out_dwconv7_restatements():
    img = E.noise(2, 3, 28, 42, seed=13)
    _same(E.patchify(img.double()), F.unfold(img.double(), 14, stride=14).transpose(1, 2).reshape(2 * 6, 588))
    f, w = E.noise(50, 16, seed=14), E.noise(16, seed=15)
    _same(E.head_out(f, w, 0.3, False), F.linear(f.double(), w.double()[None], torch.tensor([0.3], dtype=torch.float64))[:, 0])
    _same(E.head_out(f, w, 0.3, True), F.relu(F.linear(f.double(), w.double()[None], torch.tensor([0.3], dtype=torch.float64))[:, 0]))
    x, wc, b = E.noise(2, 5, 9, 6, seed=16), E.noise(6, 1, 7, 7, seed=17), E.noise(6, seed=18)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), wc.double(), b.double(), padding=3, groups=6).permute(0, 2, 3, 1)
    _same(E.dwconv7(x, wc.reshape(6, 49).t(), b), ref)


def test_tagged_inputs_tell_rows_and_channels_apart():
    x = E.tagged(2 * E.NOISE_ROWS + 5, 12, seed=19, dtype=torch.float16)
    assert torch.equal(x, x.half().float())                       # already values of the operand type
    assert float((x[E.NOISE_ROWS:2 * E.NOISE_ROWS] - x[:E.NOISE_ROWS]).abs().min()) > 0.005   # the repeat of the noise block is still a different row
    c = E.cast_input(200_003, seed=20)
    assert bool(c.isnan().any()) and bool(c.isinf().any()) and bool((c.abs() < 2.0 ** -126).logical_and(c != 0).any())


@pytest.mark.parametrize("HW,C", GN_ACC_SHAPES)
def test_groupnorm_accuracy_inputs_are_well_posed_for_fp32(HW, C):
    """torch's float32 group_norm on the N(k, 1) inputs stays below 1e-4 rel-L2 of the float64 restatement for every k of the GPU
    test: the bound there, 4 x this error, is a bound and not a licence."""
    w, b = 1 + 0.25 * E.noise(C, seed=21), 0.25 * E.noise(C, seed=22)
    for k in GN_ACC_K:
        _, _, x = E.gn_input(2, HW, C, k, seed=23)
        ref = E.group_norm(x, 32, w, b, 1e-6)
        got = F.group_norm(x.permute(0, 2, 1), 32, w, b, 1e-6).permute(0, 2, 1)
        err, mx = E.errors64(got, ref)
        print(f"torch fp32 group_norm HW={HW} C={C} k={k}: rel-L2 {err:.2e} worst {mx:.2e}")
        assert err < 1e-4, (k, err)
