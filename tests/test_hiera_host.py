"""Native Hiera trunk (vdn.HieraImageEncoder): host-side checks, no GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import hiera_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SIZES = {"hiera_tiny_224": ("tiny", (1, 2, 7, 2)), "hiera_small_224": ("small", (1, 2, 11, 2)), "hiera_base_224": ("base", (2, 3, 16, 3))}
SYMBOLS = ("vdn_hiera_embed", "vdn_hiera_attn", "vdn_hiera_pool", "vdn_hiera_reroll")


@pytest.mark.parametrize("name", sorted(SIZES))
def test_state_dict_matches_schema_and_loads_strict(name):
    import vdn
    from dn_fixture import state_dict
    short, depths = SIZES[name]
    with open(os.path.join(GOLD, f"schema_hiera_{short}.json")) as f:
        sch = json.load(f)
    m = vdn.HieraImageEncoder(name)
    assert m.depths == depths
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(s) for k, s in sch["params"]}
    assert got["model.pos_embed"] == (1, 3136, 96) and got["model.patch_embed.proj.weight"] == (96, 3, 7, 7)
    assert got["model.head.projection.weight"] == (1000, 768) and got["model.norm.weight"] == (768,)
    first = [0, depths[0], depths[0] + depths[1], depths[0] + depths[1] + depths[2]]
    with_proj = sorted(int(re.match(r"model\.blocks\.(\d+)\.proj\.weight", k).group(1)) for k in got if re.match(r"model\.blocks\.\d+\.proj\.weight", k))
    assert with_proj == first[1:]
    assert got[f"model.blocks.{first[1]}.attn.qkv.weight"] == (3 * 192, 96)
    m.load_state_dict(state_dict(m), strict=True)
    assert float(m.model.pos_embed.detach().abs().max()) > 0


def test_base_parameter_count():
    import vdn
    m = vdn.HieraImageEncoder("hiera_base_224")
    trunk = sum(p.numel() for k, p in m.named_parameters() if not k.startswith(("model.norm.", "model.head.")))
    assert round(trunk / 1e6, 1) == 50.8, trunk   # hiera_base_224 without its classifier end: 50.8 M


def test_rename_table_covers_every_key():
    from vdn.hiera_image_encoder import DEPTHS, HieraImageEncoder, transformers_key
    depths = DEPTHS["hiera_base_224"]
    keys = [k[len("model."):] for k in HieraImageEncoder("hiera_base_224").state_dict()]
    mapped = [transformers_key(k, depths) for k in keys]
    assert sum(t is None for t in mapped) == 4   # norm.{weight,bias}, head.projection.{weight,bias}
    named = [t for t in mapped if t is not None]
    assert len(set(named)) == len(named)
    assert transformers_key("blocks.5.attn.qkv.weight", depths) == "encoder.stages.2.layers.0.attn.qkv.weight"
    assert transformers_key("blocks.1.norm1.bias", depths) == "encoder.stages.0.layers.1.layernorm_before.bias"
    assert transformers_key("pos_embed", depths) == "embeddings.position_embeddings"
    with pytest.raises(KeyError):
        transformers_key("blocks.0.attn.rel_pos.weight", depths)


def test_refused_names_and_input_size():
    import vdn
    for n in ("hiera_base_plus_224", "hiera_large_224", "hiera_huge_224"):
        with pytest.raises(NotImplementedError, match="96"):
            vdn.HieraImageEncoder(n)
    with pytest.raises(ValueError, match="Unsupported model"):
        vdn.HieraImageEncoder("dinov2_vits14")
    m = vdn.HieraImageEncoder("hiera_tiny_224")
    for shape in ((1, 3, 256, 256), (1, 3, 224, 256), (1, 1, 224, 224)):
        with pytest.raises(ValueError, match="224"):
            m(torch.zeros(shape))


def test_set_finetune_only_flips_requires_grad():
    import vdn
    m = vdn.HieraImageEncoder("hiera_tiny_224", finetune=False)
    assert not any(p.requires_grad for p in m.parameters())
    m.set_finetune(True)
    assert all(p.requires_grad for p in m.parameters()) and m.finetune is True


def test_unroll_and_reroll_tables_equal_the_fixture():
    """The package's host-side token order (vdn.hiera_engine.unroll_index, what the embedding's pos_embed permutation uses)
    and the restatement's reroll against the tables the fixture generator took from the oracle's own unroll / reroll."""
    from vdn.hiera_engine import unroll_index
    with np.load(os.path.join(GOLD, "hiera_tiny_f2.npz")) as z:
        assert np.array_equal(unroll_index(3).numpy(), z["unroll"])
        assert np.array_equal(HR.unroll_index(3).numpy(), z["unroll"])
        for s in range(4):
            T = 3136 >> (2 * s)
            got = HR.reroll(torch.arange(T, dtype=torch.float32).reshape(1, T, 1), s).reshape(-1).long().numpy()
            assert np.array_equal(got, z[f"reroll{s}"]), s
            # reroll undoes the unroll of a stage that has n = 3 - s levels left
            assert np.array_equal(unroll_index(3 - s).numpy()[z[f"reroll{s}"]], np.arange(T)), s


def test_attention_geometry_is_the_shape_table():
    from vdn.hiera_engine import attn_geometry
    table = {(0, True): (49, 64, 1), (0, False): (49, 64, 1), (1, True): (49, 64, 4), (1, False): (49, 16, 1),
             (2, True): (49, 16, 4), (2, False): (1, 196, 1), (3, True): (1, 196, 4), (3, False): (1, 49, 1)}
    for (s, first), want in table.items():
        assert attn_geometry(s, first) == want, (s, first)
        assert HR.geometry(s, first) == want


@pytest.mark.parametrize("stage,first", [(0, False), (1, True), (1, False), (2, True), (2, False), (3, True), (3, False)])
def test_attention_row_addressing(stage, first):
    """For the geometry the engine launches each block of the shape table with (vdn.hiera_engine.attn_geometry, HEADS): the
    row / column addressing that vdn_hiera_attn documents, restated as plain index arithmetic in hiera_ref.attn_rows, against
    the reshape / permute formulation of mask-unit attention ([N, t, w, 3, head, 96], the query pooled over g in
    t = g*Lq + j). Beyond the geometry this is a self-check of the reference the GPU tests compare the kernel with."""
    from vdn.hiera_engine import HEAD_DIM, HEADS, attn_geometry
    heads, (W, Lkv, qs) = HEADS[stage], attn_geometry(stage, first)
    assert HEAD_DIM == HR.HEAD_DIM == 96
    g = torch.Generator().manual_seed(heads * 1000 + Lkv)
    N, C = 2, heads * 96
    qkv = torch.randn(N, W * Lkv, 3 * C, generator=g, dtype=torch.float64)
    x = qkv.reshape(N, Lkv, W, 3, heads, 96).permute(3, 0, 4, 2, 1, 5)   # 3, N, head, w, t, d
    q, k, v = x[0], x[1], x[2]
    if qs > 1:
        q = q.reshape(N, heads, W, qs, Lkv // qs, 96).max(dim=3).values
    a = torch.softmax(q * 96 ** -0.5 @ k.transpose(-1, -2), dim=-1) @ v   # N, head, w, j, d
    want = a.permute(0, 3, 2, 1, 4).reshape(N, -1, C)                       # row j*W + w, column head*96 + d
    got = HR.attn_rows(qkv, heads, W, Lkv, qs)
    assert got.shape == want.shape == (N, W * Lkv // qs, C)
    assert float((got - want).abs().max()) < 1e-12


def test_nested_trunks_drop_their_engines_on_the_outer_load():
    """load_state_dict on the outer model never calls the trunks' own load_state_dict: the recursion must still drop their
    packed weights (and the two native trunks share one runtime owner without registering it as a submodule)."""
    import vdn
    m = vdn.VideoDepthEstimationModel.with_native_trunks(8, encoder="hiera_tiny_224")
    assert m.img_encoder._rt_owner == (m.encoder,) and m.encoder._rt_owner == ()
    assert not any(k.startswith("img_encoder.encoder") or "_rt_owner" in k for k in m.state_dict())
    for t in (m, m.encoder, m.img_encoder, m.head):
        t._eng = {"stale": True}
    m.load_state_dict(m.state_dict(), strict=True)
    assert m._eng is None and m.encoder._eng is None and m.img_encoder._eng is None and m.head._eng is None


def test_header_library_and_binding_agree_on_the_new_symbols():
    from vdn import _abi
    with open(os.path.join(ROOT, "include", "vdn.h")) as f:
        hdr = f.read()
    for s in SYMBOLS:
        m = re.search(r"\bint " + s + r"\(([^;]*)\);", hdr)
        assert m, s
        assert len(m.group(1).split(",")) == len(_abi.EXPORTS[s][1]), s
        assert getattr(_abi.lib, s).argtypes == _abi.EXPORTS[s][1]


def test_entry_points_reject_bad_arguments_without_launch():
    from vdn import _abi
    L = _abi.lib
    p = ctypes.c_void_p(256)
    assert L.vdn_hiera_embed(0, None, p, None, 1, 192, None) == -1
    assert L.vdn_hiera_embed(0, p, p, None, 0, 192, None) == -1
    assert L.vdn_hiera_embed(0, p, p, None, 1, 128, None) != 0      # ldk below 147
    assert L.vdn_hiera_embed(0, p, p, None, 1, 200, None) != 0      # not a multiple of 64
    assert L.vdn_hiera_embed(2, p, p, None, 1, 192, None) == -2     # f32 rows
    assert L.vdn_hiera_attn(0, None, None, p, None, 1, 1, 49, 64, 1, 0.1, None) == -1
    assert L.vdn_hiera_attn(0, p, p, p, None, 1, 1, 49, 64, 1, 0.1, None) == -1     # half of the split planes
    assert L.vdn_hiera_attn(0, p, None, p, None, 1, 1, 49, 64, 3, 0.1, None) == -1  # L_kv not a multiple of the stride
    assert L.vdn_hiera_attn(0, p, None, p, None, 1, 0, 49, 64, 1, 0.1, None) == -1
    assert L.vdn_hiera_attn(2, p, None, p, None, 1, 1, 49, 64, 1, 0.1, None) == -2
    assert L.vdn_hiera_pool(None, p, 1, 49, 96, None) == -1
    assert L.vdn_hiera_pool(p, p, 1, 49, 98, None) != 0
    assert L.vdn_hiera_reroll(p, p, 1, 4, 96, None) == -1
    assert L.vdn_hiera_reroll(p, None, 1, 0, 96, None) == -1
    assert L.vdn_hiera_reroll(p, p, 1, 0, 98, None) != 0


def test_with_native_trunks_keys_and_plain_constructor_still_raises():
    import vdn
    from vdn import synth
    with pytest.raises(ValueError, match="trunk"):
        vdn.VideoDepthEstimationModel(8)
    m = vdn.VideoDepthEstimationModel.with_native_trunks(8, encoder="hiera_tiny_224")
    assert isinstance(m.encoder, vdn.HieraImageEncoder) and isinstance(m.img_encoder, vdn.HieraImageEncoder)
    assert m.encoder is not m.img_encoder
    keys = set(m.state_dict())
    with open(os.path.join(GOLD, "schema_hiera_tiny.json")) as f:
        trunk = [k for k, _ in json.load(f)["params"]]
    for pre in ("encoder.", "img_encoder."):
        assert {pre + k for k in trunk} <= keys
    assert sum(k.startswith("head.") for k in keys) == 818
    assert not any(p.requires_grad for p in m.encoder.parameters())
    with pytest.raises(NotImplementedError):
        vdn.VideoDepthEstimationModel.with_native_trunks(8, encoder="hiera_large_224")
    # an injected trunk is still what it was
    inj = vdn.VideoDepthEstimationModel(8, trunk=synth.dn_trunk(), img_trunk=synth.dn_trunk())
    assert not isinstance(inj.encoder, vdn.HieraImageEncoder)


def test_fixtures_present_and_small():
    for n in ("hiera_tiny_f2", "hiera_base_f2", "hiera_base_f8", "dn_model_native"):
        path = os.path.join(GOLD, n + ".npz")
        assert os.path.getsize(path) <= 1 << 20
        with np.load(path) as z:
            assert "meta" in z.files
