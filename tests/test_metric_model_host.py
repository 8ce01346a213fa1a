"""Host side of the metric-depth model (vdn.metric_depth): the constructor contract, the state-dict keys of an upstream
metric checkpoint, and the condition the M* fixtures were generated under (tools/make_golden_metric_model.py). No GPU."""
import inspect
import os

import numpy as np
import pytest
import torch

from common import GOLD, schema

FIXTURES = [("M_vits_266x350", "M", "vits", {}), ("Mf_vits_266", "Mf", "vits", dict(use_bn=True, use_clstoken=True)),
            ("M_vitl_518_heavy", "M", "vitl", {})]


def _cls():
    from vdn.metric_depth.depth_anything_v2.dpt import DepthAnythingV2
    return DepthAnythingV2


def test_constructor_signature_is_the_reference_s():
    """metric_depth/depth_anything_v2/dpt.py:153-161: the six parameters, their order and their defaults."""
    p = inspect.signature(_cls().__init__).parameters
    assert list(p) == ["self", "encoder", "features", "out_channels", "use_bn", "use_clstoken", "max_depth"]
    got = {k: v.default for k, v in p.items() if k != "self"}
    assert got == dict(encoder="vitl", features=256, out_channels=[256, 512, 1024, 1024], use_bn=False, use_clstoken=False,
                       max_depth=20.0)


def test_import_paths_of_the_reference_scripts():
    """run.py:8, train.py:20 and depth_to_pointcloud.py:21 import depth_anything_v2.dpt; the main copy's file name and the
    package attribute give the same class."""
    import vdn.metric_depth
    from vdn.metric_depth.depth_anything_v2.depth_anything_v2 import DepthAnythingV2 as again
    assert again is _cls() and vdn.metric_depth.DepthAnythingV2 is _cls()
    import vdn
    assert _cls() is not vdn.DepthAnythingV2
    for m in ("forward", "infer_image", "image2tensor", "infer_image_vis", "infer_image_points"):
        assert callable(getattr(_cls(), m)), m
    assert not hasattr(_cls(), "clear_memory")
    from vdn.points import depth_to_points
    assert callable(depth_to_points)


@pytest.mark.parametrize("which,enc,flags", [(w, e, f) for _, w, e, f in FIXTURES])
def test_state_dict_schema_matches_the_composed_reference(which, enc, flags):
    """Constructs on the CPU; parameter and buffer names and shapes are those of the reference's live DINOv2 and DPTHead under
    `pretrained.` and `depth_head.`; there is no memory block; its own state dict loads with strict=True."""
    import vdn
    m = _cls()(**dict(vdn.MODEL_CONFIGS[enc], **flags))
    sch = schema(which, enc)
    assert {k: tuple(v.shape) for k, v in m.named_parameters()} == {k: tuple(s) for k, s in sch["params"]}
    assert {k: tuple(v.shape) for k, v in m.named_buffers()} == {k: tuple(s) for k, s in sch["buffers"]}
    sd = m.state_dict()
    assert sd and all(k.startswith(("pretrained.", "depth_head.")) for k in sd)
    assert not any("memory" in k for k in sd)
    assert not hasattr(m, "memory_block")
    m.load_state_dict(sd, strict=True)
    assert m.max_depth == 20.0 and _cls()(**vdn.MODEL_CONFIGS["vits"], max_depth=80).max_depth == 80


def test_encoders_construct():
    """vits and vitb here (vitl is built by the schema test, ViT-g by the next one); the tap table names all four
    (dpt.py:164-169)."""
    import vdn
    for enc in ("vits", "vitb"):
        m = _cls()(**vdn.MODEL_CONFIGS[enc])
        assert m.pretrained.embed_dim == vdn.modules.ENCODERS[enc]["dim"]
    assert m.intermediate_layer_idx == {"vits": [2, 5, 8, 11], "vitb": [2, 5, 8, 11], "vitl": [4, 11, 17, 23],
                                        "vitg": [9, 19, 29, 39]}


def test_vitg_constructs_with_the_reference_s_keys():
    """ViT-g on the meta device (1.1 G parameters, none allocated): its `pretrained.*` and `depth_head.*` names and shapes are
    those of the relative model's ViT-g schema, whose DINOv2 is the same file and whose DPT head differs in the last,
    parameter-free activation only."""
    import vdn
    with torch.device("meta"):
        m = _cls()(**vdn.MODEL_CONFIGS["vitg"])
    sch = schema("A", "vitg")
    want = {k: tuple(s) for k, s in sch["params"] if k.startswith(("pretrained.", "depth_head."))}
    assert len(want) > 600 and {k: tuple(v.shape) for k, v in m.named_parameters()} == want
    assert not list(m.named_buffers())
    assert m.pretrained.blocks[0].mlp.w12.weight.shape == (2 * 4096, 1536)   # the SwiGLU FFN


def test_model_refuses_cpu():
    import vdn
    from vdn._abi import VdnError
    m = _cls()(**vdn.MODEL_CONFIGS["vits"])
    with pytest.raises(VdnError, match="no CPU path"):
        m.forward(torch.zeros(1, 3, 14, 14))


@pytest.mark.parametrize("name", [f[0] for f in FIXTURES])
def test_fixture_reaches_both_ends_of_the_sigmoid(name):
    """The condition the generator asserts, re-checked from the stored reference map: at least 1 % of the pixels below 0.05
    max_depth, 1 % above 0.95 max_depth and 20 % inside 0.2 .. 0.8 — a ReLU or a clamp in place of the sigmoid would not pass
    the parity test on such a map. The stored logits give the stored depth, and the gain is 4 or more."""
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    md = float(g["max_depth"])
    s = g["depth"].astype(np.float64) / md
    assert s.min() >= 0.0 and s.max() <= 1.0
    assert (s < 0.05).mean() >= 0.01 and (s > 0.95).mean() >= 0.01 and ((s > 0.2) & (s < 0.8)).mean() >= 0.20
    assert float(g["gain"]) >= 4.0
    B, H, W, sub, ls, _ = [int(v) for v in g["meta"]]
    assert g["depth"].shape == (B, -(-H // sub), -(-W // sub)) and g["logits"].shape == (B, -(-H // ls), -(-W // ls))
    step = sub // ls
    lg = torch.from_numpy(g["logits"][:, ::step, ::step])
    # a few ulp: torch's vectorised and scalar sigmoid (full map there, strided sample here) differ in the last bit
    assert torch.allclose(torch.sigmoid(lg.contiguous()) * md, torch.from_numpy(g["depth"]), rtol=4e-6, atol=0)
    assert g["last_weight"].shape == (1, 32, 1, 1) and g["last_bias"].shape == (1,)


def test_points_argument_checks_need_no_device():
    from vdn.points import depth_to_points
    d, c = torch.zeros(4, 5), torch.zeros(4, 5, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        depth_to_points(torch.zeros(2, 4, 5), c, 1.0, 1.0)
    with pytest.raises(ValueError):
        depth_to_points(d, c.float(), 1.0, 1.0)
    with pytest.raises(ValueError):
        depth_to_points(d, torch.zeros(4, 6, 3, dtype=torch.uint8), 1.0, 1.0)
    with pytest.raises(ValueError):
        depth_to_points(d, c, 0.0, 1.0)
    with pytest.raises(ValueError):
        depth_to_points(d, c, 1.0, float("nan"))
