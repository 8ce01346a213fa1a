"""CPU restatement of the v2 / v3 depth-refiner wrappers' forward (models/video_depth_model_v2.py:75-100,
models/video_depth_model_v3.py:167-206), built from the oracle's pieces: the encoder + temporal head with `head.*` keys
(O.video_depth_anything_forward), the Sobel normals (O.sobel_normals) and torch.quantile. tools/make_golden_refiners.py
holds it to <= 1e-5 of the imported reference before it writes a fixture; v4 / v5 are O.depth_refiner_forward."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O

# The twelve final_res scalars of the R2 fixture. The plain synthetic draw gives the first BatchNorm a negative gamma, the
# first ReLU then zeroes every pixel and the output is one constant; these leave both ReLUs partly active on the fixture clip.
R2_FINAL_RES = {
    "final_res.0.weight": [0.9, -1.1], "final_res.0.bias": [0.05],
    "final_res.1.weight": [1.2], "final_res.1.bias": [-0.3], "final_res.1.running_mean": [0.1], "final_res.1.running_var": [0.8],
    "final_res.3.weight": [-0.8], "final_res.3.bias": [0.4],
    "final_res.4.weight": [1.1], "final_res.4.bias": [0.05], "final_res.4.running_mean": [-0.1], "final_res.4.running_var": [1.3],
}


def with_final_res(sd, values=R2_FINAL_RES):
    """A copy of the state dict `sd` with the final_res scalars replaced (shapes kept)."""
    sd = dict(sd)
    for k, v in values.items():
        sd[k] = torch.as_tensor(v, dtype=torch.float32).reshape(sd[k].shape)
    return sd


def r2_state_dict(g, base):
    """`base` (synth_sd("R2", ...)) with the final_res scalars the R2 fixture `g` was made with, stored in it under "sd/<key>"."""
    return with_final_res(base, {k[3:]: g[k] for k in g.files if k.startswith("sd/")})


def final_res(sd, depth, x, trace=None, p="final_res."):
    """v2:64-72,96-97: Conv2d(2,1,1) - BatchNorm2d(1) - ReLU - Conv2d(1,1,1) - BatchNorm2d(1) - ReLU on stack([depth, x]),
    BatchNorm in eval mode (eps 1e-5). depth, x [N,H,W] -> [N,H,W], in the dtype of the inputs."""
    def get(k):
        return sd[p + k].to(depth.dtype)

    def bn(t, i):
        return F.batch_norm(t, get(f"{i}.running_mean"), get(f"{i}.running_var"), get(f"{i}.weight"), get(f"{i}.bias"), False, 0.0, 1e-5)

    t = bn(F.conv2d(torch.stack([depth, x], dim=1), get("0.weight"), get("0.bias")), 1)
    if trace is not None:
        trace["pre_relu1"] = t[:, 0]
    t = bn(F.conv2d(F.relu(t), get("3.weight"), get("3.bias")), 4)
    return F.relu(t)[:, 0]


def refiner23_forward(sd, input_depth, encoder="vitl", version=3, use_residual=True, input_normal=True, trace=None):
    """input_depth [B,S,H,W] in [0, 65535], H and W multiples of 14 -> [B,S,H,W], normalised (neither version multiplies
    the result back by 65535)."""
    assert version in (2, 3)
    B, S, H, W = input_depth.shape
    x = input_depth / 65535.0                                                   # v2:77, v3:169
    if version == 3:                                                            # v3:175-177, GlobalScaleHead v3:63-87,165
        med = torch.quantile(x.reshape(B * S, -1), 0.5, dim=-1)
        g = med * sd["final_scale2.feat.1.weight"].reshape(()) + sd["final_scale2.feat.1.bias"].reshape(())
        scale = torch.exp(torch.tanh(g) * 1.0)
        x = x * scale.reshape(B, S, 1, 1)
        if trace is not None:
            trace.update(median=med, scale=scale)
    d1 = x.reshape(B * S, 1, H, W)
    net_in = torch.cat([d1, O.sobel_normals(d1)[:, :2]], dim=1) if input_normal else d1.expand(-1, 3, -1, -1)   # v2:78-85, v3:179-186
    # encoder, temporal head, resize to (H, W), ReLU: v2:87-92, v3:188-193
    out = O.video_depth_anything_forward(sd, net_in.reshape(B, S, 3, H, W), encoder, pre_relu=False, head_prefix="head.")
    if trace is not None:
        trace["net_depth"] = out
    if use_residual and version == 3:                                           # v3:203-204
        out = x + (out * sd["final_res2.0.weight"].reshape(()) + sd["final_res2.0.bias"].reshape(()))
    elif use_residual:                                                          # v2:96-98
        out = final_res(sd, out.flatten(0, 1), x.flatten(0, 1), trace).unflatten(0, (B, S))
    return out
