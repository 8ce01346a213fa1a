"""From-scratch torch restatement of the Hiera trunk (hiera_{tiny,small,base}_224, inference, no masking) on a state dict
keyed by the hub names vdn.HieraImageEncoder holds (without the `model.` prefix). tools/make_golden_hiera.py proves it equal
to the `transformers` port of the model to 1e-5 on every stage output; the tests use it for kernel-level references and for
the attention row addressing. The `fault` switches restate the four mistakes the fixtures must be able to see."""
import torch
import torch.nn.functional as Fn

EMBED_DIM, HEAD_DIM, HEADS = 96, 96, (1, 2, 4, 8)
SIDE, TOKENS, WINDOWS = 56, 3136, 49
LN_EPS = 1e-6
FAULTS = ("no_q_pool", "no_res_pool", "global", "no_unroll")


def unroll_index(n=3):
    """perm [T]: unrolled token u of a (7 << n)-sided grid with n stride-2 levels is row-major token perm[u]."""
    side = 7 << n
    idx = torch.arange(side * side).reshape(1, side, side)
    for _ in range(n):
        b, h, w = idx.shape
        idx = idx.reshape(b, h // 2, 2, w // 2, 2).permute(0, 2, 4, 1, 3).reshape(b * 4, h // 2, w // 2)
    return idx.reshape(-1)


def reroll(x, stage):
    """unrolled tokens [N, T, C] of `stage` -> NHWC [N, side, side, C]."""
    side = SIDE >> stage
    out = torch.empty_like(x)
    out[:, unroll_index(3 - stage)] = x
    return out.reshape(x.shape[0], side, side, x.shape[-1])


def embed(sd, img, unrolled=True):
    """patch_embed.proj (7 x 7, stride 4, pad 3) + pos_embed -> tokens [N, 3136, 96], in unrolled order."""
    x = Fn.conv2d(img, sd["patch_embed.proj.weight"].to(img.dtype), sd["patch_embed.proj.bias"].to(img.dtype), stride=4, padding=3)
    x = x.flatten(2).transpose(1, 2) + sd["pos_embed"].to(img.dtype)
    return x[:, unroll_index(3)] if unrolled else x


def attn_rows(qkv, heads, W, Lkv, qs, scale=HEAD_DIM ** -0.5):
    """Mask-unit attention on packed rows: qkv [N, W*Lkv, 3*heads*96] with token t of window w at row t*W + w and columns
    q | k | v, each [heads][96]; query j of a q-stride block is the max over rows t = g*Lq + j. -> [N, W*Lq, heads*96] with
    query j of window w at row j*W + w. Plain loops over the index arithmetic of the table, no reshape tricks."""
    N = qkv.shape[0]
    C = heads * HEAD_DIM
    Lq = Lkv // qs
    out = qkv.new_empty(N, W * Lq, C)
    t = torch.arange(Lkv)
    j = torch.arange(Lq)
    for w in range(W):
        rows = t * W + w
        for h in range(heads):
            c = slice(h * HEAD_DIM, (h + 1) * HEAD_DIM)
            q = qkv[:, rows][:, :, c]
            k = qkv[:, rows][:, :, C + h * HEAD_DIM:C + (h + 1) * HEAD_DIM]
            v = qkv[:, rows][:, :, 2 * C + h * HEAD_DIM:2 * C + (h + 1) * HEAD_DIM]
            if qs > 1:
                q = torch.stack([q[:, g * Lq + j] for g in range(qs)], 0).max(0).values
            p = torch.softmax(q @ k.transpose(1, 2) * scale, dim=-1)
            out[:, j * W + w, c] = p @ v
    return out


def _ln(x, w, b):
    return Fn.layer_norm(x, (x.shape[-1],), w.to(x.dtype), b.to(x.dtype), LN_EPS)


def _lin(x, sd, name):
    return Fn.linear(x, sd[name + ".weight"].to(x.dtype), sd[name + ".bias"].to(x.dtype))


def geometry(stage, first, fault=None):
    tokens_in = TOKENS >> (2 * (stage - 1 if first and stage > 0 else stage))
    qs = 4 if first and stage > 0 else 1
    windowed = (stage < 2 or (stage == 2 and first)) and fault != "global"
    W = WINDOWS if windowed else 1
    return W, tokens_in // W, qs


def block(sd, n, x, stage, first, fault=None):
    p = f"blocks.{n}."
    W, Lkv, qs = geometry(stage, first, fault)
    heads = HEADS[stage]
    C = EMBED_DIM << stage
    xn = _ln(x, sd[p + "norm1.weight"], sd[p + "norm1.bias"])
    if qs > 1:
        r = _lin(xn, sd, p + "proj")
        N, T, _ = r.shape
        x = r[:, :T // 4] if fault == "no_res_pool" else r.reshape(N, 4, T // 4, C).max(1).values
    qkv = _lin(xn, sd, p + "attn.qkv")
    if qs > 1 and fault == "no_q_pool":   # the first group's queries alone
        Lq = Lkv // qs
        keep = (torch.arange(Lq)[:, None] * W + torch.arange(W)[None, :]).reshape(-1)
        full = attn_rows(qkv, heads, W, Lkv, 1)
        a = full[:, keep]
    else:
        a = attn_rows(qkv, heads, W, Lkv, qs)
    x = x + _lin(a, sd, p + "attn.proj")
    h = Fn.gelu(_lin(_ln(x, sd[p + "norm2.weight"], sd[p + "norm2.bias"]), sd, p + "mlp.fc1"))
    return x + _lin(h, sd, p + "mlp.fc2")


def forward(sd, img, depths, fault=None):
    """-> (four NHWC stage maps, taps {'embed', 'first0'..'first3'} of the unrolled stream)."""
    x = embed(sd, img, unrolled=fault != "no_unroll")
    taps = {"embed": x}
    maps, n = [], 0
    for s, d in enumerate(depths):
        for i in range(d):
            x = block(sd, n, x, s, i == 0, fault)
            if i == 0:
                taps[f"first{s}"] = x
            n += 1
        maps.append(reroll(x, s))
    return maps, taps
