"""The score patterns of tests/attn_cases.py have teeth: a CPU fp32 restatement of the kernels' tiled online softmax (64-key
tiles, lazy reference point, per-row m and l, optional fp16 P) passes every case, and each of seven ways to get it wrong fails
at least one. No GPU."""
import math

import pytest
import torch

import attn_cases as AC
from common import rel_l2, worst_px

SHAPES = ((130, 321), (70, 1100))   # the GPU tests' flash shape; 18 key tiles, where a frozen reference point leaves fp32
DH, SCALE = 64, 0.125
MUTANTS = ("no_max", "frozen", "bump_o_only", "bump_l_only", "unmasked", "tile_max", "lazy20_p16")
LOG2E = 1.4426950408889634


def tiled(q, k, v, scale, *, p16=False, lazy=6.0, mutant=None, tile=64, rows=64, group=32):
    """fp32 online softmax as flash_attn_kernel runs it: raw scores per 64-key tile, the reference point m moves only when a
    row of the 32-query group exceeds it by 2^lazy (then for every row of the group, to its own maximum), P = exp2 of the
    difference, optionally rounded to fp16, l and o rescaled by alpha on a bump."""
    nq, nk = q.shape[0], k.shape[0]
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    nt = (nk + tile - 1) // tile
    kp = torch.zeros(nt * tile, k.shape[1])
    vp = torch.zeros(nt * tile, v.shape[1])
    kp[:nk], vp[:nk] = k, v
    m = torch.full((nq,), -1e30)
    l = torch.zeros(nq)
    o = torch.zeros(nq, v.shape[1])
    grp = torch.arange(nq) // group
    rt = torch.arange(nq) // rows
    for t in range(nt):
        s = q @ kp[t * tile:(t + 1) * tile].t()
        if mutant != "unmasked":
            s[:, max(0, nk - t * tile):] = -math.inf
        mx = s.max(dim=1).values
        if mutant == "no_max":
            m_new = torch.zeros(nq)
            alpha = torch.ones(nq)
        else:
            need = (mx - m) * sl2 > lazy
            bump = torch.zeros(int(grp.max()) + 1, dtype=torch.bool).index_put_((grp,), need, accumulate=True)[grp]   # wave-uniform
            if mutant == "frozen" and t > 0:
                bump = torch.zeros_like(bump)
            to = mx
            if mutant == "tile_max":
                to = torch.full((int(rt.max()) + 1,), -math.inf).scatter_reduce(0, rt, mx, "amax")[rt]
            m_new = torch.where(bump, torch.maximum(m, to), m)
            alpha = torch.exp2((m - m_new) * sl2)
        m = m_new
        p = torch.exp2(s * sl2 - (m * sl2)[:, None])
        if p16:
            p = p.half().float()
        l = l * (1.0 if mutant == "bump_o_only" else alpha) + p.sum(dim=1)
        o = o * (1.0 if mutant == "bump_l_only" else alpha[:, None]) + p @ vp[t * tile:(t + 1) * tile]
    return o / l[:, None]


def _inputs():
    for nq, nk in SHAPES:
        for case in AC.CASES:
            q, k, v = AC.make(case, nq, nk, DH, SCALE, seed=nk)
            yield case, nq, nk, q, k, v


def _fails(got, ref, bar, bar_px):
    return (not bool(torch.isfinite(got).all())) or not (rel_l2(got, ref) < bar and worst_px(got, ref) < bar_px)


@pytest.fixture(scope="module")
def table():
    """(case, nq, nk) -> inputs, fp64 reference, e32 and the bars of the fp32 (B = 1e-5) and the fp16-P (B = 3e-4) restatement."""
    rows = []
    for case, nq, nk, q, k, v in _inputs():
        ref, e32, bar, bar_px = AC.bars(q, k, v, SCALE, 1e-5, 8)
        _, _, bar16, bar16_px = AC.bars(q, k, v, SCALE, 3e-4, 8)
        rows.append(dict(case=case, nq=nq, nk=nk, q=q, k=k, v=v, ref=ref, e32=e32, bars={False: (bar, bar_px), True: (bar16, bar16_px)}))
    return rows


def test_every_case_is_generated_and_well_conditioned(table):
    assert {r["case"] for r in table} == set(AC.CASES) and len(table) == len(AC.CASES) * len(SHAPES)   # none skipped
    for r in table:
        r32 = AC.ref32(r["q"], r["k"], r["v"], SCALE)
        assert bool(torch.isfinite(r32).all()) and bool(torch.isfinite(r["ref"]).all()), r["case"]
        print(f"{r['case']:14s} {r['nq']}x{r['nk']}  e32 {r['e32']:.2e}")
        assert r["e32"] < 1e-4, (r["case"], r["e32"])   # the conditioned bar never rises to where it would hide a real error


def test_patterns_are_what_they_claim(table):
    """On the half-rounded operands: the offsets sit at +-120, a one-hot row is its V row, a flat row the mean of V, the ramps
    gain their bits per tile, and the mixed tile has its spike row next to rows whose maximum is in tile 0."""
    for r in table:
        case, nk = r["case"], r["nk"]
        q, k, v = (t.half().double() for t in (r["q"], r["k"], r["v"]))
        s = q @ k.t() * SCALE
        out = AC.attend64(s, v)
        if case in ("offset_pos", "offset_neg"):
            sign = 1 if case == "offset_pos" else -1
            assert float((s * sign).min()) > AC.OFFSET - 8 and float((s * sign).max()) < AC.OFFSET + 8
        elif case in ("one_hot_last", "one_hot_first"):
            hot = nk - 1 if case == "one_hot_last" else 0
            others = torch.cat([s[:, :hot], s[:, hot + 1:]], dim=1)
            assert float((s[:, hot] - others.max(dim=1).values).min()) >= 60
            assert rel_l2(out, v[hot].expand_as(out)) < 1e-12
        elif case == "flat":
            assert rel_l2(out, v.mean(dim=0).expand_as(out)) < 1e-12
        elif case.startswith("ramp"):
            bits = {"ramp_up_fast": AC.FAST, "ramp_up_slow": AC.SLOW, "ramp_down": -AC.DOWN}[case]
            tile_mean = torch.stack([s[:, t * 64:(t + 1) * 64].mean() for t in range(nk // 64)]) / AC.LN2
            assert float(((tile_mean[1:] - tile_mean[:-1]) - bits).abs().max()) < 0.5, (case, tile_mean)
        elif case == "mixed_rows":
            arg = s.argmax(dim=1)
            spike = torch.arange(r["nq"]) % 64 == AC.SPIKE_ROW
            assert bool((arg[spike] == nk - 1).all()) and float(s[spike, nk - 1].min()) > AC.HOT - 8
            big = torch.arange(r["nq"]) % 4 >= 2
            assert bool((arg[big & ~spike] < 64).all())
            assert float(s[torch.arange(r["nq"]) % 4 == 3].abs().max()) > 35   # the +-40 rows next to the gain-0 rows


def test_correct_restatement_passes_every_case(table):
    for r in table:
        for p16 in (False, True):
            got = tiled(r["q"], r["k"], r["v"], SCALE, p16=p16)
            bar, bar_px = r["bars"][p16]
            err, px = rel_l2(got, r["ref"]), worst_px(got, r["ref"])
            print(f"{r['case']:14s} {r['nq']}x{r['nk']} p16={int(p16)}  rel-L2 {err:.2e} worst {px:.2e}  e32 {r['e32']:.2e}  bar {bar:.1e} / {bar_px:.1e}")
            assert not _fails(got, r["ref"], bar, bar_px), (r["case"], p16, err, px, bar, bar_px)


def test_every_mutant_is_caught(table):
    """Each mutant runs with P in fp32 and with P rounded to fp16 (the pv = 1 / 2 kernels), against that mode's bar; lazy20_p16
    exists with fp16 P only. Failing = over the bar or non-finite."""
    caught = {}
    for mutant in MUTANTS:
        hits = []
        for p16 in ((True,) if mutant == "lazy20_p16" else (False, True)):
            for r in table:
                kw = dict(lazy=20.0) if mutant == "lazy20_p16" else dict(mutant=mutant)
                got = tiled(r["q"], r["k"], r["v"], SCALE, p16=p16, **kw)
                if _fails(got, r["ref"], *r["bars"][p16]):
                    hits.append(f"{r['case']}@{r['nk']}{'/p16' if p16 else ''}")
        caught[mutant] = hits
        print(f"{mutant:12s} caught by: {', '.join(hits) if hits else 'NOTHING'}")
    for mutant, hits in caught.items():
        assert hits, f"mutant {mutant} survives every case"
        if mutant != "lazy20_p16":   # and with P kept in fp32, so the fp32-P kernels are held too
            assert any(not h.endswith("/p16") for h in hits), f"mutant {mutant} survives every case with fp32 P: {hits}"
