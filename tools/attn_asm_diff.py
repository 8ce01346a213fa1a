#!/usr/bin/env python3
"""Compare the flash-attention kernels of two builds of csrc/attn.hip instruction by instruction (profiles/attn_refactor.md
is such a comparison). Make the two inputs with the flags of vdn/_build.py:

    hipcc <flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/attn.hip -o A.s 2> A.remarks
    python tools/attn_asm_diff.py A.s A.remarks B.s B.remarks

Kernels are matched by name and template arguments (a trailing `false` fourth argument of flash_attn_kernel, the QK8 flag it
once had, is dropped). A kernel's text is its lines from the label to .Lfunc_end with comments and directives stripped and
block labels renumbered. A line is IN-LOOP when it lies between a block label and a backward branch to that label. Prints,
per kernel, registers / scratch / occupancy of both builds, every differing line, and the number of differing lines inside
loops."""
import difflib
import re
import sys


def key_of(mangled):
    m = re.search(r"\d+(flash_attn2?_kernel)I((?:L[ib]\d+E)+)E", mangled)
    if not m:
        return None
    name, args = m.group(1), re.findall(r"L[ib](\d+)E", m.group(2))
    if name == "flash_attn_kernel" and len(args) == 4 and args[3] == "0":
        args = args[:3]
    return f"{name}<{','.join(args)}>"


def kernels(path):
    res, cur, name = {}, None, None
    for ln in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                if key_of(name):
                    res[key_of(name)] = cur
                cur = None
                continue
            t = ln.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.startswith(".LBB")):
                continue
            t = re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", t))
            cur.append(re.sub(r"\s+", " ", t))
    return res


def resources(path):
    res = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
        def get(pat):
            m = re.search(pat + r":\s*(\d+)", b)
            return m.group(1) if m else "?"
        k = key_of(b.split()[0])
        if k:
            v, sg, sc, oc = get(" VGPRs"), get("TotalSGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"Occupancy \[waves/SIMD\]")
            res[k] = f"VGPRs {v} SGPRs {sg} scratch {sc} occupancy {oc}"
    return res


def loops(body):
    lab = {ln[:-1]: i for i, ln in enumerate(body) if ln.startswith(".LBB_") and ln.endswith(":")}
    out = []
    for i, ln in enumerate(body):
        m = re.match(r"s_c?branch\w* (\.LBB_\d+)", ln)
        if m and lab.get(m.group(1), i) < i:
            out.append((lab[m.group(1)], i))
    return out


def main():
    pa, pr, na, nr = sys.argv[1:5]
    A, B, RA, RB = kernels(pa), kernels(na), resources(pr), resources(nr)
    print("kernels A:", sorted(A), "\nkernels B:", sorted(B))
    for k in sorted(A):
        a, b = A[k], B.get(k)
        print(f"\n== {k}\n  A {RA.get(k)} instructions {len(a)}\n  B {RB.get(k)} instructions {len(b) if b else None}")
        if b is None or a == b:
            print("  IDENTICAL" if b else "  MISSING in B")
            continue
        la, lb = loops(a), loops(b)
        nd = nin = 0
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
            if tag == "equal":
                continue
            inl = any(l0 <= i <= l1 for i in range(i1, max(i2, i1 + 1)) for l0, l1 in la) or \
                any(l0 <= j <= l1 for j in range(j1, max(j2, j1 + 1)) for l0, l1 in lb)
            nd += max(i2 - i1, j2 - j1)
            nin += max(i2 - i1, j2 - j1) if inl else 0
            print(f"  {tag} A[{i1}:{i2}] B[{j1}:{j2}] {'IN-LOOP' if inl else 'outside loops'}")
            for x in a[i1:i2]:
                print("    -", x)
            for x in b[j1:j2]:
                print("    +", x)
        print(f"  differing lines: {nd}, of them in loops: {nin}; loops A {la} B {lb}")


if __name__ == "__main__":
    main()
