#!/usr/bin/env python3
"""Compare the kernels of two builds of one csrc/*.hip unit instruction by instruction (profiles/attn_refactor.md and
profiles/gemm_epilogue_refactor.md are such comparisons). Make the two inputs with the flags of vdn/_build.py:

    hipcc <flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage csrc/attn.hip -o A.s 2> A.remarks
    python tools/asm_diff.py 'flash_attn2?_kernel' A.s A.remarks B.s B.remarks [--brief]

The first argument is a regular expression; a kernel takes part when its mangled name contains a match (the mangled name,
template arguments included, is also what pairs the kernels of the two builds). A kernel's text is its lines from the label to
.Lfunc_end with comments and directives stripped and block labels renumbered. A line is IN-LOOP when it lies between a block
label and a backward branch to that label. Prints, per kernel, registers / scratch / occupancy / instruction count of both
builds, every differing line (--brief: only their number), and the number of differing lines inside loops; then one summary
line: kernels in A, missing in B, new in B, identical, with other resources, with more VGPRs or instructions in B, with
differences inside loops."""
import difflib
import re
import sys


def kernels(path, pat):
    res, cur, name = {}, None, None
    for ln in open(path).read().split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            name, cur = m.group(1), []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                if pat.search(name):
                    res[name] = cur
                cur = None
                continue
            t = ln.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.startswith(".LBB")):
                continue
            t = re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", t))
            cur.append(re.sub(r"\s+", " ", t))
    return res


def resources(path, pat):
    res = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", open(path).read())[1:]:
        def get(p):
            m = re.search(p + r":\s*(\d+)", b)
            return int(m.group(1)) if m else -1
        k = b.split()[0]
        if pat.search(k):
            res[k] = (get(" VGPRs"), get("TotalSGPRs"), get(r"ScratchSize \[bytes/lane\]"), get(r"Occupancy \[waves/SIMD\]"))
    return res


def loops(body):
    lab = {ln[:-1]: i for i, ln in enumerate(body) if ln.startswith(".LBB_") and ln.endswith(":")}
    out = []
    for i, ln in enumerate(body):
        m = re.match(r"s_c?branch\w* (\.LBB_\d+)", ln)
        if m and lab.get(m.group(1), i) < i:
            out.append((lab[m.group(1)], i))
    return out


def fmt(r):
    return "VGPRs %d SGPRs %d scratch %d occupancy %d" % r if r else "?"


def main():
    brief = "--brief" in sys.argv
    pat, (pa, pr, na, nr) = re.compile(sys.argv[1]), [a for a in sys.argv[2:] if a != "--brief"]
    A, B, RA, RB = kernels(pa, pat), kernels(na, pat), resources(pr, pat), resources(nr, pat)
    missing, same, other_res, grew, in_loop = [k for k in A if k not in B], 0, 0, 0, 0
    for k in sorted(A):
        a, b = A[k], B.get(k)
        print(f"\n== {k}\n  A {fmt(RA.get(k))} instructions {len(a)}\n  B {fmt(RB.get(k))} instructions {len(b) if b else None}")
        if b is None:
            print("  MISSING in B")
            continue
        other_res += RA.get(k) != RB.get(k)
        grew += RB.get(k, (0,))[0] > RA.get(k, (0,))[0] or len(b) > len(a)
        if a == b:
            same += 1
            print("  IDENTICAL")
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
            if brief:
                continue
            print(f"  {tag} A[{i1}:{i2}] B[{j1}:{j2}] {'IN-LOOP' if inl else 'outside loops'}")
            for x in a[i1:i2]:
                print("    -", x)
            for x in b[j1:j2]:
                print("    +", x)
        in_loop += nin > 0
        print(f"  differing lines: {nd}, of them in loops: {nin}; loops A {la} B {lb}")
    print(f"\nSUMMARY kernels {len(A)} missing-in-B {len(missing)} new-in-B {len([k for k in B if k not in A])} identical {same} "
          f"other-resources {other_res} more-VGPRs-or-instructions {grew} with-in-loop-differences {in_loop}")


if __name__ == "__main__":
    main()
