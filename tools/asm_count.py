#!/usr/bin/env python3
"""Static instruction mix of kernels in a device assembly file of `make -C cvx_proj_amd/csrc asm`: by default
   cvx_proj_amd/csrc/apap_kernels.gfx950.s, or the .s file given as the first argument.
   tools/asm_count.py k_warp_fastILb0ELi4 k_warp_rowsILb0ELi4
   tools/asm_count.py cvx_proj_amd/csrc/apap_panorama.gfx950.s k_panoramaILi0

   Compare mode: two .s files of the same source from two trees, one line per kernel.
   tools/asm_count.py --compare old/apap_kernels.gfx950.s new/apap_kernels.gfx950.s [name ...]
   Directives, comments, labels and symbols outside the kernels (__hip_cuid_...) are ignored; the number of a basic-block
   label (.LBB12_3: 12 is the function's position in the file) is not part of an instruction.  Per kernel: `identical`, or
   the instruction counts of both, whether the opcode sequences are equal, the index of the first difference and of the last
   one (counted from the end, -1 = the last instruction), and `loop equal` / `loop DIFFERS`: the opcode sequence of the
   steady state.  The steady state is taken from the code itself: every backward branch whose body holds an MFMA (the VALU
   K1 has none: v_rsq_f64, the head of its weight chain) closes a loop; inside the outermost such body the sequence runs
   from the first instruction of a weight chain (v_rsq_f64, v_sqrt_f32) or MFMA to the last s_barrier (the one that closes
   the chunk loop), or to the closing branch where the loop has no barrier.  Prefetch loads at the loop's top are outside it.

   Loop table: every loop of a kernel that holds an MFMA, in file order, one line each.
   tools/asm_count.py --loops [file.s] k_assemble_mfmaILi4ELb0ELb0E
   Instructions from the loop's label to its backward branch, and of its largest basic block (the unrolled steps), with the
   MFMAs, LDS reads and float64 adds and fused multiply-adds inside.  k_assemble_mfma with float64 weights has twelve: per body
   (plain grid, levelled, paired) the chunk loop and the partial-chunk loop of a block that forms the row term in every lane,
   then the two of a block that shares it (2 v_add_f64 and 1 FMA fewer per weight chain, one ds_read_b64 more per group)."""
import os
import re
import sys
from collections import Counter


def kernels(path, labels=None):
    """{mangled name: [instruction text without comment, block-label numbers normalised]} in file order; `labels`, when
    given, receives {mangled name: {label: index of the instruction that follows it}}"""
    out, cur, lab = {}, None, None
    for l in open(path).read().split("\n"):
        if l.startswith("_Z") and ": " in l and "@" in l:
            cur = out.setdefault(l.split(":")[0], [])
            lab = {}
            if labels is not None:
                labels[l.split(":")[0]] = lab
            continue
        t = re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip())
        if t.startswith(".Lfunc_end"):
            cur = None
        if cur is not None and t.endswith(":"):
            lab[t[:-1]] = len(cur)
        if cur is None or not t or t.startswith((".", "//")) or t.endswith(":"):
            continue
        cur.append(" ".join(t.split()))
    return out


def steady(ins, lab):
    ops = [i.split()[0] for i in ins]
    anchor = "v_mfma" if any(o.startswith("v_mfma") for o in ops) else "v_rsq_f64"
    lo, hi = None, None
    for k, i in enumerate(ins):
        if ops[k].startswith(("s_cbranch", "s_branch")) and lab.get(i.split()[-1], k + 1) <= k:
            t = lab[i.split()[-1]]
            if any(o.startswith(anchor) for o in ops[t:k]):
                lo, hi = min(t, lo if lo is not None else t), max(k, hi or k)
    if lo is None:
        return []
    head = next(k for k in range(lo, hi + 1) if ops[k].startswith(("v_rsq_f64", "v_sqrt_f32", "v_mfma")))
    bars = [k for k in range(head, hi + 1) if ops[k] == "s_barrier"]
    return ops[head:(bars[-1] if bars else hi) + 1]


def loops(path, names):
    lab = {}
    for name, ins in kernels(path, lab).items():
        if names and not any(n in name for n in names):
            continue
        ops = [i.split()[0] for i in ins]
        starts = sorted(set(lab[name].values()))
        found = []
        for k, i in enumerate(ins):
            if ops[k].startswith(("s_cbranch", "s_branch")) and lab[name].get(i.split()[-1], k + 1) <= k:
                t = lab[name][i.split()[-1]]
                if any(o.startswith("v_mfma") for o in ops[t:k]):
                    found.append((t, k))
        found = [f for f in found if not any(g != f and f[0] <= g[0] and g[1] <= f[1] for g in found)]     # innermost
        print(f"{name}: {len(ins)} instructions, {len(found)} loops with MFMAs")
        for t, k in found:
            cuts = [t] + [b for b in starts if t < b <= k] + [k + 1]
            big = max(zip(cuts, cuts[1:]), key=lambda ab: ab[1] - ab[0])
            body = ops[big[0]:big[1]]
            c = Counter(ops[t:k + 1])
            grp = lambda pre: sum(n for o, n in c.items() if o.startswith(pre))  # noqa: E731
            print(f"    {k + 1 - t:5d} instructions ({len(body)} in the largest block): v_mfma {grp('v_mfma')}, ds_read {grp('ds_read')}, "
                  f"v_add_f64 {grp('v_add_f64')}, FMA f64 {grp(('v_fma_f64', 'v_fmac_f64'))}, VALU {grp('v_') - grp('v_mfma')}, "
                  f"s_barrier {c['s_barrier']}")


def compare(path_a, path_b, names):
    la, lb = {}, {}
    a, b = kernels(path_a, la), kernels(path_b, lb)
    same = 0
    for k in list(a) + [k for k in b if k not in a]:
        if names and not any(n in k for n in names):
            continue
        if k not in a or k not in b:
            print(f"{k}: only in {path_a if k in a else path_b}")
            continue
        x, y = a[k], b[k]
        if x == y:
            same += 1
            print(f"{k}: identical ({len(x)} instructions)")
            continue
        ox, oy = [i.split()[0] for i in x], [i.split()[0] for i in y]
        first = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        last = next((i for i, (p, q) in enumerate(zip(reversed(x), reversed(y))) if p != q), min(len(x), len(y)))
        print(f"{k}: {len(x)} -> {len(y)} instructions, opcode sequence {'equal' if ox == oy else 'differs'}, "
              f"first difference at {first}, last at -{last + 1}, loop {'equal' if steady(x, la[k]) == steady(y, lb[k]) else 'DIFFERS'} "
              f"({len(steady(x, la[k]))} -> {len(steady(y, lb[k]))} opcodes)")
    print(f"{same} kernels identical")


def mix(path, names):
    lines = open(path).read().split("\n")

    def func(name):
        start = [i for i, l in enumerate(lines) if l.startswith("_ZN") and name in l.split(":")[0] and ": " in l][0]
        out = []
        for l in lines[start + 1:]:
            t = l.strip()
            if t.startswith(".Lfunc_end"):
                break
            if not t or t.startswith((".", ";", "//")) or t.split(";")[0].strip().endswith(":"):
                continue
            out.append(t.split()[0])
        return out

    for name in names:
        c = Counter(func(name))
        tot = sum(c.values())
        grp = lambda pre: sum(n for k, n in c.items() if k.startswith(pre))  # noqa: E731
        print(f"{name}: {tot} instructions, VALU {grp('v_')}, SALU {grp('s_')}, vector memory {grp(('global_', 'buffer_', 'flat_'))}, "
              f"f64 {sum(n for k, n in c.items() if 'f64' in k)}")
        print("   ", ", ".join(f"{k} {n}" for k, n in c.most_common(28)))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--compare":
        compare(args[1], args[2], args[3:])
    elif args and args[0] == "--loops":
        args.pop(0)
        default = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvx_proj_amd/csrc/apap_kernels.gfx950.s")
        loops(args.pop(0) if args and args[0].endswith(".s") else default, args)
    else:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cvx_proj_amd/csrc/apap_kernels.gfx950.s")
        if args and args[0].endswith(".s"):
            path = args.pop(0)
        mix(path, args)
