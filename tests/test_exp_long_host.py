"""K1's long exp table and short weight chain on the CPU: tools/exp_long_check.cpp, built with AddressSanitizer and UBSan as
a program of its own, walks the table's layout, compares the full and the short chain bit for bit wherever the short one may
run (every table boundary and its neighbours, 10^7 seeded values per gamma^2), and checks the limit and the bound
(cvx_proj_amd/csrc/apap_exp_long.h).  The table it checks is kExp2Tab as apap_kernels.hip spells it.

The body test: that the two settings of the switch give the same bits (tests/test_gpu_k1_short_chain.py) says nothing unless
the short body exists and is the one a proved chunk runs.  test_the_compiled_kernels_hold_the_short_body cross-compiles
apap_kernels.hip to gfx950 assembly with the Makefile's flags (no GPU needed) and reads the chunk loops off it."""
import os
import re
import subprocess
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exp_long_check_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "exp_long_check")
    csrc = os.path.join(ROOT, "cvx_proj_amd", "csrc")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-ffp-contract=off", "-I", csrc, os.path.join(ROOT, "tools", "exp_long_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    r = subprocess.run([exe, os.path.join(csrc, "apap_kernels.hip")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"exp_long_check: ok \((\d+) entries, (\d+) chain pairs equal, (\d+) refused, (\d+) bounded distances\)", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 768 and int(m.group(2)) >= 10 ** 7 and int(m.group(3)) > 0 and int(m.group(4)) > 0
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_switch_binding_and_budget_agree():
    """The short chain's switch is declared, bound and named for Context() beside the option table, which keeps its count; its
    default and range need no GPU; and the table's length is what the budget in DESIGN.md counts (four blocks of 40 960 bytes in
    a CU's 160 KiB)."""
    import ctypes
    import pytest
    from cvx_proj_amd import _native as native
    text = open(os.path.join(ROOT, "include", "apap_hip.h")).read()
    for name in ("apap_ctx_set_short_chain", "apap_ctx_get_short_chain"):
        assert re.search(rf"\bint {name}\(", text) and name in native.SIGNATURES
    ctx = native.Context(short_chain=0)
    assert ctx.get("short_chain") == 0 and ctx.set("short_chain", 1).get("short_chain") == 1
    with pytest.raises(ValueError):
        ctx.set("short_chain", 2)
    ctx.close()
    v = ctypes.c_int(-1)
    assert native.lib().apap_ctx_get_short_chain(None, ctypes.byref(v)) == native.OK and v.value == 1
    long_h = open(os.path.join(ROOT, "cvx_proj_amd", "csrc", "apap_exp_long.h")).read()
    entries = int(re.search(r"constexpr int kExpLong = (\d+);", long_h).group(1))
    assert entries % 64 == 0 and 2 * 64 * 256 + entries * 8 + 2 * 64 * 2 * 8 <= 40960


def _table_chain_loops(path):
    """{kernel: [Counter of opcodes]} of every innermost loop that holds the table-driven weight chain (its v_fract_f64)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import asm_count
    finally:
        sys.path.pop(0)
    labels = {}
    out = {}
    for name, ins in asm_count.kernels(path, labels).items():
        ops = [i.split()[0] for i in ins]
        back = [(labels[name][i.split()[-1]], k) for k, i in enumerate(ins)
                if ops[k].startswith(("s_cbranch", "s_branch")) and labels[name].get(i.split()[-1], k + 1) <= k]
        inner = [f for f in back if not any(g != f and f[0] <= g[0] and g[1] <= f[1] for g in back)]
        loops = [Counter(ops[t:k + 1]) for t, k in inner]
        out[name] = [c for c in loops if any(o.startswith("v_fract_f64") for o in c)]
    return out


def test_the_compiled_kernels_hold_the_short_body(tmp_path):
    """In the code the library is built from: the two float64-weight instances of k_assemble_mfma hold, beside every chunk loop
    with the full chain (one v_ldexp_f64 and one v_max_f64 per weight), a chunk loop with the short one - no v_ldexp_f64, no
    mask, no arithmetic shift, no s_and_saveexec, and exactly the vote's two v_max_f64 - that is at least 2 vector instructions
    per weight shorter, vote included; the partial-chunk loops likewise (4 per weight, no vote).  No other kernel of the source
    - k_assemble_valu, k_assemble_mfma4, k_solve_small, the float32-weight instance - holds a table chain without its ldexp
    and its clamp."""
    csrc = os.path.join(ROOT, "cvx_proj_amd", "csrc")
    make = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = str(tmp_path / "apap_kernels.gfx950.s")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", *flags, "-S", "--cuda-device-only", "apap_kernels.hip", "-o", asm], cwd=csrc,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    loops = _table_chain_loops(asm)
    count = lambda c, prefix: sum(n for o, n in c.items() if o.startswith(prefix))     # noqa: E731
    valu = lambda c: count(c, "v_") - count(c, "v_mfma")                               # noqa: E731
    short_kernels = [k for k in loops if "k_assemble_mfmaILi4ELb0ELb0E" in k or "k_assemble_mfmaILi4ELb1ELb0E" in k]
    assert len(short_kernels) == 2, sorted(loops)
    assert sum("k_assemble_mfmaILi4ELb1ELb1E" in k for k in loops) == 1 and sum("k_assemble_valu" in k for k in loops) == 1
    for name, ls in loops.items():
        if name in short_kernels:
            continue
        if "k_assemble_mfmaILi4ELb1ELb1E" in name:
            assert not ls, "the float32-weight form has no table chain"
        for c in ls:        # the full chain, whole
            assert count(c, "v_ldexp_f64") == count(c, "v_fract_f64") == count(c, "v_max_f64"), (name, dict(c))
    for name in short_kernels:
        ls = loops[name]
        full = [c for c in ls if count(c, "v_ldexp_f64")]
        short = [c for c in ls if not count(c, "v_ldexp_f64")]
        assert len(full) + len(short) == len(ls) and full and short
        for c in full:
            assert count(c, "v_ldexp_f64") == count(c, "v_fract_f64") == count(c, "v_max_f64") and not count(c, "s_and_saveexec"), dict(c)
        for c in short:
            chunk = c["s_barrier"] == 1
            assert count(c, "v_max_f64") == (2 if chunk else 0), (name, dict(c))
            assert not count(c, "s_and_saveexec") and not count(c, "v_and_b32") and not count(c, "v_ashrrev_i32"), (name, dict(c))
            assert count(c, "v_cvt_i32_f64") == count(c, "v_fract_f64"), (name, dict(c))
        # the forms pair up: plain grid / levelled / paired, sharing the row term or not, whole chunks and the partial one
        for chunk, saving in ((True, 2), (False, 4)):
            forms = lambda group: sorted({(count(c, "v_mfma"), count(c, "v_fract_f64"), valu(c))                # noqa: E731
                                          for c in group if (c["s_barrier"] == 1) == chunk})
            f, s = forms(full), forms(short)
            assert len(f) == len(s) == 4 and sum((c["s_barrier"] == 1) == chunk for c in full) == 6, (name, chunk, f, s)
            for (mf, wf, vf), (ms, ws, vs) in zip(f, s):
                assert (mf, wf) == (ms, ws) and vs <= vf - saving * wf, (name, chunk, f, s)
            print(name[:48], "whole chunks" if chunk else "partial chunk", "full", f, "short", s)
