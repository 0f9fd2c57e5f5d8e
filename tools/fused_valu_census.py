#!/usr/bin/env python3
"""Static instruction census of the fused pixel launch (compile-only, no GPU, changes no file of the tree).

Builds the gfx950 device assembly of csrc/fitter_kernels.hip with the flags the Makefile compiles it with (taken from
`make -n`, so a flag scoped to that file is picked up) plus -gline-tables-only, and reports for one instantiation of
k_fit_pixels_fused (default <0,4,5>: ALL, 4 anchors, 5 waves per SIMD):
  * VGPRs, AGPRs, SGPRs, scratch (spill) bytes, code bytes, occupancy, as the compiler states them;
  * per source region, the VALU instructions by opcode class, and the SALU / LDS / memory instruction counts.

Regions are line ranges of fitter_kernels.hip found from the source's own anchors (the lambdas of node_body, pixel_body,
the branch of sums that walks a batch slot by slot). An instruction belongs to the region of the .loc in force where it
stands; the .loc's comment carries the chain of inlined call sites, and the innermost fitter_kernels.hip line of the
chain that lies in a named region decides (so div_rn, face_test, matvec3 and the functions of pixel_terms.hpp count with
their caller). A compiler
generated instruction without a line keeps the region before it. The counts are static: a loop body counts once, both
sides of a branch count.

--check exits non-zero unless <0,4,5> keeps its 5 waves per SIMD (at most 96 VGPRs, at most 8 bytes of scratch) and
<0,4,4> has no scratch.

usage: fused_valu_census.py [--csrc DIR] [--kernel MODE,MAXK,WPE] [--also MODE,MAXK,WPE ...] [--keep-asm FILE] [--check]
"""
import argparse
import collections
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = "fitter_kernels.hip"

REGIONS = ["prologue", "pass 1", "grouping", "gather", "jacobians", "sums fast path", "sums slot-serial"]
CLASSES = ["v_mov", "v_cndmask", "packed", "fp64", "convert", "address", "cross-lane", "rest"]

ADDRESS_OPS = {"v_mad_u64_u32", "v_mad_i64_i32", "v_lshlrev_b64", "v_lshl_add_u64", "v_ashrrev_i32", "v_add_co_u32",
               "v_addc_co_u32", "v_add_co_ci_u32"}


def compile_command(csrc):
    """The Makefile's own command line for fitter_kernels.o, as a list (without -c / -o)."""
    out = subprocess.check_output(["make", "-n", "-B", "-C", csrc, "build/fitter_kernels.o"], text=True)
    line = [l for l in out.splitlines() if SRC in l and "hipcc" in l][-1]
    args = shlex.split(line)
    cmd, skip = [], False
    for a in args:
        if skip:
            skip = False
            continue
        if a == "-o":
            skip = True
            continue
        if a == "-c" or a == SRC:
            continue
        cmd.append(a)
    return cmd


def build_asm(csrc, path):
    cmd = compile_command(csrc) + ["--cuda-device-only", "-gline-tables-only", "-Wno-pass-failed", "-S", SRC, "-o", path]
    subprocess.check_call(cmd, cwd=csrc)
    return cmd


def source_regions(csrc):
    """[(first line, last line, region)] of fitter_kernels.hip, from the source's anchors."""
    lines = open(os.path.join(csrc, SRC)).read().splitlines()

    def find(pat, start=0):
        rx = re.compile(pat)
        for i in range(start, len(lines)):
            if rx.search(lines[i]):
                return i + 1
        raise SystemExit(f"census: anchor not found in {SRC}: {pat}")

    p1 = find(r"void pixel_body\(")
    p1_end = find(r"^}", p1)
    wmin = find(r"int wave_min_i32\(")
    wmin_end = find(r"^}", wmin)
    grp = find(r"auto group = \[&\]")
    gat = find(r"auto gather = \[&\]", grp)
    jac = find(r"auto jacobians = \[&\]", gat)
    sms = find(r"auto sums = \[&\]", jac)
    serial = find(r"^\t+} else {\s*$", find(r"__all\(n_first == n_last\)", sms))
    sync = find(r"auto wave_sync = \[&\]", sms)
    # the ballot-free declarations between group and gather (registers of gather) count as gather
    gat_decl = find(r"^\t};", grp) + 1
    return [(p1, p1_end, "pass 1"), (wmin, wmin_end, "grouping"), (grp, gat_decl - 1, "grouping"), (gat_decl, jac - 1, "gather"),
            (jac, sms - 1, "jacobians"), (sms, serial - 1, "sums fast path"), (serial, sync - 1, "sums slot-serial")]


def classify(op):
    if op.startswith(("v_mov_b", "v_accvgpr_", "v_swap_b")):
        return "v_mov"
    if op.startswith("v_cndmask"):
        return "v_cndmask"
    if op.startswith("v_pk_"):
        return "packed"
    if op.startswith("v_cvt_"):
        return "convert"
    if re.search(r"_f64(_|$)", op):
        return "fp64"
    base = re.sub(r"_(e32|e64|dpp|sdwa|e64_dpp)$", "", op)
    if base in ADDRESS_OPS:
        return "address"
    if base.startswith(("v_readlane", "v_readfirstlane", "v_writelane", "v_mbcnt", "v_permlane")) or op.endswith("_dpp"):
        return "cross-lane"
    return "rest"


def kernel_symbol(spec):
    mode, maxk, wpe = spec
    return f"_ZN4nnrt18k_fit_pixels_fusedILi{mode}ELi{maxk}ELi{wpe}EEEvNS_12FitPixelArgsE"


def census(asm_path, csrc, spec):
    sym = kernel_symbol(spec)
    text = open(asm_path).read().splitlines()
    start = next((i for i, l in enumerate(text) if l.startswith(sym + ":")), None)
    if start is None:
        raise SystemExit(f"census: {sym} not in the assembly")
    regions = source_regions(csrc)

    def region_of(line):
        for a, b, r in regions:
            if a <= line <= b:
                return r
        return "prologue"

    valu = {r: collections.Counter() for r in REGIONS}
    other = {r: collections.Counter() for r in REGIONS}
    sites = collections.Counter()
    cur = "prologue"
    info = {}
    i = start + 1
    while i < len(text):
        l = text[i].strip()
        i += 1
        if l.startswith(".Lfunc_end"):
            break
        if l.startswith(".loc"):
            # "; file:line:col @[ caller:line:col @[ ... ] ]": the innermost frame inside a named region decides
            hits = [region_of(int(n)) for f, n in re.findall(r"([^\s\[]+):(\d+):\d+", l.partition(";")[2])
                    if os.path.basename(f) == SRC and int(n) > 0]
            if hits:
                cur = next((r for r in hits if r != "prologue"), "prologue")
            continue
        if not l or l[0] in ".;" or l.endswith(":"):
            continue
        op = l.split()[0]
        if op.startswith("v_"):
            valu[cur][classify(op)] += 1
        elif op.startswith("s_"):
            other[cur]["salu" if not op.startswith(("s_load", "s_buffer_load", "s_waitcnt", "s_nop")) else
                       ("smem" if op.startswith(("s_load", "s_buffer_load")) else "wait/nop")] += 1
        elif op.startswith("ds_"):
            other[cur]["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            other[cur]["vmem"] += 1
            if op.startswith("global_atomic"):
                sites["global_atomic"] += 1
            elif op.startswith("global_store"):
                sites["global_store"] += 1
            elif op.startswith("scratch_"):
                sites["scratch access"] += 1
    for l in text[i:i + 80]:
        m = re.match(r";\s*(NumVgprs|NumAgprs|TotalNumSgprs|ScratchSize|Occupancy|codeLenInByte|LDSByteSize)\s*[:=]\s*(\d+)", l.strip())
        if m and m.group(1) not in info:
            info[m.group(1)] = int(m.group(2))
    return valu, other, sites, info


def report(spec, valu, other, sites, info, out):
    name = "k_fit_pixels_fused<%d,%d,%d>" % spec
    out.write(f"== {name}\n")
    out.write("resources: VGPRs %d, AGPRs %d, SGPRs %d, scratch %d bytes, code %d bytes, LDS %d bytes, occupancy %d waves/SIMD\n" % tuple(
        info.get(k, -1) for k in ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "codeLenInByte", "LDSByteSize", "Occupancy")))
    out.write("sites: " + ", ".join(f"{k} {v}" for k, v in sorted(sites.items())) + "\n")
    head = f"{'region':<18}" + "".join(f"{c:>11}" for c in CLASSES) + f"{'VALU':>8}" + "".join(f"{c:>9}" for c in ("salu", "lds", "vmem", "smem"))
    out.write(head + "\n")
    total = collections.Counter()
    tother = collections.Counter()
    for r in REGIONS:
        n = sum(valu[r].values())
        out.write(f"{r:<18}" + "".join(f"{valu[r][c]:>11}" for c in CLASSES) + f"{n:>8}" +
                  "".join(f"{other[r][c]:>9}" for c in ("salu", "lds", "vmem", "smem")) + "\n")
        total.update(valu[r])
        tother.update(other[r])
    n = sum(total.values())
    out.write(f"{'total':<18}" + "".join(f"{total[c]:>11}" for c in CLASSES) + f"{n:>8}" +
              "".join(f"{tother[c]:>9}" for c in ("salu", "lds", "vmem", "smem")) + "\n")
    out.write(f"{'share of VALU':<18}" + "".join(f"{100.0 * total[c] / max(n, 1):>10.1f}%" for c in CLASSES) + "\n\n")


def parse_spec(s):
    t = tuple(int(x) for x in s.split(","))
    if len(t) != 3:
        raise argparse.ArgumentTypeError("MODE,MAXK,WPE")
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=os.path.join(ROOT, "dynamicfuion_python_amd", "csrc"))
    ap.add_argument("--kernel", type=parse_spec, default=(0, 4, 5))
    ap.add_argument("--also", type=parse_spec, nargs="*", default=[(0, 4, 4)], help="further instantiations (default: <0,4,4>)")
    ap.add_argument("--keep-asm", default=None, help="keep the assembly in this file")
    ap.add_argument("--check", action="store_true", help="fail unless the register and scratch budgets hold")
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.abspath(a.keep_asm) if a.keep_asm else os.path.join(tmp, "fitter_kernels.s")
        cmd = build_asm(csrc, asm)
        sys.stdout.write("flags: " + " ".join(c for c in cmd[1:] if c not in ("-S", SRC, "-o", asm)) + "\n\n")
        for spec in [a.kernel] + [s for s in a.also if s != a.kernel]:
            report(spec, *census(asm, csrc, spec), sys.stdout)
        if a.check:
            bad = []
            i5, i4 = census(asm, csrc, (0, 4, 5))[3], census(asm, csrc, (0, 4, 4))[3]
            if i5["NumVgprs"] > 96 or i5["ScratchSize"] > 8:
                bad.append("<0,4,5>: %d VGPRs, %d bytes of scratch (budget 96, 8)" % (i5["NumVgprs"], i5["ScratchSize"]))
            if i4["ScratchSize"] > 0:
                bad.append("<0,4,4>: %d bytes of scratch (budget 0)" % i4["ScratchSize"])
            if bad:
                raise SystemExit("census --check: " + "; ".join(bad))


if __name__ == "__main__":
    main()
