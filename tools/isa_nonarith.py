#!/usr/bin/env python3
"""Static list of the VALU instructions of one extract_kernel instance that compute no feature: everything that
is not f64 / f32 / packed / transcendental arithmetic and not a float conversion (moves, compares, selects, DPP
moves, readlanes, integer and bit operations, lane-address arithmetic), by phase (the `;mgxmark` comments of a
-DMGX_MARKS build) and by source line (the `.loc` directives of -gline-tables-only).
Build the listing with:  tools/isa.sh OUT.s -DMGX_MARKS -gline-tables-only
usage: isa_nonarith.py FILE.s [N] [--lines] [--skip-fft]
  --lines     one row per (phase, opcode, source line) instead of per (phase, opcode)
  --skip-fft  leave out the segments between stage0_done and fft_done (run_passes)"""
import re
import sys
from collections import Counter, OrderedDict

ARITH = re.compile(r"v_(pk_)?(add|sub|subrev|mul|fma|fmac|mac|mad|max|min|rsq|rcp|sqrt|log|exp|frexp_mant|ldexp|fract|floor|"
                   r"trunc|rndne|ceil|div_fixup|div_fmas|div_scale|dot\w*)_(f64|f32|f16|legacy_f32)")


def klass(op, text):
    if not op.startswith("v_"):
        return None
    if op.startswith("v_cvt_f32_f64") or op.startswith("v_cvt_f64_f32"):
        return None  # the reference's roundings
    if "mfma" in op:
        return None
    if ARITH.match(op):
        # an arithmetic instruction that carries a DPP move does the move for free
        return None
    if "dpp" in op or "row_" in text or "quad_perm" in text or "wave_" in text:
        return "dpp"
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return "lane"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith(("v_mov", "v_accvgpr")):
        return "mov"
    if op.startswith("v_cvt"):
        return "cvt_other"
    return "int/bit"


def main():
    a = sys.argv[1:]
    path = a[0]
    n = int(a[1]) if len(a) > 1 and not a[1].startswith("-") else 1024
    by_line = "--lines" in a
    skip_fft = "--skip-fft" in a
    name = re.compile(r"_ZN3mgx12_GLOBAL__N_114extract_kernelILi%dELb1ELb0(ELb0)*EEEv[^:\s]*:" % n)
    lines = open(path).read().split("\n")
    start = [i for i, l in enumerate(lines) if name.match(l)][0]
    seg, loc, order = "prologue", 0, []
    counts = OrderedDict()
    totals = Counter()
    for l in lines[start + 1:]:
        if l.startswith(".Lfunc_end"):
            break
        s = l.strip()
        m = re.search(r";mgxmark (\w+)", s)
        if m:
            seg = m.group(1)
            continue
        m = re.match(r"\.loc\s+\d+\s+(\d+)", s)
        if m:
            loc = int(m.group(1))
            continue
        if not s or s.startswith(";") or s.startswith(".") or s.split(";")[0].rstrip().endswith(":"):
            continue
        op = s.split()[0]
        if not order or order[-1] != seg:
            order.append(seg)
        tag = "%03d %s" % (len(order) - 1, seg)
        if op.startswith("v_"):
            totals[tag] += 1
        k = klass(op, s)
        if k is None:
            continue
        key = (tag, k, op, loc if by_line else 0)
        counts[key] = counts.get(key, 0) + 1
    in_fft = False
    print("%-26s %-9s %-28s %6s %s" % ("segment (after mark)", "class", "opcode", "count", "line" if by_line else ""))
    seg_tot = Counter()
    for (tag, k, op, loc), c in sorted(counts.items(), key=lambda t: (t[0][0], t[0][1], t[0][2], t[0][3])):
        nm = tag.split(" ", 1)[1]
        in_fft = nm in ("stage0_done", "pass0_done", "xchg_begin", "xchg_end")
        if skip_fft and in_fft:
            continue
        seg_tot[tag] += c
        print("%-26s %-9s %-28s %6d %s" % (tag, k, op, c, loc if by_line else ""))
    print()
    print("%-26s %10s %10s" % ("segment", "non-arith", "VALU"))
    for tag in sorted(totals):
        print("%-26s %10d %10d" % (tag, seg_tot.get(tag, 0), totals[tag]))


if __name__ == "__main__":
    main()
