#!/usr/bin/env python3
"""Kernel by kernel comparison of two device assemblies of kernels.hip (tools/isa.sh OUT.s; for the parent
revision the same command in a `git archive` of it): the resource figures of the assembly's kernel metadata
(VGPRs, AGPRs, SGPRs, scratch, spills) and its "Occupancy" comment, and whether the instruction text is the same
-- comments stripped and the function number taken out of the branch labels (.LBB<function>_<block>), which
shifts when instances are added to the module. A kernel of OLD is matched with the kernel of NEW that has the
same template arguments followed by zeros only (a template parameter added since, defaulted to false); the
kernels of NEW that match none are listed after it, each beside the instance that differs in its last
argument alone.
usage: isa_compare.py OLD.s NEW.s"""
import re
import sys

KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count")


def parse(path):
    txt = open(path).read()
    meta, occ, text = {}, {}, {}
    for blk in re.split(r"\n  - \.agpr_count", txt)[1:]:
        blk = ".agpr_count" + blk
        d = {k: re.search(re.escape(k) + r":\s*(\S+)", blk).group(1) for k in KEYS + (".kernarg_segment_size", ".name")}
        meta[d[".name"]] = d
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\.Lfunc_end\d+:", txt, re.S):
        text[m.group(1)] = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", line)).strip()
                            for line in m.group(2).split("\n") if re.match(r"\t[a-z]", line)]
    for m in re.finditer(r"\t\.size\t(_Z\w+), \.Lfunc_end", txt):
        o = re.search(r"; Occupancy: (\d+)", txt[m.end():m.end() + 4000])
        occ[m.group(1)] = o.group(1) if o else "?"
    return meta, occ, text


def ident(name):
    """(kernel, template arguments) of a mangled name."""
    m = re.search(r"\d+(extract_kernel|lds_image_kernel)I(.*?)EEv", name)
    if not m:
        m2 = re.search(r"\d+([a-z_]+_kernel)", name)
        return (m2.group(1) if m2 else name), ()
    return m.group(1), tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2) + "E"))


def show(idn):
    return idn[0] + ("<%s>" % ", ".join(str(v) for v in idn[1]) if idn[1] else "")


def row(meta, occ, k):
    d = meta[k]
    return " | ".join([d[".vgpr_count"], d[".agpr_count"], d[".sgpr_count"], d[".private_segment_fixed_size"], occ.get(k, "?"),
                       d[".vgpr_spill_count"], d[".sgpr_spill_count"]])


def main():
    (pm, po, pt), (nm, no, nt) = parse(sys.argv[1]), parse(sys.argv[2])
    new_by = {ident(k): k for k in nm}
    print("kernel | VGPRs | AGPRs | SGPRs | scratch B/lane | waves/SIMD | VGPR spills | SGPR spills | kernel arguments, bytes with "
          "the hidden ones   (old -> new where a figure differs)")
    moved = same = 0
    matched = set()
    for k in pm:
        name, args = ident(k)
        # (the same mangled name first: the instances of a kernel this file's ident() does not tell apart)
        nk = k if k in nm else next((q for i, q in new_by.items() if i[0] == name and i[1][:len(args)] == args and not any(i[1][len(args):])), None)
        if nk is None:
            print("%s | %s | (not in the new assembly)" % (show((name, args)), row(pm, po, k)))
            continue
        matched.add(nk)
        a = row(pm, po, k) + " | " + pm[k][".kernarg_segment_size"]
        b = row(nm, no, nk) + " | " + nm[nk][".kernarg_segment_size"]
        moved += a != b
        same += k in pt and pt[k] == nt.get(nk)
        print("%s | %s%s" % (show((name, args)), a, "" if a == b else " -> " + b))
    print("\nexisting kernels: %d; kernels with a figure that moved: %d; kernels whose instruction text is identical, "
          "instruction for instruction: %d" % (len(pm), moved, same))
    rest = [k for k in nm if k not in matched]
    if rest:
        print("\nkernels of the new assembly alone (instructions; beside them the instance that differs in the last argument)")
    for k in rest:
        name, args = ident(k)
        base = new_by.get((name, args[:-1] + (0,))) if args else None
        print("%s | %s | %s | %d instructions%s" % (show((name, args)), row(nm, no, k), nm[k][".kernarg_segment_size"], len(nt.get(k, [])),
                                                      ", %d without" % len(nt[base]) if base in nt else ""))


if __name__ == "__main__":
    main()
