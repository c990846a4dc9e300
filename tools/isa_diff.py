#!/usr/bin/env python3
"""isa_diff.py A B [file.hip ...] -- did a change to spaln_amd/csrc change the generated code?  (host only)

A and B are two checkouts.  Every .hip of the Makefile's HIPSRC (or the ones named) is compiled device-only to
assembly with the Makefile's flags, its per-file EXTRA included; comment lines and the CUID symbol are dropped; then, per
kernel: identical, or the size of the diff and both sides' register / LDS / scratch / spill figures, and whether the
compiler's occupancy remarks are the same set.  Nothing is kept between runs.  Exit status 1 when a kernel differs."""
import difflib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROWS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count")

def recipe(csrc):
    mk = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = lambda name: re.search(r"^%s\s*\??=\s*(.*)$" % name, mk, re.M).group(1)
    flags = var("FLAGS").replace("$(ARCH)", var("ARCH")).split()
    extra = {m.group(1) + ".hip": m.group(2).split() for m in re.finditer(r"^\$\(OBJDIR\)/(\w+)\.o: EXTRA = (.*)$", mk, re.M)}
    return os.environ.get("HIPCC", var("HIPCC")), flags, extra, [s for s in var("HIPSRC").split() if s.endswith(".hip")]

def assemble(root, only, out):
    """{file: (kernels, occupancy remarks)} of one checkout"""
    csrc = os.path.join(root, "spaln_amd", "csrc")
    hipcc, flags, extra, srcs = recipe(csrc)

    def one(src):
        dst = os.path.join(out, src[:-4] + ".s")
        r = subprocess.run([hipcc, *flags, *extra.get(src, []), "--cuda-device-only", "-S", "-o", dst, os.path.join(csrc, src)],
                           capture_output=True, text=True)
        if r.returncode:
            sys.exit("%s: %s\n%s" % (root, src, r.stderr))
        return src, (kernels(open(dst).read()), sorted(re.findall(r"warning: (.*) \[-Wpass-failed\]", r.stderr)))

    with ThreadPoolExecutor(16) as pool:
        return dict(pool.map(one, [s for s in srcs if not only or s in only]))

def kernels(asm):
    lines = [l for l in asm.splitlines() if not l.lstrip().startswith(";") and "__hip_cuid_" not in l]
    lines = [re.sub(r"\s*;.*$", "", l) for l in lines]
    res = {}
    meta = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", "\n".join(lines), re.M | re.S)
    for m in re.finditer(r"^  - .*?(?=^  - |\Z)", meta.group(1) if meta else "", re.M | re.S):      # the metadata's kernel entries
        name = re.search(r"^    \.name:\s*(\S+)", m.group(0), re.M).group(1)
        res[name] = {k: int(re.search(r"^    %s:\s*(\d+)" % re.escape(k), m.group(0), re.M).group(1)) for k in ROWS}
    body = {}
    for name in res:
        i = lines.index(name + ":")
        j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body[name] = lines[i:j]
    return {n: (body[n], res[n]) for n in res}

def main():
    a, b, only = sys.argv[1], sys.argv[2], sys.argv[3:]
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        fa, fb = assemble(a, only, ta), assemble(b, only, tb)
    bad = len(set(fa) ^ set(fb))
    for src in sorted(set(fa) ^ set(fb)):
        print("%-22s only in %s" % (src, "A" if src in fa else "B"))
    for src in [f for f in fa if f in fb]:
        (ka, wa), (kb, wb) = fa[src], fb[src]
        diffs = {n: sum(1 for l in difflib.unified_diff(ka[n][0], kb[n][0], n=0, lineterm="") if l[:1] in "+-" and l[:3] not in ("+++", "---"))
                 for n in ka if n in kb}
        changed = [n for n in diffs if diffs[n]] + sorted(set(ka) ^ set(kb))
        print("%-22s %3d kernels, %s" % (src, len(ka), "all identical" if not changed else "%d differ" % len(changed)))
        for n in changed:
            bad += 1
            if n not in diffs:
                print("  %s: only in %s" % (n, "A" if n in ka else "B"))
                continue
            print("  %s: %d diff lines" % (n, diffs[n]))
            for side, k in (("A", ka), ("B", kb)):
                print("    %s  " % side + "  ".join("%s %d" % (r, k[n][1][r]) for r in ROWS))
        if wa != wb:
            print("  compiler remarks differ:\n" + "\n".join(["    A  " + w for w in wa] + ["    B  " + w for w in wb]))
        elif wa:
            print("  %d occupancy remarks, the same on both sides" % len(wa))
    return 1 if bad else 0

if __name__ == "__main__":
    sys.exit(main())
