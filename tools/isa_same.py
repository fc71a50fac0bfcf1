"""Per-kernel comparison of two hipcc -S listings (or directories / globs of them, e.g. after a file was split):
python tools/isa_same.py old.s new.s [substring]
Every kernel of the new listing(s) must have the old one's instruction stream (comments and whitespace stripped, the
.LBB<n>_ label prefix normalised) and .amdhsa_kernel descriptor; prints one line per kernel, a short diff where they
differ and the old kernels the new side lacks.  Exit status 1 if any kernel differs."""
import difflib
import glob
import os
import re
import sys


def kernels(path):
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else sorted(glob.glob(path))
    out = {}
    for f in files:
        s = open(f).read()
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", s, re.S):
            name = m.group(1)
            i = s.index("\n" + name + ":")
            body = []
            for line in s[i:s.index(".Lfunc_end", i)].split("\n"):
                line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
                if line:
                    body.append(" ".join(line.split()))
            desc = [" ".join(l.split()) for l in m.group(2).strip().split("\n")]
            out[name] = (body, desc)
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
flt = sys.argv[3] if len(sys.argv) > 3 else ""
bad = 0
for name in sorted(new):
    if flt not in name:
        continue
    if name not in old:
        print(f"NEW        {name}")
        continue
    same = [old[name][k] == new[name][k] for k in (0, 1)]
    print(f"{'same     ' if all(same) else 'DIFFERENT'}  {len(new[name][0]):6d} lines  {name}")
    if not all(same):
        bad += 1
        for k, what in ((0, "body"), (1, "descriptor")):
            if not same[k]:
                d = list(difflib.unified_diff(old[name][k], new[name][k], "old " + what, "new " + what, lineterm="", n=1))
                print("\n".join("    " + x for x in d[:40]))
for name in sorted(set(old) - set(new)):
    if flt in name:
        print(f"MISSING    {name}")
sys.exit(1 if bad else 0)
