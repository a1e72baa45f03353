"""Are two device-assembly files the same code up to the order of their symbols?

    hipcc --offload-arch=gfx950 <build.py's flags> --cuda-device-only -S csrc/spade.hip -o a.s      (at two commits)
    python tools/device_asm_diff.py a.s b.s

A host-only change reorders template instantiations, which renumbers hipcc's local labels (.LBB<function>_<block>) and moves whole
functions, kernel descriptors and metadata entries.  Labels lose their function number, the text is cut into one piece per function /
descriptor / metadata entry, and the sorted pieces are compared.  The compilation unit's id (__hip_cuid_<hash of the source>) is
blanked: it differs whenever the source text does.  Exit status 0: same code."""
import difflib
import re
import sys


def pieces(path):
    t = open(path).read()
    t = re.sub(r"BB\d+_(\d+)", r"BB_\1", t)
    t = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", t)
    t = re.sub(r"\.Ltmp\d+", ".Ltmp", t)
    t = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", t)
    out, cur = [], []
    for line in t.split("\n"):
        if re.match(r"^\t\.(protected|section|text|weak|globl)\b", line) or re.match(r"^  - \.agpr_count", line):
            out.append("\n".join(cur)); cur = []
        cur.append(line)
    out.append("\n".join(cur))
    return sorted(out)


def main(a_path, b_path):
    a, b = pieces(a_path), pieces(b_path)
    sa, sb = set(a), set(b)
    only_a = {p.split("\n")[0]: p for p in a if p not in sb}
    only_b = {p.split("\n")[0]: p for p in b if p not in sa}
    print("%d / %d pieces; %d / %d without a twin" % (len(a), len(b), len(only_a), len(only_b)))
    for k in sorted(set(only_a) | set(only_b)):
        d = [l for l in difflib.unified_diff(only_a.get(k, "").split("\n"), only_b.get(k, "").split("\n"), lineterm="", n=0)
             if not l.startswith(("---", "+++", "@@"))]
        print("%4d differing lines: %s" % (len(d), k.strip()[:140]))
    same = a == b
    print("same code up to symbol order" if same else "DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
