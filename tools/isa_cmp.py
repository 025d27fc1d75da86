"""Compare the instruction streams of every kernel symbol of two compiler listings
(hipcc -S --cuda-device-only), labels, comments and directives stripped: a refactor that
should move no instruction shows "identical" for each.  No GPU.
    python tools/isa_cmp.py PARENT.s NEW.s [regex of the kernels to list one by one] [--diff]
Kernels matching the regex and every differing kernel get a line each (a differing one with
its number of changed lines); the rest are counted.  --diff prints the unified diffs too."""
import difflib
import re
import sys

from mfma_waits import insn, split_kernels


def stream(body):
    out = []
    for line in body:
        if line.strip().startswith(".amdhsa_kernel"):   # the descriptor ends the code
            break
        s = insn(line)
        if s:
            out.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--diff"]
    a, b = split_kernels(args[0]), split_kernels(args[1])
    pat = re.compile(args[2] if len(args) > 2 else ".")
    kern = lambda ks, n: n in ks and any(l.strip().startswith(".amdhsa_kernel") for l in ks[n])
    names = [n for n in sorted(set(a) | set(b)) if kern(a, n) or kern(b, n)]
    count = {"identical": 0, "DIFFERENT": 0}
    for n in names:
        sa, sb = stream(a.get(n, [])), stream(b.get(n, []))
        d = [l for l in difflib.unified_diff(sa, sb, "parent", "new", lineterm="", n=2)]
        changed = sum(1 for l in d if l[0] in "+-" and l[:3] not in ("+++", "---"))
        kind = "identical" if sa == sb else "DIFFERENT"
        count[kind] += 1
        if pat.search(n) or sa != sb:
            print("%s  %d | %d instructions  %s%s" % (
                n, len(sa), len(sb), kind, "  (%d changed lines)" % changed if changed else ""))
        if "--diff" in sys.argv:
            for l in d:
                print("    " + l)
    print("%d kernel symbols: %s" % (len(names), ", ".join("%d %s" % (v, k)
                                                           for k, v in count.items())))


if __name__ == "__main__":
    main()
