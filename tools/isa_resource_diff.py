"""Resource figures of every kernel in two device-ISA dumps (tools/isa_dump.sh), side by side.
usage: isa_resource_diff.py parent.s branch.s  -> the kernels whose figures differ (old -> new), the number of unchanged ones, and the
checks a refactor has to pass: no kernel gains scratch, none changes its LDS size, none moves to another waves-per-SIMD bucket."""
import re
import subprocess
import sys

KEYS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def figures(path):
    out, name = {}, None
    for l in open(path):
        l = l.strip()
        if l.startswith(".amdhsa_kernel "):
            name = l.split()[1]
            out[name] = {}
        elif l.startswith(".end_amdhsa_kernel"):
            name = None
        elif name and l.startswith(".amdhsa_"):
            k, _, v = l[len(".amdhsa_"):].partition(" ")
            if k in KEYS:
                out[name][k] = int(v)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, (re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for d in r.stdout.splitlines())))
    except Exception:
        return {n: n for n in names}


def waves(f):
    """waves per SIMD the register count allows: 512 unified VGPRs per lane, granules of 8, at most 8 waves"""
    v = (f["next_free_vgpr"] + 7) // 8 * 8
    return min(8, 512 // max(v, 8))


def main():
    a, b = figures(sys.argv[1]), figures(sys.argv[2])
    dm = demangle(sorted(set(a) | set(b)))
    print("kernels: %d in the parent, %d in the branch; only in the parent: %s; only in the branch: %s" % (
        len(a), len(b), sorted(dm[n] for n in set(a) - set(b)) or "none", sorted(dm[n] for n in set(b) - set(a)) or "none"))
    common = sorted(set(a) & set(b), key=lambda n: dm[n])
    changed = [n for n in common if a[n] != b[n]]
    print("unchanged in all of %s: %d of %d" % (", ".join(KEYS), len(common) - len(changed), len(common)))
    print("\nchanged (parent -> branch):")
    for n in changed:
        d = ["%s %d -> %d" % (k, a[n][k], b[n][k]) for k in KEYS if a[n][k] != b[n][k]]
        print("  %s\n      %s; waves/SIMD by registers %d -> %d" % (dm[n], "; ".join(d), waves(a[n]), waves(b[n])))
    bad = False
    for what, f in (("gains scratch", lambda x, y: y["private_segment_fixed_size"] > x["private_segment_fixed_size"]),
                    ("changes its LDS size", lambda x, y: y["group_segment_fixed_size"] != x["group_segment_fixed_size"]),
                    ("moves to another waves-per-SIMD bucket", lambda x, y: waves(x) != waves(y))):
        hit = [dm[n] for n in changed if f(a[n], b[n])]
        bad = bad or bool(hit)
        print("\nno kernel %s: %s" % (what, "true" if not hit else "FALSE: " + ", ".join(hit)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
