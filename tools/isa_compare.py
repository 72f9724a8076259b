#!/usr/bin/env python3
"""Dev tool: are the kernels of two device-ISA dumps (tools/isa_dump.sh) the same instruction for instruction?

    tools/isa_compare.py parent.s head.s

Every function of the first dump is looked up in the second and its instructions (label to the kernel descriptor) compared; a kernel
whose instructions are equal but whose descriptor differs (.amdhsa_kernarg_size after a parameter struct grew) is listed as such and does
not count as different.  Two things are normalised:
the function index inside local labels (.LBB12_3 -> .LBB_3: inserting a kernel renumbers every later one) and the mangled name of a kernel
that gained a `template <bool>` parameter, whose <false> instantiation stands for the old kernel (k_foo(Params) -> k_foo<false>(Params)).
Prints one line per function that differs or is missing and a summary; exit status 1 when any does."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
            if name is None and m and not line.startswith(".L"):
                name, body = m.group(1), []
                continue
            if name is not None:
                if line.startswith(".Lfunc_end"):
                    out[name] = body
                    name = None
                    continue
                s = line.split(";")[0].rstrip()                       # comments carry symbol names
                if s:
                    body.append(s)
    return out


def normalise(name, body):
    """(instructions, kernel descriptor): the text up to the descriptor's section, and the .amdhsa_ lines of the descriptor."""
    cut = next((i for i, s in enumerate(body) if s.lstrip().startswith(".section") and ".rodata" in s), len(body))
    text = "\n".join(body[:cut]).replace(name, "@SELF")
    desc = [s.strip() for s in body[cut:] if s.strip().startswith(".amdhsa_") and not s.strip().startswith(".amdhsa_kernel ")]
    return re.sub(r"\.LBB\d+_", ".LBB_", text), desc


def old_name(name):
    """The name a <false> instantiation had as a plain kernel: _ZN3pba5k_fooILb0EEEvNS_6ParamsE -> _ZN3pba5k_fooENS_6ParamsE."""
    return name.replace("ILb0EEEv", "E", 1) if "ILb0EEEv" in name else None


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    by_old = {old_name(n): n for n in b if old_name(n)}
    bad = 0
    for name, body in a.items():
        other = name if name in b else by_old.get(name)
        if other is None:
            print("missing: %s" % name)
            bad += 1
        else:
            (ta, da), (tb, db) = normalise(name, body), normalise(other, b[other])
            if ta != tb:
                print("differs: %s" % name)
                bad += 1
            elif da != db:       # same instructions, another descriptor (a parameter struct that grew changes .amdhsa_kernarg_size)
                print("descriptor: %s: %s" % (name, "; ".join("%s -> %s" % (x, y) for x, y in zip(da, db) if x != y)))
    new = [n for n in b if n not in a and old_name(n) not in a]
    print("%d functions of %s compared, %d differ or are missing; %d new in %s" % (len(a), sys.argv[1], bad, len(new), sys.argv[2]))
    for n in new:
        print("new: %s" % n)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
