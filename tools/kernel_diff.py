"""Per-kernel comparison of the gfx950 code of two builds (no GPU needed).

A refactor that moves kernels between translation units should leave their machine code alone.  This tool disassembles
the gfx950 code objects of two libraries (or of two .hip.o files) and compares every kernel, matched by mangled name, as
its sequence of (mnemonic, operands).  Addresses and encodings are ignored, and so is the alignment padding after a
kernel's last real instruction: the trailing run of one instruction repeated, which the assembler appends up to the
next alignment boundary and which changes with whatever follows the kernel in its code object.

    python tools/kernel_diff.py PARENT.so NEW.so     # exit 1 if a kernel exists on one side only

Kernels that differ are reported with both instruction counts but do not fail the run: whether a different schedule
is acceptable is decided by its resource usage (make asm) and a measurement.
"""

import sys

from lds_barrier_check import disassemble, functions


def normalise(insts):
    """[(addr, mnemonic, operands, line)] -> [(mnemonic, operands)] without the trailing alignment padding."""
    seq = [(mn, " ".join(ops.split())) for _, mn, ops, _ in insts]
    n = len(seq)
    while n >= 2 and seq[n - 1] == seq[n - 2]:
        n -= 1
    if n < len(seq):  # a run of >= 2 copies: all of it is padding
        n -= 1
    return seq[:n]


def kernels(path):
    """-> {mangled name: normalised instruction sequence} over every gfx950 code object of ``path``."""
    out = {}
    for text in disassemble(path):
        for name, (_, insts) in functions(text).items():
            key, k = name, 1
            while key in out:  # the same local name in two code objects
                k += 1
                key = "%s#%d" % (name, k)
            out[key] = normalise(insts)
    return out


def compare(a, b):
    """Two {name: sequence} maps -> (only in a, only in b, identical, differing).  A differing entry is (name, len a,
    len b, positions that differ, first differing pair); the last two only for sequences of equal length (else 0,
    None), where they show at a glance a kernel that differs in nothing but a resolved pc-relative literal."""
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    same, differ = [], []
    for name in sorted(set(a) & set(b)):
        if a[name] == b[name]:
            same.append(name)
        elif len(a[name]) != len(b[name]):
            differ.append((name, len(a[name]), len(b[name]), 0, None))
        else:
            pairs = [(x, y) for x, y in zip(a[name], b[name]) if x != y]
            differ.append((name, len(a[name]), len(b[name]), len(pairs), pairs[0]))
    return only_a, only_b, same, differ


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    only_a, only_b, same, differ = compare(kernels(argv[1]), kernels(argv[2]))
    print("only in %s: %d" % (argv[1], len(only_a)))
    for name in only_a:
        print("  " + name)
    print("only in %s: %d" % (argv[2], len(only_b)))
    for name in only_b:
        print("  " + name)
    print("identical: %d" % len(same))
    for name in same:
        print("  " + name)
    print("differing: %d" % len(differ))
    for name, na, nb, npos, first in differ:
        print("  %s: %d -> %d instructions" % (name, na, nb))
        if first:
            print("    %d position(s) differ, the first: %s | %s" % (npos, " ".join(first[0]), " ".join(first[1])))
    return 1 if only_a or only_b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
