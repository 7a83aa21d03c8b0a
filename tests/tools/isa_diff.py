"""Compare the machine code of two builds of the library, kernel by kernel: what a refactoring of device code has to leave alone.

    python tests/tools/isa_diff.py OLD.so NEW.so

Prints the kernels that only one library has and the kernels whose fingerprint (kernel_resources.kernel_isa_hashes: machine code
and kernel descriptor) differs; exit status 1 if there are any, 0 if the two libraries hold the same kernels with the same code."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr


def isa_diff(old, new):
    """(number of kernels in `new`, [report lines]); no lines: every kernel of either library is in both, byte for byte."""
    a, b = kr.kernel_isa_hashes(lib=old), kr.kernel_isa_hashes(lib=new)
    lines = [f"only in {old}: {kr.demangle(n)}" for n in sorted(set(a) - set(b))]
    lines += [f"only in {new}: {kr.demangle(n)}" for n in sorted(set(b) - set(a))]
    lines += [f"differs: {kr.demangle(n)}  {a[n]} -> {b[n]}" for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    return len(b), lines


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    n, lines = isa_diff(sys.argv[1], sys.argv[2])
    print("\n".join(lines + [f"{n} kernels in {sys.argv[2]}: " + (f"{len(lines)} differences" if lines else "identical machine code")]))
    sys.exit(1 if lines else 0)
