"""Compare the instruction streams of the matrix kernels in two device assembly files of
csrc/sw_matrix.hip (hipcc ... -S --cuda-device-only), label numbers aside: shows that a change to
the shared strip step left the existing instantiations alone (DESIGN.md sections 11, 12).

    python tools/asm_diff_matrix.py OLD.s NEW.s

Prints, per kernel of OLD, its instruction count in both files and "same" or "DIFFERENT", then the
kernels only NEW has.  Exit 1 if a kernel of OLD is missing from NEW or differs."""
import re
import sys


def kernels(path):
    """{demangled-ish symbol: [instruction lines]} of every .globl function in the file."""
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
            if m and not line.startswith(".L") and name is None and re.match(r"^_Z\w*sw_matrix\w*", m.group(1)):
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            t = line.strip()
            if t.startswith(".Lfunc_end"):
                out[name] = body
                name = None
                continue
            if not t or t.startswith(";") or t.startswith("."):
                if re.match(r"^\.LBB\d+_\d+:", t):
                    body.append("LABEL:")
                continue
            t = t.split(";")[0].strip()
            t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", t)       # the function's number in the file
            body.append(t)
    return out


def main(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    for k in sorted(a):
        n_old = sum(1 for x in a[k] if x != "LABEL:")
        if k not in b:
            print("%-60s %5d  MISSING" % (k, n_old))
            bad = 1
            continue
        n_new = sum(1 for x in b[k] if x != "LABEL:")
        same = a[k] == b[k]
        bad |= not same
        print("%-60s %5d %5d  %s" % (k, n_old, n_new, "same" if same else "DIFFERENT"))
    for k in sorted(set(b) - set(a)):
        print("%-60s     - %5d  new" % (k, sum(1 for x in b[k] if x != "LABEL:")))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
