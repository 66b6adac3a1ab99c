"""Compare the instruction streams of the matrix kernels in two device assembly files of
csrc/sw_matrix.hip (hipcc ... -S --cuda-device-only), label numbers aside: shows that a change to
the shared strip step left the existing instantiations alone (DESIGN.md sections 11, 12).

    python tools/asm_diff_matrix.py OLD.s NEW.s

Prints, per kernel of OLD, its instruction count in both files and "same" or "DIFFERENT", then the
kernels only NEW has.  Exit 1 if a kernel of OLD is missing from NEW or differs.

A kernel of OLD that NEW has made a template on the alignment mode is compared
with NEW's instantiation at 0, local -- the symbol with "ILi0EEEv" after the name -- and its line says so."""
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


def local_instance(name, new):
    """The symbol in `new` of kernel `name` made a template on one int and instantiated at 0, or None."""
    m = re.match(r"^(_ZN?(?:\d+[A-Za-z_]\w*?)*?\d+sw_matrix\w*?kernel)(E?)(.*)$", name)
    if not m:
        return None
    cand = m.group(1) + "ILi0EE" + m.group(2) + "v" + m.group(3)
    return cand if cand in new else None


def main(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    paired = set()
    for k in sorted(a):
        n_old = sum(1 for x in a[k] if x != "LABEL:")
        kn, note = k, ""
        if k not in b:
            kn = local_instance(k, b)
            if kn is None:
                print("%-60s %5d  MISSING" % (k, n_old))
                bad = 1
                continue
            paired.add(kn)
            note = "  (now a template: its instantiation at 0)"
        n_new = sum(1 for x in b[kn] if x != "LABEL:")
        same = a[k] == b[kn]
        bad |= not same
        print("%-60s %5d %5d  %s%s" % (k, n_old, n_new, "same" if same else "DIFFERENT", note))
    for k in sorted(set(b) - set(a) - paired):
        print("%-60s     - %5d  new" % (k, sum(1 for x in b[k] if x != "LABEL:")))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
