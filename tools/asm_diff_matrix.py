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


def one_more_false(name, new):
    """The symbol in `new` of a template instantiation `name` whose template gained one more bool parameter
    that defaults to false (DESIGN.md sections 19, 20), or None."""
    m = re.match(r"^(.*kernelI(?:L[ib]\d+E)+)(EEv.*)$", name)
    cand = m.group(1) + "Lb0E" + m.group(2) if m else None
    return cand if cand in new else None


KERNARG = re.compile(r"^(s_load_dword(?:x\d+)? \S+ s\[0:1\], )0x[0-9a-f]+$")


def kernarg_only(x, y):
    """The two streams differ only in the offsets of scalar loads from the kernel arguments (a later argument
    moved because an earlier one grew)."""
    if len(x) != len(y):
        return False
    for p, q in zip(x, y):
        if p != q:
            mp, mq = KERNARG.match(p), KERNARG.match(q)
            if not (mp and mq and mp.group(1) == mq.group(1)):
                return False
    return True


def main(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    paired = set()
    for k in sorted(a):
        n_old = sum(1 for x in a[k] if x != "LABEL:")
        kn, note = k, ""
        if k not in b:
            kn = one_more_false(k, b)
            note = "  (one more template parameter: its instantiation at false)"
            if kn is None:
                kn = local_instance(k, b)
                note = "  (now a template: its instantiation at 0)"
            if kn is None:
                print("%-60s %5d  MISSING" % (k, n_old))
                bad = 1
                continue
            paired.add(kn)
        n_new = sum(1 for x in b[kn] if x != "LABEL:")
        same = a[k] == b[kn]
        if not same and kernarg_only(a[k], b[kn]):
            print("%-60s %5d %5d  same but for kernel-argument offsets%s" % (k, n_old, n_new, note))
            continue
        bad |= not same
        print("%-60s %5d %5d  %s%s" % (k, n_old, n_new, "same" if same else "DIFFERENT", note))
    for k in sorted(set(b) - set(a) - paired):
        print("%-60s     - %5d  new" % (k, sum(1 for x in b[k] if x != "LABEL:")))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
