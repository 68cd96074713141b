"""Do two builds compile the same kernels?  python tools/isa_diff.py old.s new.s [more_new.s ...]

Reads hipcc's device assembly (`make -C csrc asm` leaves it under csrc/_build/asm/).  The first file is the old build; the others, taken
together, are the new one (a translation unit that was split).  Every kernel -- a `; -- Begin function` ... `; -- End function` block
that contains s_endpgm -- and every device function the compiler left out of line is compared after dropping comments and renumbering local labels (.LBB<n>_<m>) in order of appearance.  Kernels
are matched by their own name and template arguments and a kernel's own symbol is written KERNEL, so that a parameter type that changed
its namespace (or an anonymous namespace's hash) does not count.  Prints per kernel `identical`, or both sides' VGPRs, SGPRs,
scratch bytes, LDS bytes, occupancy and instruction count; then one summary line per kernel family.  Exit status 1 if a kernel differs
or exists on one side only."""
import re
import sys

_OWN = re.compile(r"(\d+)([A-Za-z_]\w*)")


def short(sym):
    """a kernel's key: its own name and template arguments, without namespaces and parameter types --
    _ZN12_GLOBAL__N_115knn_tile_kernelILi8E...Lb0EEEv11GridParams... -> knn_tile_kernelILi8E...Lb0E"""
    s = sym[2:].lstrip("NL").replace("12_GLOBAL__N_1", "")
    m = _OWN.match(s)
    if not m:
        return sym
    n = int(m.group(1))
    name, rest = m.group(2)[:n], s[m.end(1) + n:]
    args = re.match(r"(I.*?E)E*v", rest)
    return name + (args.group(1) if args else "")


def kernels(paths):
    out = {}
    for p in paths:
        txt = open(p).read()
        for blk in txt.split("; -- Begin function ")[1:]:
            sym = blk.split("\n", 1)[0].strip()
            body, _, tail = blk.partition("; -- End function")
            if "s_endpgm" in body:
                out[short(sym)] = (body, tail, sym)
            elif "s_setpc_b64" in body:                  # a device function left out of line: compared too, under its whole name
                out["(function) " + sym.replace("12_GLOBAL__N_1", "")] = (body, tail, sym)
    return out


def normal(body, sym):
    labels = {}
    lines = []
    for ln in body.split("\n")[1:]:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip():
            continue
        if sym:
            ln = ln.replace(sym, "KERNEL")
        ln = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+(_\d+)?", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), ln)
        lines.append(ln)
    return lines


def facts(body, tail):
    def num(pat, txt):
        m = re.search(pat, txt)
        return int(m.group(1)) if m else -1
    ins = sum(1 for ln in normal(body, "") if ln.startswith("\t") and not ln.lstrip().startswith("."))
    return dict(vgpr=num(r"\.amdhsa_next_free_vgpr (\d+)", body), sgpr=num(r"\.amdhsa_next_free_sgpr (\d+)", body), scratch=num(r"ScratchSize: (\d+)", tail),
                lds=num(r"LDSByteSize: (\d+)", tail), occupancy=num(r"Occupancy: (\d+)", tail), instructions=ins)


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    old, new = kernels(argv[1:2]), kernels(argv[2:])
    fam = {}
    bad = 0
    for name in sorted(set(old) | set(new)):
        f = fam.setdefault(re.match(r"\(function\)|[a-z0-9_]+", name).group(0), [0, 0, 0])
        f[0] += 1
        if name not in old or name not in new:
            print("%-90s only in the %s build" % (name, "old" if name in old else "new"))
            f[2] += 1
            bad = 1
            continue
        if normal(old[name][0], old[name][2]) == normal(new[name][0], new[name][2]):
            print("%-90s identical" % name)
            f[1] += 1
            continue
        bad = 1
        a, b = facts(*old[name][:2]), facts(*new[name][:2])
        print("%-90s DIFFERS  " % name + "  ".join("%s %d -> %d" % (k, a[k], b[k]) for k in a))
    for k in sorted(fam):
        n, same, lone = fam[k]
        print("summary %-24s %3d kernels, %3d identical, %d different, %d on one side only" % (k, n, same, n - same - lone, lone))
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv))
