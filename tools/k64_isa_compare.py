"""Same-machine-code check for csrc/pam_bwd64.hip across a refactor: compares the gfx950 instruction streams and the
register / scratch metadata of the 24 shipped pam_bwd_k64_kernel instantiations (CT 1..6 x F16 x ATOMIC) and of the two
helper kernels in two assembly listings.

    hipcc <build.py FLAGS> --cuda-device-only -S gan-danet_amd/csrc/pam_bwd64.hip -o before.s      (at the older commit)
    hipcc <build.py FLAGS> --cuda-device-only -S gan-danet_amd/csrc/pam_bwd64.hip -o after.s
    python tools/k64_isa_compare.py before.s after.s

Either listing may come from the five-parameter template <CT, F16, VREG, ATOMIC, ORDER> (the shipped instantiations
are VREG = 2, ORDER = 8; the others are counted and ignored) or from the three-parameter <CT, F16, ATOMIC>.
Normalised before the diff: the mangled kernel symbol (template arguments, the dropped trailing `unsigned int*`
parameter), the per-function number in local labels (.LBB<n>_, .Lfunc_end<n>), comment-only lines.
Where a pair differs, the line says whether the sweep over the query tiles (the innermost loop around an s_barrier, where
the kernel spends its time) is still identical or the same instructions with other register numbers, and the diff follows.  Exit status 0 = every pair identical."""
import difflib
import re
import sys

K64 = re.compile(r"pam_bwd_k64_kernelI((?:L[ib]\d+E)+)EEvPKtS2_S2_S2_S2_PKfiPfS5_Pvll(?:Pj)?")
META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size")
INFO_KEYS = (".group_segment_fixed_size", ".kernarg_segment_size")


def canon(sym):
    """mangled name -> ('k64', CT, F16, ATOMIC) for a shipped instantiation, None for a variant, the name itself otherwise"""
    m = K64.search(sym)
    if not m:
        return sym
    a = [int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1))]
    if len(a) == 5:
        if a[2] != 2 or a[4] != 8:
            return None
        a = [a[0], a[1], a[3]]
    return ("k64", a[0], a[1], a[2])


def normalise(line):
    line = K64.sub(lambda m: "pam_bwd_k64_kernel<%s>" % (canon(m.group(0)),), line)
    line = re.sub(r"\s*;.*$", "", line)                     # trailing comments (symbol names, loop notes with padding)
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    return re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)


def parse(path):
    """-> ({key: [normalised body lines]}, {key: {metadata key: value}}, counts)"""
    lines = open(path).read().split("\n")
    bodies, meta = {}, {}
    n_k64 = n_spill = n_kernels = 0
    i = 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+):", lines[i])
        if m and not m.group(1).endswith(".kd"):
            j = i
            while not re.match(r"^\.Lfunc_end\d+:", lines[j]):
                j += 1
            key = canon(m.group(1))
            if key is not None:
                body = [normalise(l) for l in lines[i:j + 1]]
                bodies[key] = [l for l in body if l.strip() and not l.strip().startswith(";")]
            i = j
        i += 1
    cur = None
    for l in lines[lines.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in lines else []:
        if l.startswith("  - "):
            if cur:
                _store(cur, meta)
            cur, l = {}, "    " + l[4:]
        m = re.match(r"^    (\.\w+):\s+(\S+)$", l)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
        if l.startswith("amdhsa.target"):
            break
    if cur:
        _store(cur, meta)
    for name, d in meta.pop("_all").items():
        n_kernels += 1
        if "pam_bwd_k64_kernel" in name:
            n_k64 += 1
            n_spill += int(d[".vgpr_spill_count"]) != 0
    return bodies, meta, (n_k64, n_spill, n_kernels)


def _store(d, meta):
    meta.setdefault("_all", {})[d[".name"]] = d
    key = canon(d[".name"])
    if key is not None:
        meta[key] = d


def tile_loop(body):
    """[first, last] line of the innermost loop around an s_barrier (the sweep over the query tiles), or None"""
    at = {l[:-1]: i for i, l in enumerate(body) if l.startswith(".LBB_") and l.endswith(":")}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"\s+s_cbranch_\w+ (\.LBB_\d+)$", l)
        if m and at.get(m.group(1), i) < i and any("s_barrier" in x for x in body[at[m.group(1)]:i]):
            if best is None or i - at[m.group(1)] < best[1] - best[0]:
                best = (at[m.group(1)], i)
    return best


def loop_verdict(x, y):
    """(number of differing lines, what became of the tile loop)"""
    lx, ly = tile_loop(x), tile_loop(y)
    if lx is None or ly is None:
        return 0, "NO TILE LOOP FOUND"
    n = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes()
            if tag != "equal")
    bx, by = x[lx[0]:lx[1] + 1], y[ly[0]:ly[1] + 1]
    if bx == by:
        return n, "tile loop (%d lines) identical" % len(by)
    # same opcodes, immediates, labels and order; only register numbers differ
    skel = lambda b: [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l) for l in b]
    if skel(bx) == skel(by):
        return n, "tile loop (%d lines): same instructions in the same order, register numbers differ in %d" % (
            len(by), sum(p != q for p, q in zip(bx, by)))
    return n, "TILE LOOP DIFFERS"


def label(key):
    return "pam_bwd_k64_kernel<CT=%d, F16=%d, ATOMIC=%d>" % key[1:] if isinstance(key, tuple) else re.sub(r"^_ZN\d+_GLOBAL__N_1\d+(\w+?)E.*", r"\1", key)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (b0, m0, c0), (b1, m1, c1) = parse(sys.argv[1]), parse(sys.argv[2])
    for name, c in (("before", c0), ("after", c1)):
        print("%-6s: %d pam_bwd_k64_kernel symbols, %d of them spill, %d kernels in the file" % (name, *c))
    bad = 0
    keys = sorted(set(b0) | set(b1), key=lambda k: (isinstance(k, str), k))
    if sum(isinstance(k, tuple) for k in keys) != 24:
        print("expected 24 shipped instantiations, found %d" % sum(isinstance(k, tuple) for k in keys))
        bad += 1
    for k in keys:
        if k not in b0 or k not in b1:
            print("%-52s MISSING in %s" % (label(k), "before" if k not in b0 else "after"))
            bad += 1
            continue
        same_isa = b0[k] == b1[k]
        same_meta = all(m0[k][q] == m1[k][q] for q in META_KEYS)
        clean = int(m1[k][".vgpr_spill_count"]) == 0 and int(m1[k][".private_segment_fixed_size"]) == 0
        info = "  ".join("%s %s -> %s" % (q[1:].split("_")[0], m0[k][q], m1[k][q]) for q in INFO_KEYS)
        regs = "v%s a%s s%s spill %s scratch %s" % tuple(m1[k][q] for q in META_KEYS)
        ok = same_isa and same_meta and clean
        status = "identical"
        if not same_isa:
            n, what = loop_verdict(b0[k], b1[k])
            status = "%d lines differ; %s" % (n, what)
        elif not ok:
            status = "METADATA DIFFERS"
        print("%-52s %s  %5d lines  %s  %s" % (label(k), status, len(b1[k]), regs, info))
        if not ok:
            bad += 1
            if not same_meta:
                print("    metadata before: " + ", ".join("%s=%s" % (q, m0[k][q]) for q in META_KEYS))
            for l in list(difflib.unified_diff(b0[k], b1[k], "before", "after", lineterm="", n=2))[:200]:
                print("    " + l)
    print("VERDICT: " + ("all %d kernels identical" % len(keys) if not bad else "%d kernel(s) differ" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
