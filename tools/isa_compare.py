"""Same-machine-code check for a PAM kernel family across a refactor: compares the gfx950 instruction streams and the
register / scratch / LDS metadata of the family's shipped instantiations, and of every other kernel in the files, in
assembly listings made before and after.

    hipcc <build.py FLAGS> --cuda-device-only -S gan-danet_amd/csrc/pam_bwd64.hip -o before.s      (at the older commit)
    hipcc <build.py FLAGS> --cuda-device-only -S gan-danet_amd/csrc/pam_bwd64.hip -o after.s
    python tools/isa_compare.py k64 before.s after.s
    python tools/isa_compare.py pam_fwd pam_before.s pam_after.s pam_wide_before.s pam_wide_after.s
    python tools/isa_compare.py dkv3 pam_before.s pam_after.s pam_bwd64_before.s pam_bwd64_after.s

A family (FAMILIES below) names the kernel templates that are one kernel under different names or parameter lists and
maps each instantiation to its canonical parameters, None for a variant that is not shipped (counted and ignored).
Listings come in (before, after) pairs; the pairs are pooled, for a family whose instantiations sit in several files.
Normalised before the diff: the mangled kernel symbol, the per-function number in local labels (.LBB<n>_,
.Lfunc_end<n>), comment-only lines.
Where a pair differs, the line says whether the tile loop (the innermost loop around an s_barrier, where the kernel
spends its time) is still identical or the same instructions with other register numbers; --diff prints the diff too.
A kernel passes when its metadata is unchanged, nothing spills (family kernels, but for the instantiations a family lists
as spilling already) and its instructions are identical or differ outside an identical / register-renamed tile loop
only.  Exit status 0 = every kernel passes."""
import difflib
import re
import sys

META_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size",
             ".group_segment_fixed_size")
INFO_KEYS = (".kernarg_segment_size",)


def _k64(a):
    """<CT, F16, VREG, ATOMIC, ORDER> (shipped: VREG = 2, ORDER = 8) or <CT, F16, ATOMIC>"""
    if len(a) == 5:
        return (a[0], a[1], a[3]) if a[2] == 2 and a[4] == 8 else None
    return tuple(a)


def _dkv3(a):
    """<CT, DQ, NW> (shipped: DQ = 0, NW = 4; <CT, 1, 8> was the K32 parts form) or <CT>"""
    if len(a) == 3:
        return (a[0],) if a[1] == 0 and a[2] == 4 else None
    return tuple(a)


# family -> (canonical template, parameter names, shipped instantiations, {template name: arguments -> canonical tuple}
#            [, canonical tuples that spill as they stand: their spill count must only stay what it was])
FAMILIES = {
    "k64": ("pam_bwd_k64_kernel", ("CT", "F16", "ATOMIC"), 24, {"pam_bwd_k64_kernel": _k64}),
    "dkv3": ("pam_bwd_dkv3_kernel", ("CT",), 6, {"pam_bwd_dkv3_kernel": _dkv3}, {(6,)}),   # CT = 6: 256 VGPRs + 1 spilled
    "pam_fwd": ("pam_fwd_kernel", ("CT", "D", "KT", "ONES", "F16", "MAXFREE", "CHUNKED"), 40, {
        "pam_fwd_kernel": tuple,
        "pam_fwd_dma_kernel": lambda a: (a[0], 32, a[2], a[3], a[4], 1, 0) if a[1] == 8 else None,   # <CT, NW, KT, ONES, F16>
        "pam_wide_fwd_kernel": lambda a: (a[0], a[1], a[2], 0, a[3], 0, 1),                          # <CT, D, KT, F16>
    }),
}


class Family:
    def __init__(self, name):
        self.template, self.params, self.shipped, self.maps = FAMILIES[name][:4]
        self.spilling = {(self.template, *args) for args in (FAMILIES[name][4] if len(FAMILIES[name]) > 4 else ())}
        self.sym = re.compile(r"_Z\w*?\d+(%s)I((?:L[ib]\d+E)+)E\w*" % "|".join(sorted(self.maps, key=len, reverse=True)))

    def canon(self, sym):
        """mangled name -> (template, canonical arguments) for a shipped instantiation, None for a variant, the name
        itself for a kernel outside the family"""
        m = self.sym.fullmatch(sym[:-3] if sym.endswith(".kd") else sym)
        if not m:
            return sym
        args = self.maps[m.group(1)]([int(v) for v in re.findall(r"L[ib](\d+)E", m.group(2))])
        return None if args is None else (self.template, *args)

    def normalise(self, line):
        line = self.sym.sub(lambda m: "%s<%s>" % (self.template, self.canon(m.group(0))), line)
        line = re.sub(r"\s*;.*$", "", line)                     # trailing comments (symbol names, loop notes with padding)
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        return re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", line)

    def label(self, key):
        if isinstance(key, tuple):
            return "%s<%s>" % (key[0], ", ".join("%s=%d" % pv for pv in zip(self.params, key[1:])))
        m = re.search(r"\d+([a-z]\w*?_kernel)((?:I(?:L[ib]\d+E)+E)?)", key)
        return "%s<%s>" % (m.group(1), ", ".join(re.findall(r"L[ib](\d+)E", m.group(2)))) if m else key


def parse(fam, paths):
    """-> ({key: [normalised body lines]}, {key: {metadata key: value}}, (family symbols, of them spilling, kernels))"""
    bodies, meta, everything = {}, {}, {}
    for path in paths:
        lines = open(path).read().split("\n")
        i = 0
        while i < len(lines):
            m = re.match(r"^(_Z\w+):", lines[i])
            if m and not m.group(1).endswith(".kd"):
                j = i
                while not re.match(r"^\.Lfunc_end\d+:", lines[j]):
                    j += 1
                key = fam.canon(m.group(1))
                if key is not None:
                    body = [fam.normalise(l) for l in lines[i:j + 1]]
                    bodies[key] = [l for l in body if l.strip() and not l.strip().startswith(";")]
                i = j
            i += 1
        cur = None
        for l in lines[lines.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in lines else []:
            if l.startswith("  - "):
                if cur:
                    everything[cur[".name"]] = cur
                cur, l = {}, "    " + l[4:]
            m = re.match(r"^    (\.\w+):\s+(\S+)$", l)
            if cur is not None and m:
                cur[m.group(1)] = m.group(2)
            if l.startswith("amdhsa.target"):
                break
        if cur:
            everything[cur[".name"]] = cur
    n_fam = n_spill = 0
    for name, d in everything.items():
        key = fam.canon(name)
        if key is not None:
            meta[key] = d
        if key != name:
            n_fam += 1
            n_spill += int(d[".vgpr_spill_count"]) != 0
    return bodies, meta, (n_fam, n_spill, len(everything))


def tile_loop(body):
    """[first, last] line of the innermost loop around an s_barrier (the sweep over the tiles), or None"""
    at = {l[:-1]: i for i, l in enumerate(body) if l.startswith(".LBB_") and l.endswith(":")}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w* (\.LBB_\d+)$", l)
        if m and at.get(m.group(1), i) < i and any("s_barrier" in x for x in body[at[m.group(1)]:i]):
            if best is None or i - at[m.group(1)] < best[1] - best[0]:
                best = (at[m.group(1)], i)
    return best


def loop_verdict(x, y):
    """(number of differing lines, what became of the tile loop, whether it is the same loop)"""
    n = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes()
            if tag != "equal")
    lx, ly = tile_loop(x), tile_loop(y)
    if lx is None or ly is None:
        return n, "NO TILE LOOP FOUND", False
    bx, by = x[lx[0]:lx[1] + 1], y[ly[0]:ly[1] + 1]
    # local labels are numbered through the function: code that moved outside the loop renumbers the ones inside
    ren = lambda b: [re.sub(r"\.LBB_\d+", ".LBB_#", l) for l in b]
    if ren(bx) == ren(by):
        return n, "tile loop (%d lines) identical" % len(by), True
    # same opcodes, immediates and order; only register numbers differ
    skel = lambda b: [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l) for l in ren(b)]
    if skel(bx) == skel(by):
        return n, "tile loop (%d lines): same instructions in the same order, register numbers differ in %d" % (
            len(by), sum(p != q for p, q in zip(ren(bx), ren(by)))), True
    return n, "TILE LOOP DIFFERS", False


def main():
    argv = [a for a in sys.argv[1:] if a != "--diff"]
    if len(argv) < 3 or len(argv) % 2 == 0 or argv[0] not in FAMILIES:
        sys.exit(__doc__)
    fam = Family(argv[0])
    (b0, m0, c0), (b1, m1, c1) = parse(fam, argv[1::2]), parse(fam, argv[2::2])
    for name, c in (("before", c0), ("after", c1)):
        print("%-6s: %d symbols of the %s family, %d of them spill, %d kernels in the file(s)" % (name, c[0], argv[0], c[1], c[2]))
    bad = 0
    keys = sorted(set(b0) | set(b1), key=lambda k: (isinstance(k, str), k))
    if sum(isinstance(k, tuple) for k in keys) != fam.shipped:
        print("expected %d shipped instantiations, found %d" % (fam.shipped, sum(isinstance(k, tuple) for k in keys)))
        bad += 1
    width = max(len(fam.label(k)) for k in keys)
    for k in keys:
        if k not in b0 or k not in b1:
            print("%-*s MISSING in %s" % (width, fam.label(k), "before" if k not in b0 else "after"))
            bad += 1
            continue
        same_isa = b0[k] == b1[k]
        same_meta = all(m0[k][q] == m1[k][q] for q in META_KEYS)
        clean = isinstance(k, str) or k in fam.spilling or (int(m1[k][".vgpr_spill_count"]) == 0 and int(m1[k][".private_segment_fixed_size"]) == 0)
        info = "  ".join("%s %s -> %s" % (q[1:].split("_")[0], m0[k][q], m1[k][q]) for q in INFO_KEYS)
        regs = "v%s a%s s%s spill %s scratch %s lds %s" % tuple(m1[k][q] for q in META_KEYS)
        status, same_loop = "identical", True
        if not same_isa:
            n, what, same_loop = loop_verdict(b0[k], b1[k])
            status = "%d lines differ; %s" % (n, what)
        ok = same_meta and clean and same_loop
        if not same_meta:
            status += "; METADATA DIFFERS"
        print("%-*s %s  %5d lines  %s  %s" % (width, fam.label(k), status, len(b1[k]), regs, info))
        if not same_meta:
            print("    metadata before: " + ", ".join("%s=%s" % (q, m0[k][q]) for q in META_KEYS))
        if not ok:
            bad += 1
        if "--diff" in sys.argv and not same_isa:
            for l in list(difflib.unified_diff(b0[k], b1[k], "before", "after", lineterm="", n=2))[:200]:
                print("    " + l)
    print("VERDICT: " + ("all %d kernels keep their metadata and their tile loop" % len(keys) if not bad else "%d kernel(s) fail" % bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
