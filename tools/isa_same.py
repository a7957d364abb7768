"""Are the kernels of two hipcc -S listings the same code? (measurement aid; sibling of isa_loop.py)

    hipcc --offload-arch=gfx950 ... --cuda-device-only -S -o old.s langsplat_amd/csrc/lsr_render.hip
    python3 tools/isa_same.py old.s new.s [name-substring]

Per kernel of either listing: the instruction counts, whether the two mnemonic sequences are
identical (operands, hence register names and label numbers, are not compared) and whether the
resource figures the listing records are: VGPRs, SGPRs, scratch bytes per lane, VGPR and SGPR
spills, waves per SIMD and static LDS bytes.

    python3 tools/isa_same.py --loops old.s new.s [name-substring]

compares the kernels' loops instead (the blocks the compiler marks "Loop Header" / "in Loop:
Header=", as isa_loop.py finds them): per kernel, every loop's depth and instruction count, and
whether a loop with the same mnemonic sequence exists in the other listing.  A change confined to a
kernel's load phase leaves every inner (walk) loop "same" and shows only in the outer loops that
contain the load phase.
"""
import re
import shutil
import subprocess
import sys

INFO = {"NumVgprs": "vgpr", "TotalNumSgprs": "sgpr", "ScratchSize": "scratch", "Occupancy": "waves",
        "LDSByteSize": "lds"}
FIGURES = ["vgpr", "sgpr", "scratch", "vspill", "sspill", "waves", "lds"]


def kernels(path):
    """{symbol: ([mnemonic, ...], {figure: value})} of the listing's functions, in its order."""
    out, name, body, last, funcs = {}, None, False, None, set()
    for l in open(path):
        if m := re.match(r"^\s+\.type\s+(\w+),@function", l):
            funcs.add(m.group(1))
        elif (m := re.match(r"^(_Z\w+):", l)) and m.group(1) in funcs:
            name = last = m.group(1)
            out[name], body = ([], {}), True
        elif l.startswith(".Lfunc_end"):
            body = False
        elif body:
            s = l.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                out[name][0].append(s.split()[0])
        elif (m := re.match(r"^; (\w+): (\d+)", l)) and m.group(1) in INFO and last:
            out[last][1][INFO[m.group(1)]] = int(m.group(2))
        elif (m := re.match(r"^\s+\.name:\s+(\S+)", l)) and m.group(1) in out:  # the metadata follows all code
            last = m.group(1)
        elif (m := re.match(r"^\s+\.([sv])gpr_spill_count:\s+(\d+)", l)) and last in out:
            out[last][1][m.group(1) + "spill"] = int(m.group(2))
    return out


def loops(path):
    """{symbol: [(depth, [mnemonic, ...]), ...]} of the listing's loops, each with every block of its body."""
    out, name, funcs, blocks, cur = {}, None, set(), [], None
    def close():
        if name is None:
            return
        found = []
        for lab, ann, _ in blocks:
            if "Loop Header" not in ann or not lab.startswith(".LBB"):
                continue
            h = lab[2:]
            body = [x for lb, an, ls in blocks if lb == lab or re.search(r"Header=" + re.escape(h) + r"\b", an) for x in ls]
            depth = int(m.group(1)) if (m := re.search(r"Loop Header: Depth=(\d+)", ann)) else 0
            found.append((depth, body))
        out[name] = found
    for l in open(path):
        if m := re.match(r"^\s+\.type\s+(\w+),@function", l):
            funcs.add(m.group(1))
        elif (m := re.match(r"^(_Z\w+):", l)) and m.group(1) in funcs:
            name, blocks, cur = m.group(1), [], None
        elif l.startswith(".Lfunc_end"):
            close()
            name = None
        elif name is not None:
            if m := re.match(r"^(\.LBB\S+|; %bb\.\d+):?(.*)$", l):
                cur = [m.group(1).lstrip("; %").rstrip(":"), m.group(2), []]
                blocks.append(cur)
            elif cur is not None:
                if l.strip().startswith(";"):
                    cur[1] += l
                else:
                    t = l.split(";")[0].strip()
                    if t and not t.startswith(".") and not t.endswith(":"):
                        cur[2].append(t.split()[0])
    return out


def main_loops(argv):
    old, new = loops(argv[0]), loops(argv[1])
    want = argv[2] if len(argv) > 2 else ""
    names = [n for n in dict.fromkeys(list(old) + list(new)) if want in n]
    pretty = demangle(names)
    for n in names:
        lo, ln = old.get(n, []), new.get(n, [])
        seqs_old = [tuple(b) for _, b in lo]
        row = [f"d{d}:{len(b)}:" + ("same" if tuple(b) in seqs_old else "NEW") for d, b in ln]
        gone = sum(tuple(b) not in [tuple(x) for _, x in ln] for _, b in lo)
        print(f"{pretty[n]:<48} loops old {len(lo)} new {len(ln)}  " + " ".join(row) + (f"  ({gone} old loops have no match)" if gone else ""))


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return dict(zip(names, names))
    got = subprocess.run([tool] + names, capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void |lsr::|\(lsr::\w+\)$", "", g) for n, g in zip(names, got)}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--loops":
        return main_loops(sys.argv[2:])
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    want = sys.argv[3] if len(sys.argv) > 3 else ""
    names = [n for n in dict.fromkeys(list(old) + list(new)) if want in n]
    pretty = demangle(names)
    print(f"{'kernel':<48} {'instr old':>9} {'new':>6}  sequence   figures (" + " ".join(FIGURES) + ")")
    for n in names:
        (io, fo), (inw, fn) = old.get(n, ([], {})), new.get(n, ([], {}))
        seq = "only old" if n not in new else "only new" if n not in old else "identical" if io == inw else "DIFFERS"
        fig = lambda f: " ".join(str(f.get(k, "-")) for k in FIGURES)
        figs = f"same: {fig(fn)}" if fo == fn else f"{fig(fo)} -> {fig(fn)}"
        print(f"{pretty[n]:<48} {len(io):>9} {len(inw):>6}  {seq:<9}  {figs}")


if __name__ == "__main__":
    main()
