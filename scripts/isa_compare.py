"""Compare the gfx950 code of chosen kernels between two builds of libpdhg.so (static check, CPU only).
usage: python scripts/isa_compare.py OLD_LIB NEW_LIB [kernel-name ... | --all]

Every kernel whose symbol contains one of the substrings (default: the kernels that are wrappers around a shared
body, and their mixed forms) is disassembled from both libraries with the helpers of tests/test_isa_dma.py and
compared as text after normalisation: addresses, encodings, comments and branch targets are dropped.  Per symbol:
  A  the instruction sequences are identical
  B  the same multiset of opcodes, and the same VGPR / AGPR / SGPR counts, scratch and spill bytes and LDS bytes in
     the code object's metadata (occupancy is a function of these), in another order or on other registers
  C  anything else (the opcodes that differ in number are listed)
--all takes every symbol of the code objects (a host-only change must leave all of them in tier A) and ends with the
symbol counts.  The script knows nothing about particular instructions.  Exit status 1 if a symbol is missing on one
side or in C.
"""
import collections
import importlib.util
import os
import pathlib
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["k_invy_update_fast_2d", "k_invy_update_pair_2d", "k_dual_fast_2d", "k_invy_update_2d", "k_dual_2d",
           "k_dual_multi_2d", "k_invy_update_fast_mixed_2d", "k_dual_fast_mixed_2d", "k_invy_update_mixed_2d",
           "k_dual_mixed_2d", "k_dual_multi_mixed_2d"]
META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count",
        ".sgpr_spill_count", ".group_segment_fixed_size"]

_spec = importlib.util.spec_from_file_location("test_isa_dma", os.path.join(ROOT, "tests", "test_isa_dma.py"))
isa = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa)


def normalise(body):
    out = []
    for ln in body:
        ln = ln.split("//")[0].strip()
        if not ln or re.match(r"^[0-9a-f]+ <.*>:$", ln):
            continue
        ln = re.sub(r"\s+", " ", ln)
        if re.match(r"^s_(c?branch|call)", ln):
            ln = ln.split(" ")[0]
        out.append(ln)
    return out


def metadata(code_object):
    txt = subprocess.run([os.path.join(isa.LLVM, "llvm-readelf"), "--notes", code_object], check=True,
                         capture_output=True, text=True).stdout
    out, cur = {}, {}
    for ln in txt.splitlines() + ["  - .end: 0"]:
        m = re.match(r"^  (-| ) (\.\w+):\s*(\S*)$", ln)
        if not m:
            continue
        if m.group(1) == "-":
            if ".name" in cur:
                out[cur[".name"]] = tuple(cur.get(k, "0") for k in META)
            cur = {}
        cur[m.group(2)] = m.group(3)
    return out


def kernels(lib, parts):
    isa.LIB = lib
    with tempfile.TemporaryDirectory() as td:
        lines = isa._disassemble(pathlib.Path(td))
        meta = metadata(os.path.join(td, "gfx950.o"))
    out = {}
    for part in parts:
        needle = "" if part == "--all" else "pdhg" + str(len(part)) + part + "I"
        for head, body in isa._kernel_bodies(lines, needle).items():
            sym = re.search(r"<(.*)>:", head).group(1)
            out[sym] = (normalise(body), meta.get(sym))
    return out


def main():
    old_lib, new_lib, parts = sys.argv[1], sys.argv[2], sys.argv[3:] or DEFAULT
    old, new = kernels(old_lib, parts), kernels(new_lib, parts)
    syms = sorted(set(old) | set(new))
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.splitlines()
    bad, tiers = 0, collections.Counter()
    print("# tier  instructions old/new  kernel   (metadata: {})".format(" ".join(k.lstrip(".") for k in META)))
    for sym, name in zip(syms, dem):
        name = re.sub(r"^void pdhg::|\(pdhg::KP<.*$", "", name)
        if sym not in old or sym not in new:
            print("missing in {}: {}".format("OLD" if sym not in old else "NEW", name))
            bad += 1
            continue
        (bo, mo), (bn, mn) = old[sym], new[sym]
        ho, hn = collections.Counter(l.split(" ")[0] for l in bo), collections.Counter(l.split(" ")[0] for l in bn)
        if bo == bn and mo == mn:
            tier, note = "A", ""
        elif ho == hn and mo == mn:
            tier, note = "B", "  metadata {}".format(" ".join(mn))
        else:
            diff = {k: (ho[k], hn[k]) for k in sorted(set(ho) | set(hn)) if ho[k] != hn[k]}
            tier, note = "C", "  metadata {} -> {}  opcodes {}".format(" ".join(mo), " ".join(mn), diff)
            bad += 1
        tiers[tier] += 1
        print("{}  {:>6}/{:<6} {}{}".format(tier, len(bo), len(bn), name, note))
    if parts == ["--all"]:
        print("# symbols: old {} new {}; tier A {}, B {}, C {}".format(len(old), len(new), tiers["A"], tiers["B"], tiers["C"]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
