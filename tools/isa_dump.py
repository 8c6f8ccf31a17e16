"""The gfx950 code object inside a built object or library, and its disassembly.

    python tools/isa_dump.py yocto_raytracing_amd/libyrt.so            # code identity (sha256)
    python tools/isa_dump.py --isa OUT.txt yocto_raytracing_amd/_build/wavefront.o
    python tools/isa_dump.py --compare PARENT.o [--out TABLE.txt] NEW.o   # one verdict per kernel

The disassembly is normalised (addresses, encodings and branch-target offsets
stripped) so that two builds can be diffed: a refactor that only removes
compile-time variants must leave every default kernel's instructions unchanged.

--compare gives each symbol of the two builds one verdict (classify):
    identical   the same instruction lines and the same resources
    same-mix    the same number of instructions per mnemonic and the same resources (registers,
                spills, private and LDS bytes); the number of differing lines follows. This is
                what moving straight-line statements into an inlined function may do: the
                scheduler places an instruction elsewhere or swaps a commutative operation's
                operands
    changed     anything else; the mnemonic and resource deltas follow
"""
from __future__ import annotations

import argparse
import collections
import difflib
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def _codeid():
    # by path: importing the package would load libyrt.so (and torch)
    import importlib.util

    spec = importlib.util.spec_from_file_location("yrt_codeid", ROOT / "yocto_raytracing_amd" / "codeid.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_C = _codeid()
LLVM, code_identity, code_objects = _C.LLVM, _C.code_identity, _C.code_objects


def disassemble(co: bytes) -> str:
    with tempfile.TemporaryDirectory() as td:
        p = Path(td) / "co"
        p.write_bytes(co)
        r = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", str(p)],
                           check=True, capture_output=True, text=True)
    out = []
    for line in r.stdout.splitlines():
        line = re.sub(r"//.*$", "", line).rstrip()
        line = re.sub(r"<[^>]*\+0x[0-9a-f]+>", "<L>", line)  # branch targets inside a function
        if line and not line.startswith(str(p)):
            out.append(line)
    return "\n".join(out) + "\n"


def split_symbols(isa: str) -> dict:
    """normalised disassembly -> {symbol: its instruction lines, stripped}"""
    out, cur = {}, None
    for line in isa.splitlines():
        m = re.fullmatch(r"<(\S+)>:", line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line[:1].isspace() and line.strip():
            cur.append(line.strip())
    return out


Verdict = collections.namedtuple("Verdict", "verdict differing mnemonics resources")


def classify(parent: list, new: list, parent_res: dict | None = None, new_res: dict | None = None) -> Verdict:
    """the verdict on one symbol from its instruction lines and resource figures in both builds.
    differing: lines of the longer listing that a diff of the two leaves unmatched; mnemonics: {mnemonic: new count - parent count} where
    they differ; resources: {figure: (parent, new)} where they differ"""
    pr, nr = parent_res or {}, new_res or {}
    resources = {k: (pr.get(k), nr.get(k)) for k in sorted(set(pr) | set(nr)) if pr.get(k) != nr.get(k)}
    if parent == new and not resources:
        return Verdict("identical", 0, {}, {})
    sm = difflib.SequenceMatcher(None, parent, new, autojunk=False)
    differing = max(len(parent), len(new)) - sum(b.size for b in sm.get_matching_blocks())
    pm = collections.Counter(line.split()[0] for line in parent)
    nm = collections.Counter(line.split()[0] for line in new)
    mnemonics = {k: nm[k] - pm[k] for k in sorted(set(pm) | set(nm)) if nm[k] != pm[k]}
    return Verdict("changed" if mnemonics or resources else "same-mix", differing, mnemonics, resources)


def _demangle(names: list) -> dict:
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=str(LLVM))
    if not names or not filt:
        return {n: n for n in names}
    r = subprocess.run([filt], input="\n".join(names) + "\n", check=True, capture_output=True, text=True)
    return dict(zip(names, r.stdout.splitlines()))


def compare(parent: Path, new: Path) -> str:
    """the per-symbol table of two objects or libraries, and a first line of totals"""
    isa = [split_symbols("".join(disassemble(co) for co in code_objects(p))) for p in (parent, new)]
    res = [_C.kernel_resources(p) for p in (parent, new)]
    names = sorted(set(isa[0]) | set(isa[1]))
    pretty = _demangle(names)
    rows, totals = [], collections.Counter()
    for n in names:
        if n not in isa[0] or n not in isa[1]:
            v = Verdict("new" if n in isa[1] else "removed", 0, {}, {})
        else:
            v = classify(isa[0][n], isa[1][n], res[0].get(n), res[1].get(n))
        totals[v.verdict] += 1
        kind = "kernel" if n in res[0] or n in res[1] else "function"
        rows.append(f"{v.verdict:<10} {len(isa[0].get(n, [])):>6} -> {len(isa[1].get(n, [])):>6}  "
                    f"differing {v.differing:>4}  {kind:<8} {pretty[n]}")
        if v.mnemonics:
            rows.append("    mnemonics (new - parent): " + ", ".join(f"{k} {d:+d}" for k, d in v.mnemonics.items()))
        if v.resources:
            rows.append("    resources (parent -> new): " + ", ".join(f"{k} {a} -> {b}" for k, (a, b) in v.resources.items()))
    head = "  ".join(f"{k}: {totals[k]}" for k in ("identical", "same-mix", "changed", "new", "removed"))
    return head + "\n" + "\n".join(rows) + "\n"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--isa", help="write the normalised disassembly here")
    ap.add_argument("--compare", metavar="PARENT", help="classify every symbol of `path` against this build's")
    ap.add_argument("--out", help="(--compare) write the table here instead of printing it")
    a = ap.parse_args(argv)
    if a.compare:
        table = compare(Path(a.compare), Path(a.path))
        if a.out:
            Path(a.out).write_text(table)
            print(table.splitlines()[0])
        else:
            print(table, end="")
        return 0
    print(code_identity(Path(a.path)))
    if a.isa:
        Path(a.isa).write_text("".join(disassemble(co) for co in code_objects(Path(a.path))))


if __name__ == "__main__":
    sys.exit(main())
