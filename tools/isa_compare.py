#!/usr/bin/env python3
"""Compares the gfx950 device code of HIP sources between two trees, per function.

  tools/isa_compare.py OLD_TREE NEW_TREE FILE.hip... [--allow NAME]...

Each FILE (a path inside a tree, or a bare name under kingdb_amd/csrc) is
compiled in both trees to device assembly with the HIPFLAGS of that tree's
kingdb_amd/Makefile plus --cuda-device-only -S.  The assembly is split into
functions by symbol, comments are dropped, and what depends only on a
function's place in its file is normalised: the basic-block label numbers
(.LBB<n>_, .Lfunc_end<n>) and the __hip_cuid_* symbol.  One line per function:

  IDENTICAL (n lines) | DIFFERENT | only in old | only in new   <demangled name>

Exit status 1 if a function is DIFFERENT and not named by --allow (a
demangled name, or the part of it before its parameter list).  The comparison
is of text and nothing more.

Get the old tree with plain git, e.g.
  git worktree add --detach /tmp/parent HEAD~1
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

_LABEL = re.compile(r"\.L(BB|func_begin|func_end|JTI|tmp)\d+")
_CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_SIZE = re.compile(r"^\s*\.size\s+([^\s,]+),")
_SET = re.compile(r"^\s*\.set\s+([^\s,]+)\.[a-z_]+,")


def normalise(line: str) -> str:
    """One assembly line without its comment, place-dependent numbers masked; '' if nothing is left."""
    if '"' not in line:                      # (a ';' inside a string is no comment)
        line = line.split(";", 1)[0]
    line = _LABEL.sub(lambda m: ".L" + m.group(1), line)
    line = _CUID.sub("__hip_cuid", line)
    return " ".join(line.split())


def split_functions(asm: str) -> dict[str, list[str]]:
    """symbol -> its normalised lines: from `.type sym,@function` to `.size sym,` (the kernel
    descriptor lies between them), and the `.set sym.<resource>` lines that follow."""
    funcs: dict[str, list[str]] = {}
    cur = None
    for raw in asm.splitlines():
        line = normalise(raw)
        if not line:
            continue
        m = _TYPE.match(line)
        if m:
            cur = m.group(1)
            funcs[cur] = []
        if cur is not None:
            funcs[cur].append(line)
            m = _SIZE.match(line)
            if m and m.group(1) == cur:
                cur = None
            continue
        m = _SET.match(line)
        if m and m.group(1) in funcs:
            funcs[m.group(1)].append(line)
    return funcs


def compare(old: dict[str, list[str]], new: dict[str, list[str]]) -> list[tuple[str, str]]:
    """(symbol, verdict) for every symbol of either side, old's order first."""
    out = []
    for sym in list(old) + [s for s in new if s not in old]:
        if sym not in new:
            out.append((sym, "only in old"))
        elif sym not in old:
            out.append((sym, "only in new"))
        elif old[sym] == new[sym]:
            out.append((sym, f"IDENTICAL ({len(new[sym])} lines)"))
        else:
            out.append((sym, "DIFFERENT"))
    return out


def allowed(name: str, allow: list[str]) -> bool:
    return any(a == name or a == name.split("(", 1)[0] for a in allow)


def demangle(syms: list[str]) -> dict[str, str]:
    if not syms:
        return {}
    try:
        r = subprocess.run(["c++filt"], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True)
        names = r.stdout.splitlines()
        if len(names) == len(syms):
            return dict(zip(syms, names))
    except (OSError, subprocess.CalledProcessError):
        pass
    return {s: s for s in syms}


def makefile_vars(tree: str) -> dict[str, str]:
    """HIPCC and HIPFLAGS as kingdb_amd/Makefile sets them, its own variables expanded."""
    here = os.path.join(os.path.abspath(tree), "kingdb_amd") + os.sep
    text = open(os.path.join(here, "Makefile")).read().replace("\\\n", " ")
    var = {"HERE": here}
    for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M):
        if m.group(1) in ("HIPCC", "ARCH", "CSRC", "HIPFLAGS"):
            var[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda v: var.get(v.group(1), ""), m.group(2)).strip()
    var["HIPCC"] = os.environ.get("HIPCC", var["HIPCC"])
    return var


def device_asm(tree: str, rel: str, out: str) -> str:
    var = makefile_vars(tree)
    src = os.path.join(tree, rel)
    if not os.path.exists(src):
        src = os.path.join(tree, "kingdb_amd", "csrc", rel)
    r = subprocess.run([var["HIPCC"], *var["HIPFLAGS"].split(), "--cuda-device-only", "-S", src, "-o", out],
                       capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"{src}: the compiler failed\n{r.stderr}")
    return open(out).read()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("files", nargs="+", metavar="FILE.hip")
    ap.add_argument("--allow", action="append", default=[], metavar="NAME",
                    help="a function that may be DIFFERENT (repeatable)")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for rel in a.files:
            old = split_functions(device_asm(a.old_tree, rel, os.path.join(tmp, "old.s")))
            new = split_functions(device_asm(a.new_tree, rel, os.path.join(tmp, "new.s")))
            verdicts = compare(old, new)
            names = demangle([s for s, _ in verdicts])
            print(f"== {rel}: {len(old)} functions in old, {len(new)} in new")
            for sym, verdict in verdicts:
                ok = verdict != "DIFFERENT" or allowed(names[sym], a.allow)
                bad += 0 if ok else 1
                print(f"{verdict + (' (allowed)' if verdict == 'DIFFERENT' and ok else ''):<24} {names[sym]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
