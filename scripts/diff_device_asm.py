#!/usr/bin/env python3
"""Compare two directories of gfx950 device assembly, symbol by symbol.

  diff_device_asm.py PARENT_DIR NEW_DIR unit [unit ...]

Each directory holds, per translation unit, `unit.s` (hipcc --cuda-device-only
-S) and `unit.usage` (the stderr of -Rpass-analysis=kernel-resource-usage).
Comment lines and trailing "; ..." comments are dropped, the __hip_cuid_<hash>
symbol is replaced by one name, the text is cut at the symbol labels up to
their .Lfunc_end, and the instruction lines of every symbol, the text outside
the symbols and the resource-usage remarks (file:line:column prefix removed)
are compared.  Prints the record in the format of
profiles/buffer_refactor_isa.txt; exit status 1 on any difference.
"""
import re
import subprocess
import sys
from pathlib import Path

LISTED = re.compile(r"^(void )?ogbx::")  # kernels of the project; library instantiations are counted only


def clean(path):
    out = []
    for line in Path(path).read_text().splitlines():
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        out.append(re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line))
    return out


def split(lines):
    """-> ({symbol: lines}, lines outside symbols, set of kernel symbols)"""
    syms, outside, cur, name = {}, [], None, None
    kernels = {m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):$", l)
        if cur is None and m and not m.group(1).startswith(".L"):
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if re.match(r"^\.Lfunc_end\d+:$", l):
                syms[name] = cur
                cur = None
            else:
                cur.append(l)
            continue
        outside.append(l)
    return syms, outside, kernels


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, r))


def short(d):
    d = re.sub(r"\(.*$", "", d.replace("(anonymous namespace)", "{anonymous}"))  # drop the parameter list
    return d


def usage(path):
    p = Path(path)
    if not p.exists():
        return []
    # the remarks alone: the quoted source line under each carries its line number
    return [re.sub(r"^\S+?:\d+:\d+: ", "", l) for l in p.read_text().splitlines() if "remark:" in l]


def main():
    parent, new, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    same = True
    for u in units:
        ps, po, pk = split(clean(f"{parent}/{u}.s"))
        ns, no, nk = split(clean(f"{new}/{u}.s"))
        names = sorted(set(ps) | set(ns))
        dm = demangle(names)
        kernels = [n for n in names if n in pk or n in nk]
        print(f"== {u}.hip: {len(kernels)} kernels, {len(names) - len(kernels)} other symbols")
        for n in sorted(names, key=lambda n: short(dm[n])):
            a, b = ps.get(n), ns.get(n)
            eq = a == b
            same = same and eq
            if eq and not LISTED.search(dm[n]):
                continue
            word = "identical" if eq else ("DIFFERENT" if a is not None and b is not None else "MISSING  ")
            print(f"   {word}  {len(a or []):5d} /  {len(b or []):5d} lines  {short(dm[n])}")
        eq = po == no
        same = same and eq
        print(f"   outside kernels (metadata, directives): {'identical' if eq else 'DIFFERENT'}")
        pu, nu = usage(f"{parent}/{u}.usage"), usage(f"{new}/{u}.usage")
        eq = pu == nu
        same = same and eq
        print(f"   kernel-resource-usage remarks ({len(nu)} lines): {'identical' if eq else 'DIFFERENT'}")
    print("ALL IDENTICAL" if same else "DIFFERENCES FOUND")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
