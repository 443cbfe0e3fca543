#!/usr/bin/env python3
"""Compare the device code of two source trees: tools/isa_diff.py [--map REGEX=REPL] TREE_A TREE_B [UNIT.hip ...]
Compiles every .hip unit of the Makefile's SRCS in both trees with the Makefile's
flags plus --cuda-device-only -S, splits the assembly into functions and reports,
per unit, the symbols only in A, only in B, with a different body, or with a
different kernel descriptor (.amdhsa_kernel block: VGPR/SGPR, LDS, scratch).
Exit status 0 only if B equals A up to pure removals.  Text equality only.
--map REGEX=REPL rewrites tree A's assembly first: for a kernel whose mangled name moved (a
template parameter added) while its code is claimed unchanged."""
import re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = "nlp-filter_amd/csrc"


def recipe(tree):
    mk = (Path(tree) / CSRC / "Makefile").read_text()
    var = {k: re.search(rf"^{k} \??= (.*)$", mk, re.M).group(1) for k in ("HIPCC", "ARCH")}
    var.update(ROOT=str(Path(tree).resolve()), CSRC=str(Path(tree).resolve() / CSRC))
    flags = re.search(r"^FLAGS := (.*)$", mk, re.M).group(1)
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], flags)
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    return var["HIPCC"], flags.split(), srcs


def asm(tree, unit):
    hipcc, flags, _ = recipe(tree)
    cmd = [hipcc, *flags, "--cuda-device-only", "-S", "-o", "-", str(Path(tree) / CSRC / unit)]
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def split(text):
    """-> ({symbol: body}, {kernel: descriptor}), local labels normalised, comments stripped."""
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    funcs, desc, cur, kd = {}, {}, None, None
    for line in text.splitlines():
        if ".amdgpu_metadata" in line:
            break               # the YAML notes repeat the descriptors; no code follows
        line = re.sub(r"\s*;.*$", "", line).rstrip()
        if not line or re.match(r"\s*\.type\s+__hip_cuid_", line):
            continue            # (the per-unit source hash's .type line trails the symbol before it)
        m = re.match(r"\s*\.amdhsa_kernel (\S+)", line)
        if m:
            kd = m.group(1)
            desc[kd] = []
        elif kd is not None:
            if ".end_amdhsa_kernel" in line:
                kd = None
            else:
                desc[kd].append(line.strip())
        elif (m := re.match(r"([A-Za-z_$][\w$.]*):$", line)) and not line.startswith(".L"):
            cur = m.group(1)
            funcs[cur] = []
        elif re.match(r"\s*\.(section|text|rodata)\b", line):
            cur = None          # a function ends where the next section begins
        elif cur is not None:
            funcs[cur].append(line.strip())
    return funcs, desc


def main():
    argv, maps = sys.argv[1:], []
    while argv and argv[0] == "--map":
        maps.append(argv[1].split("=", 1))
        argv = argv[2:]
    a, b = argv[:2]
    units = argv[2:] or recipe(a)[2]

    def one(tu):
        text = asm(*tu)
        for pat, repl in (maps if tu[0] == a else []):
            text = re.sub(pat, repl, text)
        return split(text)
    with ThreadPoolExecutor(8) as ex:       # at most 8 compiles at a time
        outs = list(ex.map(one, [(t, u) for u in units for t in (a, b)]))
    bad = 0
    for i, u in enumerate(units):
        (fa, da), (fb, db) = outs[2 * i], outs[2 * i + 1]
        cuid = lambda s: s.startswith("__hip_cuid_")    # a per-unit hash of the source
        gone = sorted(s for s in set(fa) - set(fb) if not cuid(s))
        new = sorted(s for s in set(fb) - set(fa) if not cuid(s))
        body = sorted(s for s in set(fa) & set(fb) if fa[s] != fb[s])
        kdiff = sorted(k for k in set(da) & set(db) if da[k] != db[k])
        print(f"{u}: {len(fa)} symbols in A, {len(fb)} in B, {len(gone)} only in A, "
              f"{len(new)} only in B, {len(body)} bodies differ, {len(kdiff)} descriptors differ")
        for tag, names in (("-", gone), ("+", new), ("body", body), ("desc", kdiff)):
            for s in names:
                print(f"  {tag} {s}")
        for k in kdiff:
            for x, y in zip(da[k], db[k]):
                if x != y:
                    print(f"      {x}  ->  {y}")
        bad += len(new) + len(body) + len(kdiff)
    print("IDENTICAL up to removals" if not bad else f"DIFFERENT: {bad} symbols added or changed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
