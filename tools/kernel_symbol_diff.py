#!/usr/bin/env python3
"""Per-symbol disassembly diff of the gfx950 code objects of two builds of a library:

    tools/kernel_symbol_diff.py OLD/libhevcdbk.so NEW/libhevcdbk.so [--json out.json]

For every kernel symbol of OLD: identical in NEW, missing, or the instructions that differ.  A change that adds kernels under new
names must leave every old symbol identical up to PC-relative offsets to tables that moved (the literal of the s_add_u32 /
s_addc_u32 pair behind an s_getpc_b64); those are counted apart.  Exit status 1 when an old symbol is missing or differs otherwise.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

from check_store_hazard import OBJDUMP, code_objects


def functions(path):
    """{symbol: [instruction text]} over every gfx950 code object of the file"""
    out = {}
    for co in code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".elf") as tmp:
            tmp.write(co)
            tmp.flush()
            txt = subprocess.check_output([OBJDUMP, "-d", "--symbolize-operands", tmp.name], stderr=subprocess.DEVNULL).decode(errors="replace")
        func = None
        for ln in txt.split("\n"):
            m = re.match(r"^[0-9a-f]{8,16} <([^>]+)>:$", ln.strip())
            if m:
                if not re.match(r"^L\d+$", m.group(1)):
                    func = m.group(1)
                    out.setdefault(func, [])
                else:
                    out[func].append(m.group(1) + ":")
                continue
            if func is None or not ln[:1].isspace():
                continue
            t = ln.split("//")[0].strip()
            if t:
                out[func].append(t)
    # objdump marks a run of zero bytes with "...": as the LAST line of a function that is the padding behind it, which depends on what
    # the linker places next, and is dropped; anywhere else it stays and is compared
    for ins in out.values():
        while ins and ins[-1] == "...":
            ins.pop()
    return {f: relabel(ins) for f, ins in out.items()}


def relabel(ins):
    """objdump numbers its branch labels through the whole code object: renumber them per function, in order of appearance"""
    names = {}
    for t in ins:
        for lab in re.findall(r"\bL\d+\b", t):
            names.setdefault(lab, "L%d" % len(names))
    return [re.sub(r"\bL\d+\b", lambda m: names[m.group(0)], t) for t in ins]


def pc_relative_only(a, b):
    """the two listings differ only in literals of s_add_u32 / s_addc_u32 (offsets from s_getpc_b64 to a table)"""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x == y:
            continue
        ox, oy = x.split(None, 1), y.split(None, 1)
        if ox[0] != oy[0] or ox[0] not in ("s_add_u32", "s_addc_u32"):
            return False
        if [t.strip() for t in ox[1].split(",")][:2] != [t.strip() for t in oy[1].split(",")][:2]:
            return False
    return True


def main(argv):
    js = None
    if "--json" in argv:
        i = argv.index("--json")
        js = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    old, new = functions(argv[1]), functions(argv[2])
    res = {"old": "parent build of " + os.path.basename(argv[1]), "new": "this build of " + os.path.basename(argv[2]), "old_symbols": len(old), "new_symbols": len(new), "identical": 0, "pc_relative_only": [],
           "missing": [], "different": {}, "added": sorted(set(new) - set(old))}
    for name, ins in sorted(old.items()):
        if name not in new:
            res["missing"].append(name)
        elif new[name] == ins:
            res["identical"] += 1
        elif pc_relative_only(ins, new[name]):
            res["pc_relative_only"].append(name)
        else:
            res["different"][name] = {"old_instructions": len(ins), "new_instructions": len(new[name])}
    print("%s -> %s: %d old symbols: %d identical, %d PC-relative offsets only, %d missing, %d different; %d added" %
          (argv[1], argv[2], len(old), res["identical"], len(res["pc_relative_only"]), len(res["missing"]), len(res["different"]),
           len(res["added"])))
    for n in res["missing"]:
        print("  missing:", n)
    for n, d in res["different"].items():
        print("  different:", n, d)
    if js:
        with open(js, "w") as f:
            json.dump(res, f, indent=1)
    return 1 if res["missing"] or res["different"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
