#!/usr/bin/env python3
"""Are the kernels of two device-assembly files the same machine code?

    hipcc <the FLAGS of mod_extraction_amd/build.py> --cuda-device-only -S csrc/x.hip -o new.s      (same for the old tree)
    python tools/asm_same.py old.s new.s [old_name=new_name ...]

Per kernel present in both files it compares (a) the text between the kernel's label and its descriptor (which closes the
function, in front of .Lfunc_end<n>) and (b) its .amdhsa_* descriptor lines (registers, LDS, scratch).  Only what must differ
is normalised: the function index inside local labels (.LBB<n>_<m>, and BB<n>_<m> in the loop comments) and, for a kernel renamed by a shortened template list
(old_name=new_name, mangled), its own name.  Prints one line per kernel; exit status 1 if any kernel present in both differs or a mapped name is missing.
"""
import re
import sys


def kernels(path):
    """name -> (body lines, descriptor lines)"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        d0 = next(i for i in range(start, len(lines)) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", lines[i]))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        assert not any(re.match(r"\.Lfunc_end\d+:", ln) for ln in lines[start:d1]), name     # the descriptor closes the function
        body = [re.sub(r"(\.L|\b)BB\d+_", r"\1BB_", ln).replace(name, "KERNEL") for ln in lines[start + 1:d0]]
        out[name] = (body, [ln.strip() for ln in lines[d0 + 1:d1]])
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    rename = dict(a.split("=") for a in sys.argv[3:])
    bad = 0
    for name in old:
        to = rename.get(name, name)
        if to not in new:
            missing = name in rename
            bad += missing
            print(f"{'MISSING' if missing else 'removed':9s} {name}")
            continue
        same_body, same_desc = old[name][0] == new[to][0], old[name][1] == new[to][1]
        bad += not (same_body and same_desc)
        print(f"{'same' if same_body and same_desc else 'DIFFERENT':9s} {name}{' -> ' + to if to != name else ''}   "
              f"code {'same' if same_body else 'DIFFERENT'} ({len(old[name][0])} lines), descriptor {'same' if same_desc else 'DIFFERENT'}")
    for name in new:
        if name not in old and name not in rename.values():
            print(f"{'added':9s} {name}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
