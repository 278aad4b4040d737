#!/usr/bin/env python3
"""Are two builds the same device code?  Compares the gfx950 assembly that the Makefile keeps (csrc/build/*-gfx950.s) of two trees.

The instruction stream of an object is its assembly with everything from ';' to the end of each line removed, and trailing blanks
removed as well (the comments carry basic-block names such as %if.then.i, which change with the inlining depth and with nothing
else).  Two objects are the same when their streams are byte-identical; the files are compared as text, whole.

For every *-gfx950.s present in either directory a line SAME or DIFF is printed; a DIFF is followed by the kernel symbols whose
streams differ, with both instruction counts.  Exit status 1 on any DIFF or on a file that one side lacks.

Usage: isa_equal.py A/build B/build"""
import glob
import os
import re
import sys

SYMBOL = re.compile(r"^([A-Za-z_][\w$.]*):")
LOCAL = re.compile(r"\.L(BB|func_begin|func_end)\d+_?")
OUTSIDE = "(outside any function)"


def stream(text):
    """The instruction stream: comments and trailing blanks removed, line by line."""
    return [ln.split(";", 1)[0].rstrip() for ln in text.split("\n")]


def functions(lines):
    """{symbol: its lines} of a stream.  A function runs from its symbol label (the same labels check_kernel_resources.py and
    asm_mix.py key on; local labels start with '.') to its .Lfunc_end; whatever stands between functions is kept under OUTSIDE."""
    out, cur = {OUTSIDE: []}, OUTSIDE
    for ln in lines:
        m = SYMBOL.match(ln)
        if m and cur == OUTSIDE:
            cur = m.group(1)
            out.setdefault(cur, [])
        out[cur].append(ln)
        if ln.startswith(".Lfunc_end"):
            cur = OUTSIDE
    return out


def instructions(lines):
    n = 0
    for ln in lines:
        t = ln.strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            n += 1
    return n


def compare(a_text, b_text):
    """[] when the two streams are identical, else [(symbol, instructions in a, instructions in b)] of the functions that differ
    (None for a function that one side lacks)."""
    a, b = stream(a_text), stream(b_text)
    if a == b:
        return []
    # a function's local labels carry its index in the file (.LBB3_12): without it a function is not blamed for another one's arrival
    fa, fb = functions([LOCAL.sub(r".L\1_", ln) for ln in a]), functions([LOCAL.sub(r".L\1_", ln) for ln in b])
    diffs = []
    for name in list(fa) + [n for n in fb if n not in fa]:
        la, lb = fa.get(name), fb.get(name)
        if la != lb:
            diffs.append((name, None if la is None else instructions(la), None if lb is None else instructions(lb)))
    return diffs or [(OUTSIDE, instructions(a), instructions(b))]


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    da, db = argv[1], argv[2]
    names = sorted({os.path.basename(p) for d in (da, db) for p in glob.glob(os.path.join(d, "*-gfx950.s"))})
    bad = 0 if names else 1
    if not names:
        print("no *-gfx950.s in either directory")
    for name in names:
        pa, pb = os.path.join(da, name), os.path.join(db, name)
        missing = [d for d, p in ((da, pa), (db, pb)) if not os.path.exists(p)]
        if missing:
            print("MISSING %s in %s" % (name, missing[0]))
            bad += 1
            continue
        with open(pa) as f:
            ta = f.read()
        with open(pb) as f:
            tb = f.read()
        diffs = compare(ta, tb)
        print("%s %s" % ("DIFF" if diffs else "SAME", name))
        for sym, na, nb in diffs:
            print("     %s: %s -> %s instructions" % (sym, "absent" if na is None else na, "absent" if nb is None else nb))
        bad += 1 if diffs else 0
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
