#!/usr/bin/env python3
"""Compare the gfx950 device assembly of HIP libraries between two trees, kernel by kernel (DESIGN sections 24 and 36).

    tools/isa_compare.py BEFORE_TREE AFTER_TREE LIB [LIB ...]

Builds `isa-LIB` in each tree through that tree's own prosstt_amd/csrc/Makefile (the library's compile line with
-save-temps; cross-compiles without a GPU) and prints one line per kernel: its class, the number of differing lines, and
VGPRs / SGPRs / LDS bytes.  A kernel's text is what lies between its label and its last s_endpgm, without comments and
with .LBB<n>_ read as .LBB_; its metadata are vgpr_count, sgpr_count, agpr_count, the LDS and scratch sizes and both
spill counts.  The classes, each with equal metadata:

    identical             the same text
    outside loops (n)     all n differing lines lie before the first target of a backward branch or after the last
                          backward branch
    renamed scalars (n)   line for line the same opcodes, vector registers, literals and labels; the texts become equal
                          under ONE one-to-one renaming of scalar registers s<k> (vcc, exec, m0 and every v and a
                          register must stand as they are)

Exits 1 when a kernel is in none of them, or is missing from one tree.  It reads text and numbers only and looks for no
particular instruction.
"""
import difflib
import os
import re
import subprocess
import sys
import tempfile

META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "vgpr_spill_count", "sgpr_spill_count")


def assembly(tree, lib):
    with tempfile.TemporaryDirectory(prefix="isa_compare_%s_" % lib) as tmp:
        subprocess.check_call(["make", "-C", os.path.join(tree, "prosstt_amd", "csrc"), "isa-" + lib, "ISA_DIR=" + tmp],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        with open(os.path.join(tmp, lib + ".s")) as f:
            return f.read()


def kernels(text):
    """{name: (lines, metadata)} of every kernel of a device assembly file."""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        blk = ".agpr_count" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1)) for key in META}
        m = re.search(r"^%s:[^\n]*\n(.*?)\n\.Lfunc_end" % re.escape(name), text, re.S | re.M)
        body = m.group(1)
        body = body[:body.rindex("s_endpgm") + len("s_endpgm")]
        lines = []
        for line in body.split("\n"):
            line = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", re.sub(r";.*|//.*", "", line)).strip())
            if line:
                lines.append(line)
        out[name] = (lines, meta)
    return out


def loop_span(lines):
    """(first, last): the line of the first target of a backward branch and the line of the last backward branch; None
    without a loop."""
    at = {line[:-1]: i for i, line in enumerate(lines) if line.endswith(":")}
    first = last = None
    for i, line in enumerate(lines):
        m = re.match(r"s_c?branch\w* (\S+)$", line)
        if m and m.group(1) in at and at[m.group(1)] <= i:
            first = at[m.group(1)] if first is None else min(first, at[m.group(1)])
            last = i
    return None if first is None else (first, last)


def differing(before, after):
    """The indices of the lines of each text that the other does not have in their place."""
    b, a = [], []
    for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, before, after, autojunk=False).get_opcodes():
        if tag != "equal":
            b.extend(range(i0, i1))
            a.extend(range(j0, j1))
    return b, a


SCALAR = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def scalars(line):
    """The line with every scalar register replaced by a place holder, and the registers in order (a range as its
    members)."""
    regs = []

    def note(m):
        if m.group(1) is not None:
            regs.append(int(m.group(1)))
            return "s#"
        lo, hi = int(m.group(2)), int(m.group(3))
        regs.extend(range(lo, hi + 1))
        return "s[#%d]" % (hi - lo + 1)
    return SCALAR.sub(note, line), regs


def renamed_scalars(before, after):
    """How many lines differ if one one-to-one renaming of scalar registers makes the texts equal, else None."""
    if len(before) != len(after):
        return None
    forth, back, n = {}, {}, 0
    for x, y in zip(before, after):
        (sx, rx), (sy, ry) = scalars(x), scalars(y)
        if sx != sy:
            return None
        for r, s in zip(rx, ry):
            if forth.setdefault(r, s) != s or back.setdefault(s, r) != r:
                return None
        n += x != y
    return n


def classify(before, after):
    """(class or None, n, note)."""
    (bl, bm), (al, am) = before, after
    if bm != am:
        return None, 0, "metadata differ: %s -> %s" % (bm, am)
    if bl == al:
        return "identical", 0, ""
    db, da = differing(bl, al)
    n = max(len(db), len(da))
    inside = []
    for lines, diff in ((bl, db), (al, da)):
        span = loop_span(lines)
        inside.append(0 if span is None else sum(span[0] <= i <= span[1] for i in diff))
    if inside == [0, 0]:
        return "outside loops", n, ""
    note = "%d / %d lines differ, %d / %d inside loops" % (len(db), len(da), inside[0], inside[1])
    r = renamed_scalars(bl, al)
    if r is not None:
        return "renamed scalars", r, note
    return None, n, note + "; %d -> %d lines" % (len(bl), len(al))


def main(argv):
    if len(argv) < 4:
        sys.stderr.write(__doc__)
        return 2
    before_tree, after_tree, libs = argv[1], argv[2], argv[3:]
    bad = 0
    for lib in libs:
        before, after = kernels(assembly(before_tree, lib)), kernels(assembly(after_tree, lib))
        for name in sorted(set(before) | set(after)):
            if name not in before or name not in after:
                print("%-8s %s  MISSING %s" % (lib, name, "before" if name not in before else "after"))
                bad += 1
                continue
            cls, n, note = classify(before[name], after[name])
            meta = after[name][1]
            triple = "%d / %d / %d" % (meta["vgpr_count"], meta["sgpr_count"], meta["group_segment_fixed_size"])
            if cls is None:
                bad += 1
                print("%-8s %s  NONE (%d)  %s  [%s]" % (lib, name, n, triple, note))
            elif cls == "identical":
                print("%-8s %s  identical (%d lines)  %s" % (lib, name, len(after[name][0]), triple))
            else:
                print("%-8s %s  %s (%d)  %s%s" % (lib, name, cls, n, triple, "  [%s]" % note if note else ""))
    print("%s" % ("every kernel is in an accepted class" if not bad else "%d kernels are in no accepted class" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
