#!/usr/bin/env python3
"""Are the kernels of two builds the same? Per __global__ entry point: the instruction text and the resources.

    python tools/kernel_identity.py FIRST SECOND [--diffs 3] [--jobs 8]

FIRST and SECOND are each a source tree (its gpu-raytracer_amd/Makefile has the `asm` target: every unit's device-only assembly, csrc/<unit>.s,
compiled with the unit's own flags; it is made or brought up to date here) or a directory of such <unit>.s files made elsewhere.

"Every kernel of the parent compiles to the same text with the same resources" is how this project shows that a change costs nothing when it is
switched off, or that a refactor moved code and changed none. An entry point is matched by its symbol name across whatever units
it lives in, so a kernel may move between units. Compared per entry point:
  text       the lines from the symbol's label to its .Lfunc_end, comments dropped, runs of blanks made one, and the local labels (.LBB<function>_<block>,
             .Ltmp<n>, ...) renumbered in order of first appearance: the function's index in its unit is part of their names and says nothing.
  resources  the kernel descriptor's directives (.amdhsa_*: next free VGPR / SGPR, accumulator offset, LDS and scratch bytes, ...) and the scalar
             fields of the kernel's metadata record (VGPRs, AGPRs, SGPRs, LDS bytes, scratch bytes, spill counts, kernarg size, workgroup size).
It only diffs: it looks for no instruction in particular. Data outside function bodies (a jump table in .rodata) is not compared.

Prints one line per entry point of FIRST, a unified diff of the first --diffs differing ones, the symbols present on one side only and a summary.
Exit status 0 only if every entry point of FIRST is present in SECOND and identical there."""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys

LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


class Kernel:
    def __init__(self, unit, text, resources):
        self.unit, self.text, self.resources = unit, text, resources


def normalise(lines):
    """The comparable text of a function body: no comments, single blanks, local labels numbered by first appearance."""
    names = {}
    out = []
    for line in lines:
        line = " ".join(line.split(";", 1)[0].split())
        if not line:
            continue
        out.append(LOCAL_LABEL.sub(lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), line))
    return out


def parse(text, unit):
    """{symbol: Kernel} of one unit's assembly."""
    lines = text.split("\n")
    kernels, labels = {}, {}
    for i, line in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w.$]*):", line)
        if m:
            labels[m.group(1)] = i
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        symbol = m.group(1)
        start = labels[symbol]
        end = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
        close = next(k for k in range(i, end) if lines[k].strip() == ".end_amdhsa_kernel")
        resources = {}
        for d in lines[i + 1:close]:
            key, _, value = d.strip().partition(" ")
            resources[key] = value.strip()
        kernels[symbol] = Kernel(unit, normalise(lines[start:i] + lines[close + 1:end]), resources)
    # the metadata records: a list item per kernel under amdhsa.kernels, its scalar fields at four blanks of indent
    record = None
    for line in lines + ["  - ."]:
        if re.match(r"  - \.\w+:", line) or not line.startswith("  "):
            if record and record.get(".name") in kernels:
                kernels[record[".name"]].resources.update((k, v) for k, v in record.items() if k not in (".name", ".symbol") and v != "")
            record = {} if line.startswith("  - .") else None
        m = re.match(r"(?:  - |    )(\.\w+):\s*(.*)$", line)
        if m and record is not None:
            record[m.group(1)] = m.group(2).strip()
    return kernels


def load(path, jobs):
    """{symbol: Kernel} of a source tree (assembly made by its Makefile) or of a directory of <unit>.s files."""
    makefile_dir = os.path.join(path, "gpu-raytracer_amd")
    if os.path.exists(os.path.join(makefile_dir, "Makefile")):
        subprocess.run(["make", "-C", makefile_dir, "-j%d" % jobs, "asm"], check=True, stdout=subprocess.DEVNULL)
        path = os.path.join(makefile_dir, "csrc")
    kernels = {}
    for name in sorted(glob.glob(os.path.join(path, "*.s"))):
        unit = os.path.basename(name)[:-2]
        for symbol, kernel in parse(open(name).read(), unit).items():
            if symbol in kernels:   # (an inline kernel two units instantiate: one text, or that is a difference of its own)
                first = kernels[symbol]
                if (first.text, first.resources) != (kernel.text, kernel.resources):
                    raise SystemExit("%s: %s differs between %s and %s of the same build" % (path, symbol, first.unit, unit))
                first.unit += "+" + unit
            else:
                kernels[symbol] = kernel
    if not kernels:
        raise SystemExit("%s: no entry point found (neither a tree with gpu-raytracer_amd/Makefile nor a directory of .s files?)" % path)
    return kernels


def compare(first, second, diffs=3, out=sys.stdout):
    """Prints the report; returns (identical, differing, only in first, only in second) as lists of symbols."""
    identical, differing = [], []
    only_first = sorted(s for s in first if s not in second)
    only_second = sorted(s for s in second if s not in first)
    shown = 0
    for symbol in sorted(first):
        if symbol not in second:
            continue
        a, b = first[symbol], second[symbol]
        what = []
        if a.text != b.text:
            what.append("text")
        changed = sorted(k for k in set(a.resources) | set(b.resources) if a.resources.get(k) != b.resources.get(k))
        if changed:
            what.append("resources: " + ", ".join("%s %s -> %s" % (k, a.resources.get(k, "-"), b.resources.get(k, "-")) for k in changed))
        units = a.unit if a.unit == b.unit else "%s -> %s" % (a.unit, b.unit)
        if not what:
            identical.append(symbol)
            print("identical  %-58s %s" % (units, symbol), file=out)
            continue
        differing.append(symbol)
        print("DIFFERS    %-58s %s  (%s)" % (units, symbol, "; ".join(what)), file=out)
        if a.text != b.text and shown < diffs:
            shown += 1
            for line in difflib.unified_diff(a.text, b.text, "%s (%s)" % (symbol, a.unit), "%s (%s)" % (symbol, b.unit), lineterm="", n=2):
                print("    " + line, file=out)
    for title, symbols, side in (("only in the first", only_first, first), ("only in the second", only_second, second)):
        print("%s: %d" % (title, len(symbols)), file=out)
        for symbol in symbols:
            print("    %-40s %s" % (side[symbol].unit, symbol), file=out)
    print("%d entry points in the first, %d in the second: %d identical in text and resources, %d differ, %d only in the first, %d only in the second"
          % (len(first), len(second), len(identical), len(differing), len(only_first), len(only_second)), file=out)
    return identical, differing, only_first, only_second


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--diffs", type=int, default=3, help="unified diffs shown, of the first entry points whose text differs")
    ap.add_argument("--jobs", type=int, default=8, help="make -j for a tree's assembly")
    a = ap.parse_args(argv)
    identical, differing, only_first, only_second = compare(load(a.first, a.jobs), load(a.second, a.jobs), a.diffs)
    return 1 if differing or only_first else 0


if __name__ == "__main__":
    sys.exit(main())
