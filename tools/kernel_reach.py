#!/usr/bin/env python3
"""Which compiled kernel instantiations a set of runs launched.

usage: python tools/kernel_reach.py [--names FILE] [--notes FILE] [--units UNIT[,UNIT..]]
                                    [--require UNIT[,UNIT..]] [LABEL=]STATS.csv ...

The instantiations are tools/kres.py's list (every kernel hipcc emits for the
translation units; nothing is compiled for or started on a GPU), or with
--names a hand-written one: a line per kernel, `unit name`.  Each CSV is a
`rocprofv3 --kernel-trace --stats` kernel_stats file, or any CSV with the
columns Name and Calls; only those two are read, and Test where a CSV has it.
A row counts for the test its Test column names, else for the CSV's LABEL
(default: the file name).  Kernel names are compared as kres prints them, so
trace the runs without rocprofv3's -T, which cuts the template arguments off.

One tab-separated line per instantiation: unit, name, launches, the first
test that reached it (`-` for none; with --notes FILE, lines of `name<TAB>how
to select it`, the note of an unreached kernel follows).  Kernels of the CSVs
that are no instantiation of ours (the runtime's, torch's) are ignored.
--units: list these translation units only.  --require: exit status 1 when a
kernel of one of these units has no launch."""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kres  # noqa: E402


def read_names(path):
    rows = {}
    for ln in open(path):
        ln = ln.strip()
        if ln and not ln.startswith("#"):
            unit, name = ln.split(None, 1)
            rows[kres.kernel_name(name)] = {"unit": unit}
    return rows


def read_stats(path, label):
    """[(kernel name, calls, test)] of one CSV, in file order."""
    out = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("Kernel_Name")
            if name:
                out.append((kres.kernel_name(name), int(r["Calls"]), r.get("Test") or label))
    return out


def reach(kernels, stats):
    """{name: [launches, first test or None]} over the instantiations."""
    seen = {name: [0, None] for name in kernels}
    for name, calls, test in stats:
        if name in seen and calls > 0:
            seen[name][0] += calls
            if seen[name][1] is None:
                seen[name][1] = test
    return seen


def main(argv):
    names = notes = None
    units, require, csvs = None, [], []
    it = iter(argv)
    for a in it:
        if a == "--names":
            names = next(it)
        elif a == "--notes":
            notes = next(it)
        elif a == "--units":
            units = next(it).split(",")
        elif a == "--require":
            require = next(it).split(",")
        else:
            label, _, path = a.rpartition("=")
            csvs.append((path, label or os.path.basename(path)))
    kernels = read_names(names) if names else kres.compiled_kernels()
    if units:
        kernels = {k: v for k, v in kernels.items() if v["unit"] in units}
    how = {}
    if notes:
        for ln in open(notes):
            if "\t" in ln and not ln.startswith("#"):
                k, v = ln.rstrip("\n").split("\t", 1)
                how[kres.kernel_name(k)] = v
    seen = reach(kernels, [row for path, label in csvs for row in read_stats(path, label)])
    missing = 0
    print("# unit\tkernel\tlaunches\tfirst test to launch it" + ("\thow to select it (unreached)" if notes else ""))
    for name, (calls, test) in seen.items():
        unit = kernels[name]["unit"]
        cols = [unit, name, str(calls), test or "-"]
        if not calls and name in how:
            cols.append(how[name])
        print("\t".join(cols))
        missing += (not calls) and unit in require
    unreached = sum(1 for c, _ in seen.values() if not c)
    print(f"# {len(seen)} instantiations, {unreached} without a launch")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
