"""Development tool: which kernel instances one run of tests/test_row_instances_gpu.py launched, set against the expected-instance
table of tests/row_pass_cases.py.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python -m pytest -m gpu tests/test_row_instances_gpu.py -v > LOG 2>&1
    python tools/row_instances_profile.py DIR [--log LOG] [--out profiles/row_instances_kernels.txt]

(The traced run stands alone: no counters with it.)  Reads every *kernel_stats.csv below DIR (distinct kernel names with their call
counts), writes the report and exits with status 1 when an instance of the table never ran or a row_kernel instance of SDDMM / SpMM /
fused ran that the table does not name."""
import argparse
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OPS = {0: "SDDMM", 1: "SpMM", 2: "fused"}


def kernel_calls(directory):
    calls = {}
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        sys.exit("no *kernel_stats.csv below %s" % directory)
    for path in files:
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                row = {k.strip().lower(): v for k, v in row.items()}
                calls[row["name"]] = calls.get(row["name"], 0) + int(row["calls"])
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_instances_kernels.txt"))
    a = ap.parse_args()
    import row_pass_cases as RC

    calls = kernel_calls(a.directory)
    table = RC.expected_table()
    by_args = {"row": {}, "long": {}}  # template arguments -> calls
    for name, n in calls.items():
        m = re.search(r"(long_)?row_kernel<([^<>]*)>", name)
        if m and "max_row" not in name:
            d = by_args["long" if m.group(1) else "row"]
            d[m.group(2)] = d.get(m.group(2), 0) + n
    lines = ["Kernel instances launched by one run of tests/test_row_instances_gpu.py under a kernel trace, against the expected-instance table",
             "(tests/row_pass_cases.py: expected_table).  Template arguments: OP (0 SDDMM, 1 SpMM, 2 fused), LPR, VEC, W, EXACT, NARROW.", ""]
    if a.log:
        with open(a.log) as f:
            tail = [ln.rstrip() for ln in f if re.search(r"\b(passed|failed|error)\b.* in [0-9.]+s", ln)]
        lines += ["pytest: " + t.strip("= ") for t in tail[-1:]] + [""]
    missing, extra = [], []
    for op in sorted(OPS):
        lines.append("%s: %d instances in the table" % (OPS[op], sum(1 for i in table if i[0] == op)))
        lines.append("  %-34s %10s %16s   reached by (first cases)" % ("LPR, VEC, W, EXACT, NARROW", "row_kernel", "long_row_kernel"))
        for inst in sorted(i for i in table if i[0] == op):
            key = RC.instance_name(inst)
            n = by_args["row"].get(key, 0)
            if n == 0:
                missing.append(inst)
            lines.append("  %-34s %10d %16d   %s" % (key.split(", ", 1)[1], n, by_args["long"].get(key, 0), "; ".join(table[inst][:2])))
        lines.append("")
    named = {RC.instance_name(i) for i in table}
    for key, n in sorted(by_args["row"].items()):
        if re.match(r"\(\(anonymous namespace\)::Op\)[012],", key) and key not in named:
            extra.append((key, n))
    lines.append("in the table, never launched: %s" % (", ".join(RC.instance_name(i) for i in missing) or "none"))
    lines.append("launched, not in the table: %s" % (", ".join("%s (%d)" % e for e in extra) or "none"))
    lines += ["launch_shape instances that no public call of the three passes reaches at these sizes: none.  The wide exact SDDMM / SpMM instances",
              "(32, 5) (64, 3) (32, 7) (64, 4) run only under HNH_WIDE_SLABS=0 (128-column slabs replace them by default); the Op 3 (CG / ReLU-delivery",
              "epilogue) and Op 4 (softmax) instances belong to test_kernels_gpu.py and test_attention_instances_gpu.py."]
    lines += ["", "other kernels of the run:"]
    for name, n in sorted(calls.items()):
        if not re.search(r"(long_)?row_kernel<", name) or "max_row" in name:
            lines.append("  %8d  %s" % (n, name))
    for wdt in (1, 2):
        if not any(re.search(r"reduce_long_kernel<%d>" % wdt, k) for k in calls):
            missing.append("reduce_long_kernel<%d>" % wdt)
            lines.append("reduce_long_kernel<%d> never ran" % wdt)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if (missing or extra) else 0)


if __name__ == "__main__":
    main()
