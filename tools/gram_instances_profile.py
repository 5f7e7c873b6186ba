"""Development tool: which gram_rows_kernel instances one run of tests/test_gram_instances_gpu.py launched, set against the table of
tests/gram_cases.py.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python -m pytest -m gpu tests/test_gram_instances_gpu.py \
        -k "exact or bit_for_bit or refusals" -v > LOG 2>&1
    python tools/gram_instances_profile.py DIR [--log LOG] [--out profiles/gram_instances_kernels.txt]

(The traced run stands alone: no counters with it.  -k keeps the kernel tests: the operator cases run on loopback rank threads, and a
traced run of the whole file once ended in a segmentation fault of the host process there)  Reads every *kernel_stats.csv
below DIR (distinct kernel names with their call counts), writes the report and exits with status 1 when one of the five instances never
ran or ran less often than the table asks for (four launches per case with rows > 0; operator cases, if traced, add theirs)."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gram_instances_kernels.txt"))
    a = ap.parse_args()
    import gram_cases as G
    from row_instances_profile import kernel_calls

    calls = kernel_calls(a.directory)
    ran = {}
    for name, n in calls.items():
        m = re.search(r"gram_rows_kernel<\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*>", name)
        if m:
            inst = tuple(int(x) for x in m.groups())
            ran[inst] = ran.get(inst, 0) + n
    expected = G.expected_launches()
    lines = ["Kernel instances launched by one run of tests/test_gram_instances_gpu.py under a kernel trace, against the case table of",
             "tests/gram_cases.py (expected_launches: four launches per kernel case with rows > 0; the file's operator cases add theirs).", ""]
    if a.log:
        with open(a.log) as f:
            tail = [ln.rstrip() for ln in f if re.search(r"\b(passed|failed|error)\b.* in [0-9.]+s", ln)]
        lines += ["pytest: " + t.strip("= ") for t in tail[-1:]] + [""]
    lines.append("  %-28s %8s %10s %10s   load widths of X in the table's cases" % ("gram_rows_kernel<NJ, MI, WAVES>", "R <=", "launched", "table"))
    missing, short = [], []
    for top, inst in sorted(G.INSTANCES.items()):
        n = ran.get(inst, 0)
        if n == 0:
            missing.append(inst)
        elif n < expected[inst]:
            short.append(inst)
        vec = sorted({G.instance_of(R, xs == 0)[3] for rows, R, xs, _ in G.CASES if rows and G.instance_of(R, True)[:3] == inst})
        lines.append("  %-28s %8d %10d %10d   %s" % ("<%d, %d, %d>" % inst, top, n, expected[inst], ", ".join("16-byte" if v else "8-byte" for v in vec)))
    lines += ["", "never launched: %s" % (", ".join("<%d, %d, %d>" % i for i in missing) or "none"),
              "launched less often than the table's cases ask for: %s" % (", ".join("<%d, %d, %d>" % i for i in short) or "none"),
              "launched, not among the five: %s" % (", ".join("<%d, %d, %d> (%d)" % (i + (n,)) for i, n in sorted(ran.items()) if i not in expected) or "none")]
    lines += ["", "other kernels of the run:"]
    for name, n in sorted(calls.items()):
        if "gram_rows_kernel<" not in name:
            lines.append("  %8d  %s" % (n, name))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if (missing or short) else 0)


if __name__ == "__main__":
    main()
