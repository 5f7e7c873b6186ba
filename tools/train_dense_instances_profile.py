"""Development tool: which instances of the GAT's dense training kernels one run of tests/test_train_dense_instances_gpu.py launched,
set against what tests/train_dense_cases.py says the file must reach.

    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python -m pytest -m gpu tests/test_train_dense_instances_gpu.py -v > LOG 2>&1
    python tools/train_dense_instances_profile.py DIR [--log LOG] [--out profiles/train_dense_instances_kernels.txt]

(The traced run stands alone: no counters with it.)  Reads every *kernel_stats.csv below DIR (distinct kernel names with their call
counts), writes the report and exits with status 1 when an expected instantiation never ran."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def expected():
    import train_dense_cases as TD
    names = []
    for kernel in ("layernorm_fwd_kernel", "layernorm_bwd_kernel"):
        names += ["%s<%d, %d, %s>" % (kernel, w, t, "true" if block else "false") for w, t, block in TD.NORM_INSTANCES]
    for kernel in ("colsum_ranges_kernel", "act_grad_cols_kernel", "skip_grad_cols_kernel", "skip_addend_cols_kernel"):
        names += ["%s<%d>" % (kernel, w) for w in (1, 2)]
    names += ["optim_step_kernel<0>", "optim_step_kernel<1>", "optim_step_clip_kernel<0>", "optim_step_clip_kernel<1>", "optim_step_clip_kernel<2>"]
    return names + ["grad_sumsq_kernel", "grad_sumsq_finish_kernel", "layernorm_bwd_finish_kernel", "colsum_finish_kernel"]


def squeeze(name):
    """a demangled name without blanks and namespaces in front of the kernel, arguments cut off"""
    return re.sub(r"^void", "", re.sub(r"\s+", "", name.replace("(anonymous namespace)::", ""))).split("(")[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("directory")
    ap.add_argument("--log")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_dense_instances_kernels.txt"))
    a = ap.parse_args()
    from row_instances_profile import kernel_calls

    ran = {}
    for name, n in kernel_calls(a.directory).items():
        ran[squeeze(name)] = ran.get(squeeze(name), 0) + n
    lines = ["Kernel instantiations launched by one run of tests/test_train_dense_instances_gpu.py under a kernel trace (no counters), against",
             "the instances tests/train_dense_cases.py names (optimizer kinds: 0 Adam, 1 SGD, 2 AdamW).", ""]
    if a.log:
        with open(a.log) as f:
            tail = [ln.rstrip() for ln in f if re.search(r"\b(passed|failed|error)\b.* in [0-9.]+s", ln)]
        lines += ["pytest: " + t.strip("= ") for t in tail[-1:]] + [""]
    missing = []
    lines.append("  %10s  %s" % ("launched", "kernel"))
    want = expected()
    for name in want:
        n = ran.get(re.sub(r"\s+", "", name), 0)
        if n == 0:
            missing.append(name)
        lines.append("  %10d  %s" % (n, name))
    lines += ["", "never launched: %s" % (", ".join(missing) or "none"), "", "other kernels of the run:"]
    known = {re.sub(r"\s+", "", n) for n in want}
    for name, n in sorted(ran.items()):
        if name not in known:
            lines.append("  %10d  %s" % (n, name))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if missing else 0)


if __name__ == "__main__":
    main()
