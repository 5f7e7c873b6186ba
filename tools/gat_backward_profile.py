"""Development tool: time the GAT backward pass against its forward pass on one GPU, and the split-K weight-gradient GEMM alone.

    python tools/gat_backward_profile.py [logm] [alg] [--backward unfused|fused|both]
                                                               forward and backward ms per head (benchmark_dist.cpp:93-95 layers,
                                                               Erdos-Renyi 2^logm vertices, edge factor 32), then hnh_gemm_tn_f64
                                                               at 1024 x 1024 x 2^logm.  Backward mode "both" (the default; 15d_fusion2
                                                               only, 15d_fusion1 has the un-fused pass alone) times the un-fused and
                                                               the fused pass in the same run: both warmed up, then alternating, each
                                                               pass between two device synchronisations; mean and min .. max are printed
    python tools/gat_backward_profile.py --stats <dir>         the backward pass split into sparse passes, GEMMs and element-wise
                                                               kernels, from the *kernel_stats.csv of a run of this tool with
                                                               HNH_PROFILE_BACKWARD_ONLY=1 (and one --backward mode) under
                                                               `rocprofv3 --kernel-trace --stats`
"""
import csv, glob, os, re, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK = 78.6  # TFLOP/s, MI355X (v_mfma_f64_16x16x4_f64)


def stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit("no *kernel_stats.csv under %s" % d)
    groups = {}
    for f in files:
        for row in csv.DictReader(open(f)):
            name, ns, calls = row["Name"], float(row["TotalDurationNs"]), int(row["Calls"])
            ag = re.search(r"attn_grad_(row|long)_kernel<\s*(\d)", name)
            if ag:  # the two passes of the fused backward mode (include/hnh_attn_grad.h), hub-row segments with their pass
                g = "fused backward: column pass over S^T (packed gather)" if ag.group(2) == "1" else "fused backward: row pass over S"
            elif "attn_grad_reduce" in name:
                g = "fused backward: hub-row segment sums"
            elif "attn_grad_pack" in name:
                g = "fused backward: pack P = [A | dZ | lse delta]"
            elif "gemm_tn" in name:
                g = "TN GEMM (dW = X^T dA, split-K + reduce)"
            elif "gemm_f64" in name:
                g = "NN GEMM (A = X W, dX = dA W^T)"
            elif "row_kernel" in name or "long" in name or "hub" in name or "csr" in name or "spmm" in name or "sddmm" in name:
                g = "sparse passes (SDDMM / SpMM)"
            else:
                g = "element-wise, copies, reductions"
            t = groups.setdefault(g, [0.0, 0])
            t[0] += ns
            t[1] += calls
    total = sum(v[0] for v in groups.values())
    for g, (ns, calls) in sorted(groups.items(), key=lambda kv: -kv[1][0]):
        print("%-45s %9.1f ms  %5.1f %%  %6d launches" % (g, ns / 1e6, 100 * ns / total, calls))
    print("%-45s %9.1f ms" % ("all kernels", total / 1e6))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--stats":
        stats(sys.argv[2])
        return
    from distributed_sddmm_amd import api as H, _kernels as K
    assert H.load_backend(None) == "hip-gfx950"
    argv = list(sys.argv)
    backward = "both"
    if "--backward" in argv:
        i = argv.index("--backward")
        backward = argv[i + 1]
        del argv[i:i + 2]
    if backward not in ("unfused", "fused", "both"):
        sys.exit("--backward takes unfused, fused or both")
    logm = int(argv[1]) if len(argv) > 1 else 18
    algs = [argv[2]] if len(argv) > 2 else ["15d_fusion2", "15d_fusion1"]
    backward_only = os.environ.get("HNH_PROFILE_BACKWARD_ONLY") == "1"
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    for alg in algs:
        op = H.DistributedSparse(w, alg, sp, 256, 1)
        gnn = H.GAT(op, layers, 0.2)
        rng = np.random.default_rng(0)
        for li, (fin, fph, nh) in enumerate(layers):
            for h in range(nh):
                k, n = gnn.weight_shape(li, h)
                gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
        x = H.Dense.create(w, *gnn.buffer_shape(0))
        x.fill(0.01)
        gnn.set_input(x)
        g = H.Dense.create(w, *gnn.buffer_shape(len(layers)))
        g.fill(1.0)
        modes = ["unfused"] if alg != "15d_fusion2" else (["unfused", "fused"] if backward == "both" else [backward])
        gnn.forwardPass()
        for mode in modes:  # allocates each mode's buffers and warms it up
            gnn.set_backward(mode)
            gnn.backwardPass(g)
        w.sync()
        reps = 1 if backward_only else 3
        t = time.perf_counter()
        for _ in range(reps):
            gnn.forwardPass()
        w.sync()
        fwd = (time.perf_counter() - t) / reps
        times = {mode: [] for mode in modes}
        for _ in range(reps):  # alternating, every pass between two device synchronisations
            for mode in modes:
                gnn.set_backward(mode)
                w.sync()
                t = time.perf_counter()
                gnn.backwardPass(g)
                w.sync()
                times[mode].append(time.perf_counter() - t)
        for mode in modes:
            bwd = float(np.mean(times[mode]))
            print("GAT [%s, backward %s] 2^%d vertices, %d nnz, %d heads: forward %.1f ms (%.2f per head), backward %.1f ms (%.2f per head; "
                  "min %.1f .. max %.1f over %d), ratio %.2f"
                  % (alg, mode, logm, nnz, heads, fwd * 1e3, fwd * 1e3 / heads, bwd * 1e3, bwd * 1e3 / heads, min(times[mode]) * 1e3,
                     max(times[mode]) * 1e3, reps, bwd / fwd))
        if len(modes) == 2:
            u, f = float(np.mean(times["unfused"])), float(np.mean(times["fused"]))
            print("GAT [%s] un-fused / fused backward: %.2f x (%.1f -> %.1f ms)" % (alg, u / f, u * 1e3, f * 1e3))
        for h in (g, x, gnn, op):
            h.free()
    if backward_only:
        return
    ctx = K.Ctx(0)
    lib = ctx.lib
    M, N, Kd = 1024, 1024, 1 << logm
    need = lib.hnh_gemm_tn_f64_workspace(M, N, Kd)
    dA, dB = K.DevArray(ctx, (Kd, M), np.float64), K.DevArray(ctx, (Kd, N), np.float64)
    dC, work = K.DevArray(ctx, (M, N), np.float64), K.DevArray(ctx, max(need, 1), np.float64)
    lib.hnh_fill_f64(ctx.h, dA.ptr, Kd * M, 0.5, 0)
    lib.hnh_fill_f64(ctx.h, dB.ptr, Kd * N, 0.25, 0)
    ctx.check(lib.hnh_gemm_tn_f64(ctx.h, M, N, Kd, dA.ptr, M, dB.ptr, N, dC.ptr, N, work.ptr, need, 0), "gemm_tn")
    ctx.sync()
    reps = 10
    t = time.perf_counter()
    for _ in range(reps):
        lib.hnh_gemm_tn_f64(ctx.h, M, N, Kd, dA.ptr, M, dB.ptr, N, dC.ptr, N, work.ptr, need, 0)
    ctx.sync()
    dt = (time.perf_counter() - t) / reps
    tf = 2.0 * M * N * Kd / dt / 1e12
    print("gemm_tn_f64 %d x %d from K = %d (%d slices): %.2f ms -> %.1f TFLOP/s = %.0f %% of the fp64 matrix peak (%.1f)"
          % (M, N, Kd, need // (M * N) if need else 1, dt * 1e3, tf, 100 * tf / FP64_MATRIX_PEAK, FP64_MATRIX_PEAK))
    M2, K2, N2 = 1 << logm, 1024, 1024
    dX = K.DevArray(ctx, (M2, K2), np.float64)
    dW = K.DevArray(ctx, (K2, N2), np.float64)
    dY = K.DevArray(ctx, (M2, N2), np.float64)
    lib.hnh_gemm_f64(ctx.h, M2, N2, K2, dX.ptr, dW.ptr, dY.ptr, 0)
    ctx.sync()
    t = time.perf_counter()
    for _ in range(reps):
        lib.hnh_gemm_f64(ctx.h, M2, N2, K2, dX.ptr, dW.ptr, dY.ptr, 0)
    ctx.sync()
    dt = (time.perf_counter() - t) / reps
    tf = 2.0 * M2 * N2 * K2 / dt / 1e12
    print("gemm_f64    %d x %d x %d (dX = dA W^T at layer 1): %.2f ms -> %.1f TFLOP/s = %.0f %% of peak" % (M2, N2, K2, dt * 1e3, tf, 100 * tf / FP64_MATRIX_PEAK))
    for d in (dA, dB, dC, work, dX, dW, dY):
        d.free()
    ctx.close()


if __name__ == "__main__":
    main()
