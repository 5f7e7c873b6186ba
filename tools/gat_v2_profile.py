"""Development tool: time the GAT's forward and backward passes with the three scores ("dot": e_ij = LeakyReLU(<A_i, A_j>), backward mode
fused; "additive": e_ij = LeakyReLU(<A_i, a1> + <A_j, a2>), include/hnh_attn_additive.h; "gatv2": e_ij = a . LeakyReLU(A_i + A_j),
include/hnh_attn_v2.h), attention softmax, on one GPU.

    python tools/gat_v2_profile.py [logm] [--score dot|additive|gatv2|old|all] [--kernel-lib PATH]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32.  Every selected
                                                    score is warmed up (forward and backward), then the scores alternate three times;
                                                    every pass runs between two device synchronisations; mean and min .. max per pass,
                                                    and the ratios to score dot.  `all` (the default): the three scores; `old`: dot
                                                    and additive.
A build without the gatv2 score (an earlier commit's) runs `--score old`, which is how the two builds are compared in one session.
--kernel-lib PATH runs on another build of the kernel library (tools/build_variant.sh with HNH_VARIANT_TREE = a checkout of the parent
commit), as in tools/gat_skip_profile.py.
Under `rocprofv3 --kernel-trace --stats` the run splits into kernels (attn_rows_kernel<AvPass<0 ..>, true> = forward,
attn_rows_kernel / attn_segments_kernel<AvPass<1 ..> ..> = backward row pass, <AvPass<2 ..> ..> = backward column pass;
AgPass = score dot's fused backward; attn_v2_finish_rows_kernel / attn_v2_finish_sum_kernel = the dense finish).
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from distributed_sddmm_amd import api as H
    argv = list(sys.argv)
    score, lib = "all", None
    for opt in ("--score", "--kernel-lib"):
        if opt in argv:
            i = argv.index(opt)
            if opt == "--score":
                score = argv[i + 1]
            else:
                lib = argv[i + 1]
            del argv[i:i + 2]
    if score not in ("dot", "additive", "gatv2", "old", "all"):
        sys.exit(__doc__)
    assert H.load_backend(lib) == "hip-gfx950"
    modes = {"all": ["dot", "additive", "gatv2"], "old": ["dot", "additive"]}.get(score, [score])
    logm = int(argv[1]) if len(argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, layers, 0.2, attention="softmax", backward="fused")
    rng = np.random.default_rng(0)
    for li, (fin, fph, nh) in enumerate(layers):
        for h in range(nh):
            k, n = gnn.weight_shape(li, h)
            gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
            if "additive" in modes or "gatv2" in modes:  # (gatv2 reads the first vector)
                gnn.set_attention_vectors(li, h, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    x = H.Dense.create(w, *gnn.buffer_shape(0))
    x.fill(0.01)
    gnn.set_input(x)
    g = H.Dense.create(w, *gnn.buffer_shape(len(layers)))
    g.fill(1.0)

    def select(mode):
        if hasattr(gnn, "set_score"):
            gnn.set_score(mode)

    for mode in modes:  # allocates each score's buffers and warms it up
        select(mode)
        gnn.forwardPass()
        gnn.backwardPass(g)
    w.sync()
    reps = 3
    ft, bt = {m: [] for m in modes}, {m: [] for m in modes}
    for _ in range(reps):  # alternating, every pass between two device synchronisations
        for mode in modes:
            select(mode)
            w.sync()
            t = time.perf_counter()
            gnn.forwardPass()
            w.sync()
            ft[mode].append(time.perf_counter() - t)
            t = time.perf_counter()
            gnn.backwardPass(g)
            w.sync()
            bt[mode].append(time.perf_counter() - t)
    for mode in modes:
        f, b = np.array(ft[mode]) * 1e3, np.array(bt[mode]) * 1e3
        print("GAT [15d_fusion2, attention softmax, score %s%s] 2^%d vertices, %d nnz, %d heads: forward %.1f ms (min %.1f .. max %.1f), backward %.1f ms "
              "(min %.1f .. max %.1f) over %d" % (mode, " on " + os.path.basename(lib) if lib else "", logm, nnz, heads, f.mean(), f.min(), f.max(), b.mean(), b.min(), b.max(), reps))
    for mode in modes:
        if mode != "dot" and "dot" in modes:
            print("%s / dot: forward %.3f, backward %.3f" % (mode, np.mean(ft[mode]) / np.mean(ft["dot"]), np.mean(bt[mode]) / np.mean(bt["dot"])))
    for h in (g, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
