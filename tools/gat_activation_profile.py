"""Development tool: time the GAT's forward and backward passes with score "additive" (attention softmax) under the output activations
relu, elu and identity on every layer (GAT.set_activation; the HNH_ATTN_ACT_* flags of include/hnh_attention.h and hnh_act_grad_cols_f64 of
include/hnh_grad.h) on one GPU.

    python tools/gat_activation_profile.py [logm] [--activations relu|all]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32.  Every selected
                                                    activation is warmed up (forward and backward), then the activations alternate three
                                                    times; every pass runs between two device synchronisations; mean and min .. max per
                                                    pass, and the ratios to relu.
A build without the option (an earlier commit's) runs `--activations relu` — its own passes, which relu launches unchanged — and that is
how the two builds are compared in one session.  Under `rocprofv3 --kernel-trace --stats` the run splits into kernels: the finishing
launch of attn_rows_kernel<AaPass<0 ..>, true> carries the activation, and act_grad_cols_kernel replaces relu_grad_cols_kernel and rowdot_cols_kernel
in the backward pass of a non-ReLU layer.
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    argv = list(sys.argv)
    which = "all"
    if "--activations" in argv:
        i = argv.index("--activations")
        which = argv[i + 1]
        del argv[i:i + 2]
    if which not in ("relu", "all"):
        sys.exit(__doc__)
    modes = ["relu"] if which == "relu" else ["relu", "elu", "identity"]
    logm = int(argv[1]) if len(argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, layers, 0.2, attention="softmax", score="additive")
    rng = np.random.default_rng(0)
    for li, (fin, fph, nh) in enumerate(layers):
        for h in range(nh):
            k, n = gnn.weight_shape(li, h)
            gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / np.sqrt(k))  # signed aggregates: ELU takes both of its sides
            gnn.set_attention_vectors(li, h, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    x = H.Dense.create(w, *gnn.buffer_shape(0))
    x.upload(rng.uniform(-1, 1, x.shape))
    gnn.set_input(x)
    g = H.Dense.create(w, *gnn.buffer_shape(len(layers)))
    g.fill(1.0)

    def select(mode):
        if hasattr(gnn, "set_activation"):
            for li in range(len(layers)):
                gnn.set_activation(li, mode)
        else:
            gnn.set_input(x)  # (a build without the option: invalidate the stored forward pass, as a change of activation does)

    for mode in modes:  # allocates each mode's buffers and warms it up
        select(mode)
        gnn.forwardPass()
        gnn.backwardPass(g)
    w.sync()
    reps = 3
    ft, bt = {m: [] for m in modes}, {m: [] for m in modes}
    for rep in range(reps):  # alternating, every pass between two device synchronisations
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
        print("GAT [15d_fusion2, attention softmax, score additive, activation %s] 2^%d vertices, %d nnz, %d heads: forward %.1f ms (min %.1f .. max %.1f), "
              "backward %.1f ms (min %.1f .. max %.1f) over %d" % (mode, logm, nnz, heads, f.mean(), f.min(), f.max(), b.mean(), b.min(), b.max(), reps))
    for mode in modes[1:]:
        print("activation %s / relu: forward %.3f, backward %.3f" % (mode, np.mean(ft[mode]) / np.mean(ft[modes[0]]), np.mean(bt[mode]) / np.mean(bt[modes[0]])))
    for h in (g, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
