"""Development tool: time the GAT's forward and backward passes with both attention modes ("none": the LeakyReLU scores are the edge
weights; "softmax": normalised over each row's neighbourhood, include/hnh_attention.h) on one GPU.

    python tools/gat_softmax_profile.py [logm]      15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32: forward and
                                                    backward ms per mode, and the softmax / none ratios
Under `rocprofv3 --kernel-trace --stats`, `python tools/gat_backward_profile.py --stats <dir>` splits a run into kernel groups.
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    logm = int(sys.argv[1]) if len(sys.argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
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
    times = {}
    for mode in ("none", "softmax"):
        gnn.set_attention(mode)
        gnn.forwardPass()
        gnn.backwardPass(g)  # allocates the backward buffers
        w.sync()
        reps = 3
        t = time.perf_counter()
        for _ in range(reps):
            gnn.forwardPass()
        w.sync()
        fwd = (time.perf_counter() - t) / reps
        t = time.perf_counter()
        for _ in range(reps):
            gnn.backwardPass(g)
        w.sync()
        bwd = (time.perf_counter() - t) / reps
        times[mode] = (fwd, bwd)
        print("GAT [15d_fusion2, attention %s] 2^%d vertices, %d nnz, %d heads: forward %.1f ms (%.2f per head), backward %.1f ms (%.2f per head)"
              % (mode, logm, nnz, heads, fwd * 1e3, fwd * 1e3 / heads, bwd * 1e3, bwd * 1e3 / heads))
    (f0, b0), (f1, b1) = times["none"], times["softmax"]
    print("softmax / none: forward %.3f, backward %.3f" % (f1 / f0, b1 / b0))
    for h in (g, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
