"""Development tool: time the GAT's forward and backward passes with both attention modes ("none": the LeakyReLU scores are the edge
weights; "softmax": normalised over each row's neighbourhood, include/hnh_attention.h) on one GPU.

    python tools/gat_softmax_profile.py [logm] [--backward unfused|fused|both] [--attention none|softmax|both]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32: forward and
                                                    backward ms per attention mode and backward mode (default both: the un-fused and
                                                    the fused backward pass in the same run, both warmed up, then alternating, each
                                                    pass between two device synchronisations), and the softmax / none ratios
Under `rocprofv3 --kernel-trace --stats`, `python tools/gat_backward_profile.py --stats <dir>` splits a run into kernel groups.
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    argv = list(sys.argv)
    opts = {"--backward": "both", "--attention": "both"}
    for o in opts:
        if o in argv:
            i = argv.index(o)
            opts[o] = argv[i + 1]
            del argv[i:i + 2]
    if opts["--backward"] not in ("unfused", "fused", "both") or opts["--attention"] not in ("none", "softmax", "both"):
        sys.exit(__doc__)
    bmodes = ["unfused", "fused"] if opts["--backward"] == "both" else [opts["--backward"]]
    amodes = ["none", "softmax"] if opts["--attention"] == "both" else [opts["--attention"]]
    logm = int(argv[1]) if len(argv) > 1 else 18
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
    for mode in amodes:
        gnn.set_attention(mode)
        gnn.forwardPass()
        for b in bmodes:  # allocates each backward mode's buffers and warms it up
            gnn.set_backward(b)
            gnn.backwardPass(g)
        w.sync()
        reps = 3
        t = time.perf_counter()
        for _ in range(reps):
            gnn.forwardPass()
        w.sync()
        fwd = (time.perf_counter() - t) / reps
        bt = {b: [] for b in bmodes}
        for _ in range(reps):  # alternating, every pass between two device synchronisations
            for b in bmodes:
                gnn.set_backward(b)
                w.sync()
                t = time.perf_counter()
                gnn.backwardPass(g)
                w.sync()
                bt[b].append(time.perf_counter() - t)
        times[mode] = (fwd, {b: float(np.mean(v)) for b, v in bt.items()})
        for b in bmodes:
            bwd = times[mode][1][b]
            print("GAT [15d_fusion2, attention %s, backward %s] 2^%d vertices, %d nnz, %d heads: forward %.1f ms (%.2f per head), backward %.1f ms "
                  "(%.2f per head; min %.1f .. max %.1f over %d)"
                  % (mode, b, logm, nnz, heads, fwd * 1e3, fwd * 1e3 / heads, bwd * 1e3, bwd * 1e3 / heads, min(bt[b]) * 1e3, max(bt[b]) * 1e3, reps))
        if len(bmodes) == 2:
            u, f = times[mode][1]["unfused"], times[mode][1]["fused"]
            print("attention %s: un-fused / fused backward %.2f x (%.1f -> %.1f ms)" % (mode, u / f, u * 1e3, f * 1e3))
    if len(amodes) == 2:
        (f0, b0), (f1, b1) = times["none"], times["softmax"]
        print("softmax / none: forward %.3f" % (f1 / f0) + "".join(", backward (%s) %.3f" % (b, b1[b] / b0[b]) for b in bmodes))
    for h in (g, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
