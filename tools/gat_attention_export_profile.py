"""Development tool: time the export of the GAT's attention coefficients (GAT.attention_coefficients, include/hnh_attn_coef.h) per head in
the three score modes and, for score additive, under attention dropout, beside forwardPass of the same mode on the same build, on one GPU.

    python tools/gat_attention_export_profile.py [logm] [--mode dot|additive|gatv2|additive-dropout|all]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32.  Every selected
                                                    mode is warmed up (forward pass and one export of every head), then the modes alternate
                                                    three times; the forward pass and the 14 exports each run between two device
                                                    synchronisations; mean and min .. max per head.

An export is the head's product A = X W_h (a GEMM on the compute stream, which the forward pass hides behind the previous head's attention
pass on a second stream), for score additive the small dense pass that builds s and the packed pair [t | id], and ONE sparse pass over the
nonzeros.  The sparse pass alone is timed by the operator's kernel profile (event pairs round the kernel calls) and compared with its byte
model at 8 TB/s:  dot, gatv2  nnz (8 f + 4 + 8) B;  additive  nnz (16 + 4 + 8) B (and nnz (128 + 4 + 8) B when every 16-byte gather costs its
128-byte line).  The row operand (rows x f x 8 B) and lse are left out of the model, as they are for the forward passes.
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

MODES = {"dot": ("dot", 0.0), "additive": ("additive", 0.0), "gatv2": ("gatv2", 0.0), "additive-dropout": ("additive", 0.6)}


def main():
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    argv = list(sys.argv)
    which = "all"
    if "--mode" in argv:
        i = argv.index("--mode")
        which = argv[i + 1]
        del argv[i:i + 2]
    if which != "all" and which not in MODES:
        sys.exit(__doc__)
    modes = list(MODES) if which == "all" else [which]
    logm = int(argv[1]) if len(argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    f = 256
    every = [(li, h) for li, (_, _, nh) in enumerate(layers) for h in range(nh)]
    heads = len(every)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, layers, 0.2, attention="softmax")
    rng = np.random.default_rng(0)
    for li, h in every:
        k, n = gnn.weight_shape(li, h)
        gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
        gnn.set_attention_vectors(li, h, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    x = H.Dense.create(w, *gnn.buffer_shape(0))
    x.fill(0.01)
    gnn.set_input(x)
    out = op.like_S_values(0.0)

    def select(mode):
        score, p = MODES[mode]
        gnn.set_dropout(0.0, 0.0, 0)  # (a rate is refused with the scores that have no mask)
        gnn.set_score(score)
        gnn.set_dropout(p, 0.0, 7)

    def export_all(mode):
        for li, h in every:
            gnn.attention_coefficients(li, h, out=out, dropped=MODES[mode][1] > 0.0)

    for mode in modes:  # allocates each mode's buffers and warms it up
        select(mode)
        gnn.forwardPass()
        export_all(mode)
    w.sync()
    reps = 3
    ft, et, kt = ({m: [] for m in modes} for _ in range(3))
    for _ in range(reps):  # alternating, every timed section between two device synchronisations
        for mode in modes:
            select(mode)
            w.sync()
            t = time.perf_counter()
            gnn.forwardPass()
            w.sync()
            ft[mode].append((time.perf_counter() - t) / heads)
            t = time.perf_counter()
            export_all(mode)
            w.sync()
            et[mode].append((time.perf_counter() - t) / heads)
            op.kernel_profile(1)  # the sparse pass alone: a second round under the kernel profile's event pairs
            export_all(mode)
            w.sync()
            ms, launches = op.kernel_profile(0)
            assert launches >= heads
            kt[mode].append(ms * 1e-3 / heads)
    print("GAT attention export [15d_fusion2, attention softmax] 2^%d vertices, %d nnz, %d heads of %d, per head, over %d:" % (logm, nnz, heads, f, reps))
    for mode in modes:
        fw, ex, kn = (np.array(v[mode]) * 1e3 for v in (ft, et, kt))
        model = nnz * ((16 if MODES[mode][0] == "additive" else 8 * f) + 4 + 8)
        line = "  %-17s forward %.3f ms (min %.3f .. max %.3f)  export %.3f ms (min %.3f .. max %.3f) = %.2f x forward  sparse pass %.3f ms (min %.3f .. max %.3f)" \
               "  byte model %.3e B = %.3f of 8 TB/s" % (mode, fw.mean(), fw.min(), fw.max(), ex.mean(), ex.min(), ex.max(), ex.mean() / fw.mean(), kn.mean(), kn.min(),
                                                        kn.max(), model, model / (kn.mean() * 1e-3) / 8e12)
        if MODES[mode][0] == "additive":
            lines = nnz * (128 + 4 + 8)
            line += "  (one 128-byte line per gather: %.3e B = %.3f of 8 TB/s)" % (lines, lines / (kn.mean() * 1e-3) / 8e12)
        print(line)
    for h in (out, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
