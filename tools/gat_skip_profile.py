"""Development tool: time the GAT's forward and backward passes with score "additive" (attention softmax) with and without a bias and
skip connections (GAT.set_bias / set_residual; include/hnh_gat_skip.h: HNH_ATTN_ADDEND on the finishing launches,
hnh_skip_addend_cols_f64, hnh_skip_grad_cols_f64, hnh_colsum_f64) on one GPU.

    python tools/gat_skip_profile.py [logm] [--configs off|all] [--kernel-lib PATH]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32.  Configurations:
                                                    off (neither), bias (every layer), identity (the layer whose widths agree: layer 1,
                                                    4 heads), projection (every layer).  Every selected configuration is warmed up
                                                    (forward and backward), then they alternate over two rounds (after one untimed round
                                                    of the first: the first pass after the copies below has been seen 14 ms slow); every
                                                    pass runs between two device synchronisations; mean and min .. max per pass and the
                                                    differences of the minima to off.
The copy rate of the device (one pass over the last layer's output: read + write) is measured in the same run, and each configuration's
byte model — one rows x f block per head written by hnh_skip_addend_cols_f64 and read again by the finishing launch; backward: the second
dZ store, the reads of the addend's operands, the column sum and the dX update — is printed as the time it predicts at that rate.
For projection the forward pass also runs with HNH_GAT_SERIAL=1 (one stream): serial(projection) - serial(off) is what the extra product
and the addend cost, pipelined(projection) - pipelined(off) is what of it is NOT hidden beside the attention pass.
--kernel-lib PATH runs configuration off on another build of the kernel library (tools/build_variant.sh with HNH_VARIANT_TREE = a
checkout of the parent commit): a layer without bias and residual launches only what that library has, and that is how the two builds
are compared in one session.
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
CONFIGS = {
    "off": dict(bias=(), residual={}),
    "bias": dict(bias=(0, 1, 2), residual={}),
    "identity": dict(bias=(), residual={1: "identity"}),
    "projection": dict(bias=(), residual={0: "projection", 1: "projection", 2: "projection"}),
}


def model_bytes(cfg, rows):
    """(forward, backward) bytes a configuration adds, per the header's byte model"""
    fwd = bwd = 0
    for li, (k, f, heads) in enumerate(LAYERS):
        mode = cfg["residual"].get(li, "none")
        if li not in cfg["bias"] and mode == "none":
            continue
        block, hf = rows * f * 8, heads * f
        res_read = block if mode != "none" else 0
        fwd += heads * (2 * block + res_read)                 # addend written and read back (+ its residual operand read)
        if mode == "projection":
            fwd += heads * (rows * k * 8 + block)             # X read and the product written by the extra GEMM
        bwd += heads * (block + res_read)                     # the second dZ store (+ the residual operand read)
        if mode == "projection":
            bwd += heads * (rows * k * 8 + block)             # the recomputed product
            bwd += rows * (k + hf) * 8 + rows * (hf + k) * 8  # dW_res = X^T dZ_all, dZ_all W_res^T
        if mode != "none":
            bwd += 3 * rows * k * 8                           # dX += (two reads, one write)
        if li in cfg["bias"]:
            bwd += rows * hf * 8                              # the column sum reads dZ_all once
    return fwd, bwd


def main():
    from distributed_sddmm_amd import api as H
    argv = list(sys.argv)
    which, lib = "all", None
    for opt in ("--configs", "--kernel-lib"):
        if opt in argv:
            i = argv.index(opt)
            if opt == "--configs":
                which = argv[i + 1]
            else:
                lib = argv[i + 1]
            del argv[i:i + 2]
    if which not in ("off", "all"):
        sys.exit(__doc__)
    assert H.load_backend(lib) == "hip-gfx950"
    names = ["off"] if which == "off" or lib else list(CONFIGS)
    logm = int(argv[1]) if len(argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    heads = sum(l[2] for l in LAYERS)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, LAYERS, 0.2, attention="softmax", score="additive")
    rng = np.random.default_rng(0)
    for li, (fin, fph, nh) in enumerate(LAYERS):
        for h in range(nh):
            k, n = gnn.weight_shape(li, h)
            gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / np.sqrt(k))
            gnn.set_attention_vectors(li, h, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    x = H.Dense.create(w, *gnn.buffer_shape(0))
    x.upload(rng.uniform(-1, 1, x.shape))
    gnn.set_input(x)
    g = H.Dense.create(w, *gnn.buffer_shape(len(LAYERS)))
    g.fill(1.0)
    out = H.Dense.create(w, *gnn.buffer_shape(len(LAYERS)))
    rows = x.shape[0]
    bias = {li: rng.uniform(-1, 1, fph * nh) for li, (fin, fph, nh) in enumerate(LAYERS)}
    wres = {li: rng.uniform(-1, 1, (fin, fph * nh)) / np.sqrt(fin) for li, (fin, fph, nh) in enumerate(LAYERS)}

    def select(name):
        cfg = CONFIGS[name]
        if not hasattr(gnn, "set_bias") or lib:
            gnn.set_input(x)  # (a build without the options: invalidate the stored forward pass, as a setter does)
            return
        for li in range(len(LAYERS)):
            gnn.set_bias(li, bias[li] if li in cfg["bias"] else None)
            mode = cfg["residual"].get(li, "none")
            gnn.set_residual(li, mode)
            if mode == "projection":
                gnn.set_residual_weight(li, wres[li])

    def timed(fn):
        w.sync()
        t = time.perf_counter()
        fn()
        w.sync()
        return time.perf_counter() - t

    for name in names:  # allocates each configuration's buffers and warms it up
        select(name)
        gnn.forwardPass()
        gnn.backwardPass(g)
    gnn.get_output(out)
    w.sync()
    copies = [timed(lambda: gnn.get_output(out)) for _ in range(5)]
    copy_bytes = 2 * out.shape[0] * out.shape[1] * 8
    rate = copy_bytes / min(copies)
    print("device copy of the last layer's output (%d x %d, read + write): %.2f ms, %.2f TB/s" % (out.shape[0], out.shape[1], min(copies) * 1e3, rate / 1e12))
    select(names[0])  # (one untimed round: settles clocks and the allocator after the copies)
    gnn.forwardPass()
    gnn.backwardPass(g)
    reps = 2
    ft, bt, st = ({n: [] for n in names} for _ in range(3))
    for rep in range(reps):  # alternating, every pass between two device synchronisations
        for name in names:
            select(name)
            ft[name].append(timed(gnn.forwardPass))
            bt[name].append(timed(lambda: gnn.backwardPass(g)))
            if name in ("off", "projection"):
                os.environ["HNH_GAT_SERIAL"] = "1"
                try:
                    select(name)
                    st[name].append(timed(gnn.forwardPass))
                finally:
                    del os.environ["HNH_GAT_SERIAL"]
    for name in names:
        f, b = np.array(ft[name]) * 1e3, np.array(bt[name]) * 1e3
        print("GAT [15d_fusion2, attention softmax, score additive, %s%s] 2^%d vertices, %d nnz, %d heads: forward %.1f ms (min %.1f .. max %.1f), "
              "backward %.1f ms (min %.1f .. max %.1f) over %d" % (name, " on " + os.path.basename(lib) if lib else "", logm, nnz, heads, f.mean(), f.min(), f.max(),
                                                                  b.mean(), b.min(), b.max(), reps))
    for name in names[1:]:
        mf, mb = model_bytes(CONFIGS[name], rows)
        print("%s - off: forward %+.2f ms (byte model %.2f GB: %.2f ms at the copy rate), backward %+.2f ms (byte model %.2f GB: %.2f ms)" %
              (name, (np.min(ft[name]) - np.min(ft["off"])) * 1e3, mf / 1e9, mf / rate * 1e3, (np.min(bt[name]) - np.min(bt["off"])) * 1e3, mb / 1e9,
               mb / rate * 1e3))
    if "projection" in names:
        s_off, s_prj = np.min(st["off"]) * 1e3, np.min(st["projection"]) * 1e3
        print("forward on one stream (HNH_GAT_SERIAL=1): off %.1f ms, projection %.1f ms: the extra products and addends cost %.1f ms, of which %.1f ms "
              "are exposed in the pipelined pass" % (s_off, s_prj, s_prj - s_off, (np.min(ft["projection"]) - np.min(ft["off"])) * 1e3))
    for h in (out, g, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
