"""Development tool: time the GAT's training step (include/hnh_train.h) against the forward and backward passes it contains, and against
the host-driven update loop that was the only way to train before it, on one GPU.

    python tools/gat_train_profile.py [logm]
                                                    15d_fusion2, c = 1, attention softmax, score additive, the layers of
                                                    benchmark_dist.cpp:93-95 (14 heads of 256 features; output rows of 6 x 256 = 1536
                                                    values, heads "mean": 256 classes), Erdos-Renyi 2^logm vertices (default 18), edge
                                                    factor 32, 30 % of the rows labelled for training, Adam.
After a warm-up of every path, three rounds of, each between two device synchronisations:
    forwardPass + backwardPass          the passes alone, from a fixed output gradient
    loss(grad_out)                      the cross-entropy pass with its all-reduce and the read of the two scalars
    optimizer_step                      the table-driven update
    train_step                          forward, loss, backward, update; one host synchronisation
    host loop                           forwardPass, loss(grad_out), backwardPass, then every weight_grad / attention_grad downloaded, Adam in
                                        numpy, every head uploaded with set_weight / set_attention_vectors
and prints mean and min .. max per path.  Under `rocprofv3 --kernel-trace --stats` the new kernels are xent_rows_kernel, xent_finish_kernel
and optim_step_kernel.
"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    logm = int(sys.argv[1]) if len(sys.argv) > 1 else 18
    m = 1 << logm
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, layers, 0.2, attention="softmax", score="additive")
    rng = np.random.default_rng(0)
    keys = [(li, h) for li, (fin, fph, nh) in enumerate(layers) for h in range(nh)]
    for li, h in keys:
        k, n = gnn.weight_shape(li, h)
        gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
        gnn.set_attention_vectors(li, h, rng.uniform(-1, 1, n), rng.uniform(-1, 1, n))
    x = H.Dense.create(w, *gnn.buffer_shape(0))
    x.fill(0.01)
    gnn.set_input(x)
    g = H.Dense.create(w, *gnn.buffer_shape(len(layers)))
    g.fill(1.0)
    gnn.set_labels(rng.integers(0, layers[-1][1], m), rng.random(m) < 0.3, heads="mean")
    hyper = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)
    gnn.set_optimizer("adam", hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"])

    def timed(fn):
        w.sync()
        t = time.perf_counter()
        fn()
        w.sync()
        return (time.perf_counter() - t) * 1e3

    def passes():
        gnn.forwardPass()
        gnn.backwardPass(g)

    state = {k: [gnn.get_weight(*k), 0.0, 0.0, list(gnn.get_attention_vectors(*k)), [0.0, 0.0], [0.0, 0.0]] for k in keys}
    steps = [0]

    def host_update():
        steps[0] += 1
        t = steps[0]
        bc1, bc2 = 1.0 - hyper["beta1"] ** t, 1.0 - hyper["beta2"] ** t

        def adam(p, grad, mom, var):
            mom = hyper["beta1"] * mom + (1.0 - hyper["beta1"]) * grad
            var = hyper["beta2"] * var + (1.0 - hyper["beta2"]) * grad * grad
            return p - hyper["lr"] * (mom / bc1) / (np.sqrt(var / bc2) + hyper["eps"]), mom, var

        for k in keys:
            st = state[k]
            st[0], st[1], st[2] = adam(st[0], gnn.weight_grad(*k), st[1], st[2])
            gnn.set_weight(*k, st[0])
            da = gnn.attention_grad(*k)
            for q in (0, 1):
                st[3][q], st[4][q], st[5][q] = adam(st[3][q], da[q], st[4][q], st[5][q])
            gnn.set_attention_vectors(*k, st[3][0], st[3][1])

    def host_loop():
        gnn.forwardPass()
        gnn.loss(None, g)
        gnn.backwardPass(g)
        host_update()

    paths = {"forwardPass + backwardPass": passes, "loss(grad_out)": lambda: gnn.loss(None, g), "optimizer_step": gnn.optimizer_step,
             "train_step": gnn.train_step, "host loop": host_loop, "host loop, update only": None}
    times = {k: [] for k in paths}
    for rep in range(4):  # round 0 allocates every path's buffers and warms it up
        rec = rep > 0
        t = timed(passes)
        if rec:
            times["forwardPass + backwardPass"].append(t)
        gnn.forwardPass()
        t = timed(lambda: gnn.loss(None, g))
        if rec:
            times["loss(grad_out)"].append(t)
        gnn.backwardPass(g)
        t = timed(gnn.optimizer_step)
        if rec:
            times["optimizer_step"].append(t)
        t = timed(gnn.train_step)
        if rec:
            times["train_step"].append(t)
        gnn.forwardPass()
        gnn.loss(None, g)
        gnn.backwardPass(g)
        tu = timed(host_update)
        t = timed(host_loop)
        if rec:
            times["host loop"].append(t)
            times["host loop, update only"].append(tu)
    print("GAT training [15d_fusion2, attention softmax, score additive, Adam] 2^%d vertices, %d nnz, %d heads, output rows of %d values:"
          % (logm, nnz, heads, layers[-1][1] * layers[-1][2]))
    for k, v in times.items():
        v = np.array(v)
        print("    %-28s %9.2f ms (min %.2f .. max %.2f) over %d" % (k, v.mean(), v.min(), v.max(), len(v)))
    base = np.mean(times["forwardPass + backwardPass"])
    print("train_step / (forwardPass + backwardPass): %.4f;  host loop / train_step: %.3f" % (np.mean(times["train_step"]) / base,
                                                                                           np.mean(times["host loop"]) / np.mean(times["train_step"])))
    for h in (g, x, gnn, op):
        h.free()


if __name__ == "__main__":
    main()
