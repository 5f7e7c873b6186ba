"""Development tool: time the GAT's layer normalisation (GAT.set_norm; include/hnh_gat_norm.h: hnh_layernorm_fwd_f64,
hnh_layernorm_bwd_f64) on one GPU, per kernel against a device copy and in the model against the norm switched off.

    python tools/gat_norm_profile.py [logm] [--only kernels|model] [--kernel-lib PATH]

Per kernel (rows x cols doubles: 2^18 x 256 and 2^16 x 3584, relu, pitches = cols): the forward and the backward call against a
device-to-device copy of the same rows x cols doubles, the three alternating in one process, five repetitions after a warm-up of each,
every call between two device events.  The copy is the yardstick: it moves the forward pass's 16 B per element, so the forward
allowance is the copy's median plus the copy's own min .. max spread; the backward pass moves 24 B per element, allowance 1.5 x the copy's
median plus that spread.  Each kernel's median is set against its allowance and the verdict printed, a miss included.

Model (15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 = 14 heads of 256 features, Erdos-Renyi 2^logm vertices (default 18),
edge factor 32, attention softmax, score additive): forward, backward and train_step with the norm on every layer against the norm off,
alternating over three rounds after a warm-up of both, every pass between two device synchronisations; the expected increment is the
byte model (16 B per element and 16 B per row forward, 24 B per element backward, over the three layers' outputs) at the copy rate
measured in the same run (one pass over the last layer's output, read + write).
--kernel-lib PATH runs the model with the norm off on another build of the kernel library (tools/build_variant.sh with
HNH_VARIANT_TREE = a checkout of the parent commit): that is how the two builds are compared in one session.
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
KERNEL_SHAPES = [(1 << 18, 256), (1 << 16, 3584)]
REPS = 5


def kernels():
    from distributed_sddmm_amd import _kernels as K
    ctx = K.Ctx(0)
    lib = ctx.lib
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ctx.check(lib.hnh_event_create(ctx.h, C.byref(e)), "event")

    def timed(fn):
        ctx.check(lib.hnh_event_record(ctx.h, ev[0], K.STREAM_COMPUTE), "record")
        ctx.check(fn(), "call")
        ctx.check(lib.hnh_event_record(ctx.h, ev[1], K.STREAM_COMPUTE), "record")
        ctx.check(lib.hnh_event_sync(ctx.h, ev[1]), "sync")
        ms = C.c_float()
        ctx.check(lib.hnh_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
        return ms.value

    for rows, cols in KERNEL_SHAPES:
        n = rows * cols
        rng = np.random.default_rng(0)
        z = ctx.upload(rng.uniform(-1, 1, n))
        g = ctx.upload(rng.uniform(-1, 1, n))
        out, dz = K.DevArray(ctx, n, np.float64), K.DevArray(ctx, n, np.float64)
        stats = K.DevArray(ctx, 2 * rows, np.float64)
        gamma, beta = ctx.upload(rng.uniform(0.5, 1.5, cols)), ctx.upload(rng.uniform(-1, 1, cols))
        dgamma, dbeta = K.DevArray(ctx, cols, np.float64), K.DevArray(ctx, cols, np.float64)
        need = lib.hnh_layernorm_bwd_workspace(rows, cols)
        work = K.DevArray(ctx, need, np.float64)
        calls = {
            "copy": lambda: lib.hnh_memcpy(ctx.h, out.ptr, z.ptr, n * 8, K.D2D, K.STREAM_COMPUTE),
            "forward": lambda: lib.hnh_layernorm_fwd_f64(ctx.h, out.ptr, cols, z.ptr, cols, stats.ptr, gamma.ptr, beta.ptr, rows, cols, 1e-5, 0, K.STREAM_COMPUTE),
            "backward": lambda: lib.hnh_layernorm_bwd_f64(ctx.h, dz.ptr, cols, dgamma.ptr, dbeta.ptr, g.ptr, cols, z.ptr, cols, stats.ptr, gamma.ptr, beta.ptr, rows,
                                                          cols, 0, work.ptr, need, K.STREAM_COMPUTE),
        }
        for fn in calls.values():  # warm-up of each
            timed(fn)
        t = {k: [] for k in calls}
        for _ in range(REPS):  # alternating
            for k, fn in calls.items():
                t[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = max(t["copy"]) - min(t["copy"])
        print("%d x %d doubles (%.2f GB per matrix), partial column sums %.1f MB:" % (rows, cols, n * 8 / 1e9, need * 8 / 1e6))
        for k, v in t.items():
            bytes_ = n * (24 if k == "backward" else 16)
            print("  %-8s median %.3f ms (min %.3f .. max %.3f over %d): %.2f TB/s of its byte model" % (k, med[k], min(v), max(v), REPS, bytes_ / med[k] / 1e9))
        for k, factor in (("forward", 1.0), ("backward", 1.5)):
            allow = factor * med["copy"] + spread
            print("  %s: median %.3f ms against an allowance of %.1f x the copy's median + its spread = %.3f ms: %s (%.2f x the copy)" %
                  (k, med[k], factor, allow, "within" if med[k] <= allow else "MISSES it", med[k] / med["copy"]))
        for a in (z, g, out, dz, stats, gamma, beta, dgamma, dbeta, work):
            a.free()
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    ctx.close()


def model(logm, lib):
    from distributed_sddmm_amd import api as H
    assert H.load_backend(lib) == "hip-gfx950"
    names = ["off"] if lib else ["off", "norm"]
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
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
    gnn.set_labels(rng.integers(0, LAYERS[-1][1], 1 << logm).astype(np.int32), None, heads="mean")
    gnn.set_optimizer("adam", 1e-3)

    def select(name):
        if lib or not hasattr(gnn, "set_norm"):
            gnn.set_input(x)  # (a build without the option: invalidate the stored forward pass, as a setter does)
            return
        for li in range(len(LAYERS)):
            gnn.set_norm(li, "layer" if name == "norm" else "none")

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
        gnn.train_step()
    gnn.get_output(out)
    w.sync()
    copies = [timed(lambda: gnn.get_output(out)) for _ in range(5)]
    rate = 2 * out.shape[0] * out.shape[1] * 8 / min(copies)
    print("device copy of the last layer's output (%d x %d, read + write): %.2f ms (min of 5, max %.2f), %.2f TB/s" %
          (out.shape[0], out.shape[1], min(copies) * 1e3, max(copies) * 1e3, rate / 1e12))
    select(names[0])  # (one untimed round: settles clocks and the allocator after the copies)
    gnn.forwardPass()
    gnn.backwardPass(g)
    reps = 3
    ft, bt, tt = ({n: [] for n in names} for _ in range(3))
    for rep in range(reps):  # alternating, every pass between two device synchronisations
        for name in names:
            select(name)
            ft[name].append(timed(gnn.forwardPass))
            bt[name].append(timed(lambda: gnn.backwardPass(g)))
            tt[name].append(timed(gnn.train_step))
    for name in names:
        f, b, t = (np.array(v[name]) * 1e3 for v in (ft, bt, tt))
        print("GAT [15d_fusion2, attention softmax, score additive, norm %s%s] 2^%d vertices, %d nnz, 14 heads: forward %.1f ms (min %.1f .. max %.1f), "
              "backward %.1f ms (min %.1f .. max %.1f), train_step %.1f ms (min %.1f .. max %.1f) over %d" %
              (name, " on " + os.path.basename(lib) if lib else "", logm, nnz, f.mean(), f.min(), f.max(), b.mean(), b.min(), b.max(), t.mean(), t.min(), t.max(), reps))
    if "norm" in names:
        elems = sum(rows * fph * nh for _, fph, nh in LAYERS)
        mf, mb = 16 * elems + 16 * rows * len(LAYERS), 24 * elems
        d = {k: (np.min(v["norm"]) - np.min(v["off"])) * 1e3 for k, v in (("forward", ft), ("backward", bt), ("train_step", tt))}
        print("norm - off (minima): forward %+.2f ms (byte model %.2f GB: %.2f ms at the copy rate), backward %+.2f ms (byte model %.2f GB: %.2f ms), "
              "train_step %+.2f ms (both: %.2f ms); memory: one more rows x H f matrix per layer, %.2f GB" %
              (d["forward"], mf / 1e9, mf / rate * 1e3, d["backward"], mb / 1e9, mb / rate * 1e3, d["train_step"], (mf + mb) / rate * 1e3, elems * 8 / 1e9))
    for h in (out, g, x, gnn, op):
        h.free()


def main():
    argv = list(sys.argv)
    only, lib = None, None
    for opt in ("--only", "--kernel-lib"):
        if opt in argv:
            i = argv.index(opt)
            if opt == "--only":
                only = argv[i + 1]
            else:
                lib = argv[i + 1]
            del argv[i:i + 2]
    if only not in (None, "kernels", "model"):
        sys.exit(__doc__)
    logm = int(argv[1]) if len(argv) > 1 else 18
    if only != "model" and not lib:
        kernels()
    if only != "kernels":
        model(logm, lib)


if __name__ == "__main__":
    main()
