"""Development tool: time the GAT's gradient clipping (GAT.set_grad_clip; include/hnh_train_clip.h: hnh_grad_sumsq_f64 and
hnh_optim_step_clip_f64) on one GPU: the kernel against a device copy, and in the model against train_step without clipping.

    python tools/gat_clip_profile.py [logm] [--only kernel|model] [--kernel-lib PATH]

Kernel: hnh_grad_sumsq_f64 over a table with the shapes of the model's learned tensors (per layer the heads' column blocks of one
input_features x heads * 256 gradient matrix, and a1 / a2 interleaved at pitch 2) against a device-to-device copy of the same number of
doubles, the two alternating in one process, five repetitions after a warm-up of each, every call between two device events.  The copy
is the yardstick: the kernel reads 8 B per element and writes nothing, the copy moves 16 B, so the allowance is the copy's median plus
its own min .. max spread.  The verdict is printed, a miss included.

Model (15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 = 14 heads of 256 features, Erdos-Renyi 2^logm vertices (default 18),
edge factor 32, attention softmax, score additive, heads "mean"): train_step with set_grad_clip(1e300) (the sums and the clipped entry
point run, nothing is scaled) against train_step with clipping off, alternating over three rounds after a warm-up of both, every step
between two device synchronisations.  The allowance for the clipped step is the clip-off median plus the kernel's measured time plus the
spread of the clip-off rounds (--kernel-ms, default: measured in the same run).
--kernel-lib PATH runs the clip-off rounds alone on another build of the kernel library (tools/build_variant.sh with HNH_VARIANT_TREE =
a checkout of the parent commit): that is how the two builds are compared in one session.  Clip-off launches the parent's kernels, so
it must lie within the parent's spread.
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
REPS = 5


def kernel():
    """median ms of hnh_grad_sumsq_f64 over the model's table"""
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

    rng = np.random.default_rng(0)
    held, entries, total = [], [], 0
    for fin, f, heads in LAYERS:
        hf = heads * f
        gw, gv = ctx.upload(rng.standard_normal((fin, hf))), ctx.upload(rng.standard_normal((hf, 2)))
        held += [gw, gv]
        entries += [K.OptimTensor(None, 0, gw.ptr + 8 * h * f, hf, None, None, fin, f) for h in range(heads)]
        entries += [K.OptimTensor(None, 0, gv.ptr + 8 * q, 2, None, None, hf, 1) for q in (0, 1)]
        total += fin * hf + 2 * hf
    tab = (K.OptimTensor * len(entries))(*entries)
    need = int(lib.hnh_grad_sumsq_f64_workspace(tab, len(tab)))
    work, res = K.DevArray(ctx, need, np.float64), K.DevArray(ctx, 1, np.float64)
    src, dst = K.DevArray(ctx, total, np.float64), K.DevArray(ctx, total, np.float64)
    calls = {
        "copy": lambda: lib.hnh_memcpy(ctx.h, dst.ptr, src.ptr, total * 8, K.D2D, K.STREAM_COMPUTE),
        "sumsq": lambda: lib.hnh_grad_sumsq_f64(ctx.h, tab, len(tab), 0, res.ptr, work.ptr, need, K.STREAM_COMPUTE),
    }
    for fn in calls.values():  # warm-up of each
        timed(fn)
    t = {k: [] for k in calls}
    for _ in range(REPS):  # alternating
        for k, fn in calls.items():
            t[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    want = sum(float(np.sum(np.square(a.get().astype(np.longdouble)))) for a in held)
    got = float(res.get()[0])
    print("hnh_grad_sumsq_f64 over %d tensors, %d doubles (%.1f MB), %d doubles of workspace; result within %.1e of numpy's:" %
          (len(tab), total, total * 8 / 1e6, need, abs(got - want) / want))
    for k, v in t.items():
        print("  %-5s median %.4f ms (min %.4f .. max %.4f over %d)" % (k, med[k], min(v), max(v), REPS))
    allow = med["copy"] + max(t["copy"]) - min(t["copy"])
    print("  sumsq: median %.4f ms against the copy's median + its spread = %.4f ms: %s (%.2f x the copy; %.2f TB/s read, the copy moves %.2f TB/s)" %
          (med["sumsq"], allow, "within" if med["sumsq"] <= allow else "MISSES it", med["sumsq"] / med["copy"], total * 8 / med["sumsq"] / 1e9,
           total * 16 / med["copy"] / 1e9))
    for a in held + [work, res, src, dst]:
        a.free()
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    ctx.close()
    return med["sumsq"]


def model(logm, lib, kernel_ms):
    from distributed_sddmm_amd import api as H
    assert H.load_backend(lib) == "hip-gfx950"
    names = ["off"] if lib else ["off", "clip"]
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
    m, classes = 1 << logm, LAYERS[-1][1]
    gnn.set_labels(rng.integers(0, classes, m).astype(np.int32), rng.random(m) < 0.7, heads="mean")
    gnn.set_optimizer("adam", 1e-3)

    def select(name):  # (not timed)
        gnn.set_grad_clip(1e300 if name == "clip" else None)

    def timed(fn):
        w.sync()
        t = time.perf_counter()
        fn()
        w.sync()
        return time.perf_counter() - t

    last = {}
    for name in names:  # allocates each path's buffers and warms it up
        select(name)
        gnn.train_step()
        gnn.train_step()
    reps = 3
    tt = {n: [] for n in names}
    for rep in range(reps):  # alternating, every step between two device synchronisations
        for name in names:
            select(name)
            tt[name].append(timed(lambda: last.__setitem__(name, gnn.train_step())))
    for name in names:
        t = np.array(tt[name]) * 1e3
        print("GAT [15d_fusion2, attention softmax, score additive, clipping %s%s] 2^%d vertices, %d nnz, 14 heads, %d classes: train_step median %.1f ms "
              "(min %.1f .. max %.1f) over %d; last pair (%.4f, %.4f)" %
              (name, " on " + os.path.basename(os.path.dirname(lib)) + "/" + os.path.basename(lib) if lib else "", logm, nnz, classes, np.median(t), t.min(), t.max(),
               reps, last[name][0], last[name][1]))
    if "clip" in names:
        a, b = np.array(tt["off"]) * 1e3, np.array(tt["clip"]) * 1e3
        spread = a.max() - a.min()
        allow = np.median(a) + kernel_ms + spread
        print("clip: median %.2f ms against off %.2f ms + the kernel's %.4f ms + the spread of the off rounds %.2f ms = %.2f ms: %s; grad_norm %.6e" %
              (np.median(b), np.median(a), kernel_ms, spread, allow, "within" if np.median(b) <= allow else "MISSES it", gnn.grad_norm()))
    for h in (x, gnn, op):
        h.free()


def main():
    argv = list(sys.argv)
    only, lib, kernel_ms = None, None, None
    for opt in ("--only", "--kernel-lib", "--kernel-ms"):
        if opt in argv:
            i = argv.index(opt)
            if opt == "--only":
                only = argv[i + 1]
            elif opt == "--kernel-lib":
                lib = argv[i + 1]
            else:
                kernel_ms = float(argv[i + 1])
            del argv[i:i + 2]
    if only not in (None, "kernel", "model"):
        sys.exit(__doc__)
    logm = int(argv[1]) if len(argv) > 1 else 18
    if only != "model" and not lib:
        kernel_ms = kernel()
    if only != "kernel":
        if kernel_ms is None and not lib:
            sys.exit("--only model needs --kernel-ms (the kernel's measured time)")
        model(logm, lib, kernel_ms)


if __name__ == "__main__":
    main()
