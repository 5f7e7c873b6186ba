"""Development tool: time the GAT's multi-label head (GAT.set_multilabel_targets; include/hnh_train_multilabel.h: hnh_bce_rows_f64) on one
GPU, per kernel against the softmax head's kernel and a device copy, and in the model against train_step under set_labels.

    python tools/gat_multilabel_profile.py [logm] [--only kernels|model] [--kernel-lib PATH]

Per kernel (rows x (heads x classes): 2^18 x (1 x 121), 2^18 x (6 x 121), 2^16 x (14 x 256); pitches = the row, G a matrix of its own, a
mask over 70 % of the rows, class weights): hnh_bce_rows_f64 against hnh_xent_rows_f64 at the same shape and against a device-to-device
copy of the same rows x heads * classes doubles, the three alternating in one process, five repetitions after a warm-up of each, every
call between two device events.  hnh_xent_rows_f64 is the yardstick: it moves the same doubles and does strictly more per row (it stages
the row and reduces over it), so the allowance is its median plus its own min .. max spread.  The new kernel's median is set against
the allowance and the verdict printed, a miss included, with its share of the byte model (16 * heads * classes + 4 * ceil(classes / 32) +
1 B per row) at the copy's rate.

Model (15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 = 14 heads of 256 features, Erdos-Renyi 2^logm vertices (default 18),
edge factor 32, attention softmax, score additive, heads "mean": 256 classes): train_step under the sigmoid head against train_step under
set_labels, alternating over three rounds after a warm-up of both, every step between two device synchronisations; the expected
difference is within the spread of the set_labels rounds.
--kernel-lib PATH runs the set_labels rounds alone on another build of the kernel library (tools/build_variant.sh with HNH_VARIANT_TREE =
a checkout of the parent commit): that is how the two builds are compared in one session.
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAYERS = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
KERNEL_SHAPES = [(1 << 18, 1, 121), (1 << 18, 6, 121), (1 << 16, 14, 256)]
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

    for rows, heads, classes in KERNEL_SHAPES:
        n = heads * classes
        words = (classes + 31) // 32
        rng = np.random.default_rng(0)
        out = ctx.upload(rng.uniform(-5, 5, rows * n))
        g = K.DevArray(ctx, rows * n, np.float64)
        mask = rng.random(rows) < 0.7
        d_mask = ctx.upload(mask.astype(np.uint8))
        d_bits = ctx.upload(rng.integers(0, 1 << 32, rows * words, dtype=np.uint64).astype(np.uint32))
        d_pw = ctx.upload(rng.uniform(0.5, 2.0, classes))
        d_labels = ctx.upload(np.where(mask, rng.integers(0, classes, rows), -1).astype(np.int32))
        need = max(int(lib.hnh_bce_rows_f64_workspace(rows)), int(lib.hnh_xent_rows_f64_workspace(rows)))
        work, res = K.DevArray(ctx, need, np.float64), K.DevArray(ctx, 4, np.float64)
        inv_n = 1.0 / np.count_nonzero(mask)
        calls = {
            "copy": lambda: lib.hnh_memcpy(ctx.h, g.ptr, out.ptr, rows * n * 8, K.D2D, K.STREAM_COMPUTE),
            "xent": lambda: lib.hnh_xent_rows_f64(ctx.h, out.ptr, n, d_labels.ptr, rows, heads, classes, inv_n, g.ptr, n, res.ptr, work.ptr, need, K.STREAM_COMPUTE),
            "bce": lambda: lib.hnh_bce_rows_f64(ctx.h, out.ptr, n, d_bits.ptr, words, d_mask.ptr, d_pw.ptr, rows, heads, classes, inv_n / classes, g.ptr, n, res.ptr,
                                                work.ptr, need, K.STREAM_COMPUTE),
        }
        for fn in calls.values():  # warm-up of each
            timed(fn)
        t = {k: [] for k in calls}
        for _ in range(REPS):  # alternating
            for k, fn in calls.items():
                t[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = max(t["xent"]) - min(t["xent"])
        model = rows * (16 * n + 4 * words + 1)
        rate = rows * n * 16 / med["copy"] / 1e9  # TB/s: the copy reads and writes every double
        print("%d rows x (%d heads x %d classes) doubles (%.2f GB per matrix), %.0f %% of the rows in the loss:" % (rows, heads, classes, rows * n * 8 / 1e9, 100.0 * mask.mean()))
        for k, v in t.items():
            print("  %-4s median %.3f ms (min %.3f .. max %.3f over %d)" % (k, med[k], min(v), max(v), REPS))
        allow = med["xent"] + spread
        print("  bce: median %.3f ms against the yardstick's median + its spread = %.3f ms: %s (%.2f x xent, %.2f x the copy)" %
              (med["bce"], allow, "within" if med["bce"] <= allow else "MISSES it", med["bce"] / med["xent"], med["bce"] / med["copy"]))
        print("  bce: byte model %.3f GB = %.3f ms at the copy's %.2f TB/s: %.0f %% of the byte model's rate (every row's bytes counted, the masked-out rows' reads too)" %
              (model / 1e9, model / rate / 1e9, rate, 100.0 * (model / rate / 1e9) / med["bce"]))
        for a in (out, g, d_mask, d_bits, d_pw, d_labels, work, res):
            a.free()
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    ctx.close()


def model(logm, lib):
    from distributed_sddmm_amd import api as H
    assert H.load_backend(lib) == "hip-gfx950"
    names = ["labels"] if lib else ["labels", "multilabel"]
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
    labels = rng.integers(0, classes, m).astype(np.int32)
    targets = rng.random((m, classes)) < 0.3
    train = rng.random(m) < 0.7
    pw = rng.uniform(0.5, 2.0, classes)
    gnn.set_optimizer("adam", 1e-3)

    def select(name):  # (not timed: the most recent setter decides the head)
        if name == "labels":
            gnn.set_labels(labels, train, heads="mean")
        else:
            gnn.set_multilabel_targets(targets, train, heads="mean", pos_weight=pw)

    def timed(fn):
        w.sync()
        t = time.perf_counter()
        fn()
        w.sync()
        return time.perf_counter() - t

    last = {}
    for name in names:  # allocates each head's buffers and warms it up
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
        print("GAT [15d_fusion2, attention softmax, score additive, head %s%s] 2^%d vertices, %d nnz, 14 heads, %d classes: train_step %.1f ms "
              "(min %.1f .. max %.1f) over %d; last pair (%.4f, %.4f)" %
              (name, " on " + os.path.basename(os.path.dirname(lib)) + "/" + os.path.basename(lib) if lib else "", logm, nnz, classes, t.mean(), t.min(), t.max(), reps,
               last[name][0], last[name][1]))
    if "multilabel" in names:
        a, b = np.array(tt["labels"]) * 1e3, np.array(tt["multilabel"]) * 1e3
        spread = a.max() - a.min()
        diff = np.median(b) - np.median(a)
        print("multilabel - labels (medians): %+.2f ms; the spread of the set_labels rounds is %.2f ms: %s" %
              (diff, spread, "within" if abs(diff) <= spread else "OUTSIDE it"))
    for h in (x, gnn, op):
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
