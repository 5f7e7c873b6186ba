"""Development tool: time implicit-feedback ALS (api.ImplicitALS; include/hnh_als_implicit.h: hnh_gram_rows_f64) on one GPU.

    python tools/als_implicit_profile.py [--only kernel|operator] [logm]

Kernel: hnh_gram_rows_f64 in cg mode at 2^20 x 128 and 2^18 x 256 against the COMPOSED sequence of the same build at the same shape
(hnh_gemm_f64, hnh_axpy_f64, hnh_rowdot_f64, hnh_vec_div_f64, three hnh_relu_grad_cols_f64 selects, hnh_cg_step_f64,
hnh_row_scale_add_f64) and against a device-to-device copy of one matrix, the three alternating in one process, five repetitions after a
warm-up of each, every call between two device events, the CG state restored (untimed) in front of every call.  The allowance for the
kernel is the composed median: it replaces passes, so it has no excuse to be slower.  Its fraction of the 7-pass byte model (Out, X, x, r
read; x, r, p written) at the session's measured copy rate is reported with no threshold.  The verdict is printed, a miss included.

Operator: one CG iteration of ImplicitALS.half_step on config 5's shape (Erdos-Renyi 2^logm vertices, default 20, edge factor 96, R = 128,
15d_fusion2, one rank), folded and composed, and one iteration of Distributed_ALS::cg_optimizer in the same session: (t(11 iterations) -
t(1 iteration)) / 10, the three alternating over five rounds after a warm-up of each, embeddings re-initialised (untimed) in front of every
call, every call between two device synchronisations.
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5
SHAPES = [(1 << 20, 128), (1 << 18, 256)]


def kernel(rows, R):
    from distributed_sddmm_amd import _kernels as K
    ctx = K.Ctx(0)
    lib = ctx.lib
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ctx.check(lib.hnh_event_create(ctx.h, C.byref(e)), "event")
    s = K.STREAM_COMPUTE

    def timed(fn):
        ctx.check(lib.hnh_event_record(ctx.h, ev[0], s), "record")
        fn()
        ctx.check(lib.hnh_event_record(ctx.h, ev[1], s), "record")
        ctx.check(lib.hnh_event_sync(ctx.h, ev[1]), "sync")
        ms = C.c_float()
        ctx.check(lib.hnh_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
        return ms.value

    rng = np.random.default_rng(0)
    base = rng.standard_normal((rows, R))
    y = rng.standard_normal((4 * R, R))
    gram = y.T @ y
    # a state with the shape of a half-step's: p = r, Out = what a fused call would leave, rs = <r, r>
    host = dict(out=0.1 * base + 0.01 * np.roll(base, 1, axis=1), x=0.5 * np.roll(base, 2, axis=0), r=base, p=base,
                rs=np.einsum("ij,ij->i", base, base))
    keep = {k: ctx.upload(v) for k, v in host.items()}   # pristine copies
    live = {k: K.DevArray(ctx, v.shape, np.float64) for k, v in host.items()}
    g = ctx.upload(gram)
    tmp = K.DevArray(ctx, (rows, R), np.float64)
    vec = {k: K.DevArray(ctx, rows, np.float64) for k in ("bdot", "quot", "alpha", "beta", "rsnew")}
    del base, host

    def restore():
        for k in keep:
            ctx.check(lib.hnh_memcpy(ctx.h, live[k].ptr, keep[k].ptr, keep[k].nbytes, K.D2D, s), "restore")

    def folded():
        cg = K.GramCg(live["x"].ptr, live["r"].ptr, live["p"].ptr, live["rs"].ptr)
        ctx.check(lib.hnh_gram_rows_f64(ctx.h, live["out"].ptr, live["p"].ptr, g.ptr, rows, R, None, C.byref(cg), s), "hnh_gram_rows_f64")

    def select(out, value, cond):
        ctx.check(lib.hnh_relu_grad_cols_f64(ctx.h, out.ptr, 1, value.ptr, 1, cond.ptr, 1, 0, rows, 1, s), "select")

    def composed():
        o, x, r, p, rs = (live[k].ptr for k in ("out", "x", "r", "p", "rs"))
        ctx.check(lib.hnh_gemm_f64(ctx.h, rows, R, R, p, g.ptr, tmp.ptr, s), "gemm")
        ctx.check(lib.hnh_axpy_f64(ctx.h, o, tmp.ptr, 1.0, rows * R, s), "axpy")
        ctx.check(lib.hnh_rowdot_f64(ctx.h, p, o, vec["bdot"].ptr, rows, R, s), "rowdot")
        ctx.check(lib.hnh_vec_div_f64(ctx.h, vec["quot"].ptr, rs, vec["bdot"].ptr, rows, s), "div")
        select(vec["alpha"], vec["quot"], vec["bdot"])
        ctx.check(lib.hnh_cg_step_f64(ctx.h, x, r, p, o, vec["alpha"].ptr, vec["rsnew"].ptr, rows, R, s), "cg_step")
        ctx.check(lib.hnh_vec_div_f64(ctx.h, vec["quot"].ptr, vec["rsnew"].ptr, rs, rows, s), "div")
        select(vec["beta"], vec["quot"], live["rs"])
        select(vec["quot"], vec["beta"], vec["bdot"])
        ctx.check(lib.hnh_row_scale_add_f64(ctx.h, p, vec["quot"].ptr, 1.0, r, None, 1.0, rows, R, s), "row_scale_add")

    def copy():
        ctx.check(lib.hnh_memcpy(ctx.h, tmp.ptr, keep["r"].ptr, keep["r"].nbytes, K.D2D, s), "copy")

    calls = {"copy": copy, "folded": folded, "composed": composed}
    results = {}
    for name, fn in calls.items():  # warm-up of each, and what the two modes compute
        restore()
        timed(fn)
        if name != "copy":
            results[name] = {k: live[k].get() for k in ("x", "r", "p")}
    worst = max(float(np.max(np.abs(results["folded"][k] - results["composed"][k])) / np.max(np.abs(results["composed"][k]))) for k in ("x", "r", "p"))
    t = {k: [] for k in calls}
    for _ in range(REPS):  # alternating
        for name, fn in calls.items():
            restore()
            t[name].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    nbytes = rows * R * 8
    rate = 2 * nbytes / med["copy"] / 1e9  # TB/s: a copy reads and writes the matrix
    model = 7 * nbytes / (rate * 1e9)      # ms for the seven passes at that rate
    print("hnh_gram_rows_f64 (cg) at %d x %d (%.0f MB per matrix); folded and composed agree to %.1e:" % (rows, R, nbytes / 1e6, worst))
    for k, v in t.items():
        print("  %-8s median %.4f ms (min %.4f .. max %.4f over %d)" % (k, med[k], min(v), max(v), REPS))
    print("  folded: median %.4f ms against the composed median %.4f ms: %s (%.2f x); the device copy moves %.2f TB/s, the 7-pass byte model "
          "at that rate is %.4f ms: the kernel runs at %.2f of it" %
          (med["folded"], med["composed"], "within" if med["folded"] <= med["composed"] else "MISSES it", med["folded"] / med["composed"], rate, model,
           model / med["folded"]))
    for a in list(keep.values()) + list(live.values()) + list(vec.values()) + [g, tmp]:
        a.free()
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    ctx.close()


def operator(logm):
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    w = H.World.single(0)
    ef, r = 96, 128
    sp = H.SpmatLocal.load_tuples(w, False, logm, ef)
    nnz = sp.info()["dist_nnz"]
    op = H.DistributedSparse(w, "15d_fusion2", sp, r, 1)
    ws, wst = op.like_S_values(3.0), op.like_ST_values(3.0)
    ials = H.ImplicitALS(op, 0.1)
    ials.set_confidence(ws, wst)
    als = H.DistributedALS(op, True)

    def timed(fn):
        w.sync()
        t = time.perf_counter()
        fn()
        w.sync()
        return (time.perf_counter() - t) * 1e3

    def implicit(folded):
        def run(iters):
            ials.set_folded(folded)
            ials.initializeEmbeddings()
            return timed(lambda: ials.half_step(H.AMAT, iters))
        return run

    def reference(iters):
        als.initializeEmbeddings()
        return timed(lambda: als.cg_optimizer(H.AMAT, iters))

    calls = {"Distributed_ALS": reference, "implicit folded": implicit(True), "implicit composed": implicit(False)}
    for fn in calls.values():  # warm-up: allocates each path's buffers
        fn(1)
    per = {k: [] for k in calls}
    for _ in range(REPS):  # alternating
        for name, fn in calls.items():
            one, eleven = fn(1), fn(11)
            per[name].append((eleven - one) / 10)
    med = {k: float(np.median(v)) for k, v in per.items()}
    print("one CG iteration, Erdos-Renyi 2^%d vertices, %d nnz, R = %d, 15d_fusion2 on one rank, (t(11) - t(1)) / 10:" % (logm, nnz, r))
    for k, v in per.items():
        print("  %-17s median %.2f ms (min %.2f .. max %.2f over %d)" % (k, med[k], min(v), max(v), REPS))
    print("  folded / Distributed_ALS = %.2f, composed / Distributed_ALS = %.2f, folded / composed = %.2f: %s is the faster mode" %
          (med["implicit folded"] / med["Distributed_ALS"], med["implicit composed"] / med["Distributed_ALS"],
           med["implicit folded"] / med["implicit composed"], "folded" if med["implicit folded"] <= med["implicit composed"] else "composed"))
    ials.set_folded(True)
    ials.initializeEmbeddings()
    l0 = ials.loss()
    ials.run(1, 3)
    print("  loss %.6e -> %.6e after one alternating step of 3 iterations" % (l0, ials.loss()))
    for h in (ials, als, ws, wst, op):
        h.free()


def main():
    argv = list(sys.argv)
    only = None
    if "--only" in argv:
        i = argv.index("--only")
        only = argv[i + 1]
        del argv[i:i + 2]
    if only not in (None, "kernel", "operator"):
        sys.exit(__doc__)
    if only != "operator":
        for rows, R in SHAPES:
            kernel(rows, R)
    if only != "kernel":
        operator(int(argv[1]) if len(argv) > 1 else 20)


if __name__ == "__main__":
    main()
