"""Development tool: time top-k recommendation (api.ImplicitALS.recommend; include/hnh_topk.h: hnh_topk_rows_f64) on one GPU.

    python tools/als_topk_profile.py [--only kernel|operator] [logm]

Kernel: hnh_topk_rows_f64 (splits = 0, no exclusion lists) for nq = 1024 queries against n = 2^20 items at R = 128 and n = 2^18 at
R = 256, each at k = 10 and k = 100, and for nq = 16 at the first shape (the latency case), against the UNFUSED route on the same device
and operands in the same process: torch.matmul(Q, Y.T) in fp64, which writes the nq x n score matrix, followed by torch.topk(k), which
reads it back.  The two alternate, five repetitions after a warm-up of each, every call between two device events of its own stream with
the device idle in front of it.  The allowance for the kernel is the yardstick's median plus the yardstick's own spread (max - min).  It is
also set against the model max(2 nq n R / fp64 matrix peak, 8 n R ceil(nq / 128) / the session's device-copy rate): 128 is the query tile
of a workgroup, so Y is read once per 128 queries.  Verdicts are printed, a miss included.  The two routes' results are compared (ids equal
except where two scores are within rounding; scores to 1e-11).

Operator: recommend end to end (gather of the queries' rows, exclusion lists, kernel, download) for 1024 users on config 5's shape
(Erdos-Renyi 2^logm vertices, default 20, edge factor 96, R = 128, 15d_fusion2, one rank), with and without filter_seen; the first
filtered call, which reads the stored pairs' coordinates back and caches them, is reported on its own.
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5
FP64_MATRIX_PEAK = 78.6e12  # MI355X, FLOP/s
QUERY_TILE = 128
CASES = [(1024, 1 << 20, 128, 10), (1024, 1 << 20, 128, 100), (1024, 1 << 18, 256, 10), (1024, 1 << 18, 256, 100), (16, 1 << 20, 128, 10),
         (16, 1 << 20, 128, 100)]


def kernel():
    import torch
    from distributed_sddmm_amd import _kernels as K
    ctx = K.Ctx(0)
    lib = ctx.lib
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ctx.check(lib.hnh_event_create(ctx.h, C.byref(e)), "event")
    s = K.STREAM_COMPUTE
    dev = torch.device("cuda:0")

    def timed_ours(fn):
        torch.cuda.synchronize()
        ctx.check(lib.hnh_event_record(ctx.h, ev[0], s), "record")
        fn()
        ctx.check(lib.hnh_event_record(ctx.h, ev[1], s), "record")
        ctx.check(lib.hnh_event_sync(ctx.h, ev[1]), "sync")
        ms = C.c_float()
        ctx.check(lib.hnh_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
        return ms.value

    def timed_torch(fn):
        ctx.sync()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), out

    operands = {}
    for nq, n, R, k in CASES:
        if (n, R) not in operands:
            operands.clear()
            g = torch.Generator(device=dev).manual_seed(n + R)
            operands[(n, R)] = (torch.randn((1024, R), dtype=torch.float64, device=dev, generator=g),
                                torch.randn((n, R), dtype=torch.float64, device=dev, generator=g))
        Qall, Y = operands[(n, R)]
        Q = Qall[:nq].contiguous()
        need = lib.hnh_topk_rows_f64_workspace(nq, n, R, k)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out_s = torch.empty((nq, k), dtype=torch.float64, device=dev)
        out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
        spare = torch.empty_like(Y)

        def fused():
            ctx.check(lib.hnh_topk_rows_f64(ctx.h, Q.data_ptr(), nq, Y.data_ptr(), n, R, 0, None, None, k, 0, out_s.data_ptr(), out_i.data_ptr(),
                                            work.data_ptr(), need, s), "hnh_topk_rows_f64")

        def unfused():
            return torch.topk(torch.matmul(Q, Y.T), k, dim=1)

        def copy():
            spare.copy_(Y)

        timed_ours(fused)
        _, ref = timed_torch(unfused)
        timed_torch(copy)
        same = float((out_i == ref.indices).double().mean())
        close = float(((out_s - ref.values).abs().max() / ref.values.abs().max()))
        del ref
        t = {"fused": [], "unfused": [], "copy": []}
        for _ in range(REPS):  # alternating
            t["fused"].append(timed_ours(fused))
            t["unfused"].append(timed_torch(unfused)[0])
            t["copy"].append(timed_torch(copy)[0])
        med = {name: float(np.median(v)) for name, v in t.items()}
        rate = 2 * n * R * 8 / (med["copy"] * 1e-3)  # bytes/s: a copy reads and writes Y
        flop_ms = 2.0 * nq * n * R / FP64_MATRIX_PEAK * 1e3
        byte_ms = 8.0 * n * R * -(-nq // QUERY_TILE) / rate * 1e3
        model = max(flop_ms, byte_ms)
        allowance = med["unfused"] + (max(t["unfused"]) - min(t["unfused"]))
        print("hnh_topk_rows_f64 nq = %d, n = %d, R = %d, k = %d (ids equal to torch.topk's at %.4f of the places, scores to %.1e):" % (nq, n, R, k, same, close))
        for name, v in t.items():
            print("  %-8s median %.4f ms (min %.4f .. max %.4f over %d)" % (name, med[name], min(v), max(v), REPS))
        print("  fused: median %.4f ms against the allowance %.4f ms (unfused median + its spread): %s (%.2f x the unfused median); the device copy "
              "moves %.2f TB/s; model max(%.4f ms of fp64 matrix peak, %.4f ms of bytes) = %.4f ms: the kernel runs at %.2f of it, %s" %
              (med["fused"], allowance, "within" if med["fused"] <= allowance else "MISSES it", med["fused"] / med["unfused"], rate / 1e12, flop_ms, byte_ms,
               model, model / med["fused"], "bound by " + ("compute" if flop_ms >= byte_ms else "bytes")))
        sys.stdout.flush()
        del work, out_s, out_i, spare
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    ctx.close()


def operator(logm):
    from distributed_sddmm_amd import api as H
    assert H.load_backend(None) == "hip-gfx950"
    w = H.World.single(0)
    ef, r, nq = 96, 128, 1024
    sp = H.SpmatLocal.load_tuples(w, False, logm, ef)
    nnz = sp.info()["dist_nnz"]
    op = H.DistributedSparse(w, "15d_fusion2", sp, r, 1)
    ials = H.ImplicitALS(op, 0.1)
    ials.initializeEmbeddings()
    users = np.random.default_rng(0).choice(1 << logm, size=nq, replace=False).astype(np.int64)

    def timed(filter_seen, k):
        w.sync()
        t = time.perf_counter()
        ials.recommend(users, k, filter_seen)
        return (time.perf_counter() - t) * 1e3

    print("recommend for %d users, Erdos-Renyi 2^%d vertices, %d nnz, R = %d, 15d_fusion2 on one rank, end to end:" % (nq, logm, nnz, r))
    timed(False, 10)  # warm-up
    print("  the first call with filter_seen (reads the stored pairs' coordinates back and caches them): %.1f ms" % timed(True, 10))
    for k in (10, 100):
        t = {True: [], False: []}
        for _ in range(REPS):  # alternating
            for f in (False, True):
                t[f].append(timed(f, k))
        for f in (False, True):
            print("  k = %-3d filter_seen = %-5s median %.2f ms (min %.2f .. max %.2f over %d)" % (k, f, float(np.median(t[f])), min(t[f]), max(t[f]), REPS))
        print("  k = %-3d the exclusion lists (host scan of %d pairs, upload, the kernel's searches) cost %.2f ms per call" %
              (k, nnz, float(np.median(t[True])) - float(np.median(t[False]))))
    for h in (ials, op):
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
        kernel()
    if only != "kernel":
        operator(int(argv[1]) if len(argv) > 1 else 20)


if __name__ == "__main__":
    main()
