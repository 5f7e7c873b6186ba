"""Development tool: time the exact ranks of implicit-feedback ALS (api.ImplicitALS.rank_of / rank_metrics; include/hnh_rank.h:
hnh_rank_rows_f64) on one GPU.

    python tools/als_rank_profile.py [--only kernel|operator] [logm]

Kernel: hnh_rank_rows_f64 (splits = 0) for nq = 1024 queries against n = 2^20 items at R = 128 and n = 2^18 at R = 256, with ONE target per
query and with 16, against the yardstick hnh_topk_rows_f64 at k = 10 without exclusion lists on the same device and operands in the same
process: the same product loop with a heavier epilogue.  The three alternate, five repetitions after a warm-up of each, every call between
two device events of its own stream with the device idle in front of it.  With one target the allowance is the yardstick's median plus the
yardstick's own spread (max - min), and the verdict is printed, a miss included; with 16 targets the time is reported, not judged.  The
targets are items of the yardstick's lists with the yardstick's scores, so the counts are checked on the way: the j-th item of a list has
j items before it.

Operator: one rank_metrics call (and the rank_of calls inside it) on config 5's shape (Erdos-Renyi 2^logm vertices, default 20, edge
factor 96, R = 128, 15d_fusion2, one rank) for 1024 held-out pairs of 1024 users, end to end, with and without filter_seen.
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS = 5
CASES = [(1024, 1 << 20, 128), (1024, 1 << 18, 256)]


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

    def timed(fn):
        torch.cuda.synchronize()
        ctx.sync()
        ctx.check(lib.hnh_event_record(ctx.h, ev[0], s), "record")
        fn()
        ctx.check(lib.hnh_event_record(ctx.h, ev[1], s), "record")
        ctx.check(lib.hnh_event_sync(ctx.h, ev[1]), "sync")
        ms = C.c_float()
        ctx.check(lib.hnh_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
        return ms.value

    for nq, n, R in CASES:
        k = 10
        g = torch.Generator(device=dev).manual_seed(n + R)
        Q = torch.randn((nq, R), dtype=torch.float64, device=dev, generator=g)
        Y = torch.randn((n, R), dtype=torch.float64, device=dev, generator=g)
        need = lib.hnh_topk_rows_f64_workspace(nq, n, R, 16)
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out_s = torch.empty((nq, 16), dtype=torch.float64, device=dev)
        out_i = torch.empty((nq, 16), dtype=torch.int64, device=dev)
        # the targets: the first 16 of every query's list (one call with k = 16), with the scores the kernel itself returned
        ctx.check(lib.hnh_topk_rows_f64(ctx.h, Q.data_ptr(), nq, Y.data_ptr(), n, R, 0, None, None, 16, 0, out_s.data_ptr(), out_i.data_ptr(),
                                        work.data_ptr(), need, s), "hnh_topk_rows_f64")
        ctx.sync()
        runs = {}
        for per in (1, 16):
            tgt_s, tgt_i = out_s[:, :per].contiguous(), out_i[:, :per].contiguous()
            ptr = (per * np.arange(nq + 1)).astype(np.int64)
            rneed = lib.hnh_rank_rows_f64_workspace(nq, n, nq * per, 0)
            runs[per] = dict(s=tgt_s, i=tgt_i, ptr=ptr, need=rneed, work=torch.empty(max(rneed, 16), dtype=torch.uint8, device=dev),
                             counts=torch.full((nq, per), -1, dtype=torch.int64, device=dev))
        top_s = torch.empty((nq, k), dtype=torch.float64, device=dev)
        top_i = torch.empty((nq, k), dtype=torch.int64, device=dev)

        def yardstick():
            ctx.check(lib.hnh_topk_rows_f64(ctx.h, Q.data_ptr(), nq, Y.data_ptr(), n, R, 0, None, None, k, 0, top_s.data_ptr(), top_i.data_ptr(),
                                            work.data_ptr(), need, s), "hnh_topk_rows_f64")

        def rank(per):
            r = runs[per]
            ctx.check(lib.hnh_rank_rows_f64(ctx.h, Q.data_ptr(), nq, Y.data_ptr(), n, R, 0, r["ptr"].ctypes.data, r["s"].data_ptr(), r["i"].data_ptr(), 0,
                                            r["counts"].data_ptr(), r["work"].data_ptr(), r["need"], s), "hnh_rank_rows_f64")

        names = {"topk k=10": yardstick, "rank 1": lambda: rank(1), "rank 16": lambda: rank(16)}
        for fn in names.values():  # warm-up
            timed(fn)
        for per in (1, 16):
            want = torch.arange(per, device=dev).expand(nq, per)
            assert torch.equal(runs[per]["counts"], want), "the j-th item of a list has j items before it"
        t = {name: [] for name in names}
        for _ in range(REPS):  # alternating
            for name, fn in names.items():
                t[name].append(timed(fn))
        med = {name: float(np.median(v)) for name, v in t.items()}
        allowance = med["topk k=10"] + (max(t["topk k=10"]) - min(t["topk k=10"]))
        print("hnh_rank_rows_f64 nq = %d, n = %d, R = %d (counts equal the list indices):" % (nq, n, R))
        for name, v in t.items():
            print("  %-10s median %.4f ms (min %.4f .. max %.4f over %d)" % (name, med[name], min(v), max(v), REPS))
        print("  one target per query: median %.4f ms against the allowance %.4f ms (the yardstick's median + its spread): %s (%.3f x the yardstick's median)" %
              (med["rank 1"], allowance, "within" if med["rank 1"] <= allowance else "MISSES it", med["rank 1"] / med["topk k=10"]))
        print("  16 targets per query: median %.4f ms, %.3f x the yardstick's median, %.3f x one target (reported, not judged)" %
              (med["rank 16"], med["rank 16"] / med["topk k=10"], med["rank 16"] / med["rank 1"]))
        sys.stdout.flush()
        del runs, work, Q, Y
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
    rng = np.random.default_rng(0)
    users = rng.choice(1 << logm, size=nq, replace=False).astype(np.int64)
    items = rng.integers(0, 1 << logm, nq).astype(np.int64)

    def timed(fn):
        w.sync()
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out

    print("rank_metrics for %d held-out pairs of %d users, Erdos-Renyi 2^%d vertices, %d nnz, R = %d, 15d_fusion2 on one rank, end to end:" %
          (nq, nq, logm, nnz, r))
    timed(lambda: ials.rank_of(users, items, False))  # warm-up
    print("  the first call with filter_seen (reads the stored pairs' coordinates back and caches them): %.1f ms" % timed(lambda: ials.rank_of(users, items, True))[0])
    for f in (False, True):
        t_rank = [timed(lambda: ials.rank_of(users, items, f))[0] for _ in range(REPS)]
        t_all, got = zip(*[timed(lambda: ials.rank_metrics(users, items, filter_seen=f)) for _ in range(REPS)])
        print("  filter_seen = %-5s rank_of median %.2f ms (min %.2f .. max %.2f over %d); rank_metrics median %.2f ms (min %.2f .. max %.2f): %s" %
              (f, float(np.median(t_rank)), min(t_rank), max(t_rank), REPS, float(np.median(t_all)), min(t_all), max(t_all), got[0]))
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
