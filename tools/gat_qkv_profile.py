"""Development tool: time the GAT's score "transformer" (scaled dot-product attention with separate query, key and value projections,
include/hnh_attn_qkv.h) on one GPU, against its yardsticks.

    python tools/gat_qkv_profile.py [logm] [--rounds N]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32.  Scores "dot" (with
                                                    the fused backward) and "transformer", attention softmax, are warmed up (forward and
                                                    backward), then alternate N times (default 2); every pass runs between two device
                                                    synchronisations; min .. max per pass, and the ratio to score dot.
    python tools/gat_qkv_profile.py [logm] --passes [--reps N]
                                                    the three sparse passes alone, through the kernel ABI, on ONE Erdos-Renyi block of
                                                    2^logm rows (default 16), edge factor 32, at f = 64, 128, 256, each next to its yardstick in
                                                    the same process on the same block: the forward pass next to hnh_attn_softmax_csr_p at
                                                    R = 2 f (the same bytes gathered per nonzero), the row pass and the column pass next to
                                                    hnh_attn_grad_col_csr_p at the same f (the same two halves gathered).  N repetitions
                                                    (default 5) alternate after one warm-up each; min .. max in microseconds by device
                                                    events, the pass's share of its byte model at 8 TB/s, and whether its slowest
                                                    repetition stays within the yardstick's.
Under `rocprofv3 --kernel-trace --stats` the run splits into kernels (attn_rows_kernel<AqPass<0 ..>, true> = forward,
attn_rows_kernel / attn_segments_kernel<AqPass<1 ..> ..> = backward row pass, <AqPass<2 ..> ..> = backward column pass; AgPass = score
dot's fused backward; gemm kernels = the three products per head).
"""
import ctypes as C
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def option(argv, name, default):
    if name in argv:
        i = argv.index(name)
        v = int(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def model(argv):
    from distributed_sddmm_amd import api as H
    rounds = option(argv, "--rounds", 2)
    assert H.load_backend(None) == "hip-gfx950"
    modes = ["dot", "transformer"]
    logm = int(argv[1]) if len(argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, layers, 0.2, attention="softmax", backward="fused")
    rng = np.random.default_rng(0)
    for li, (fin, fph, nh) in enumerate(layers):
        for h in range(nh):
            k, n = gnn.weight_shape(li, h)
            gnn.set_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
            gnn.set_query_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
            gnn.set_key_weight(li, h, rng.uniform(-1, 1, (k, n)) / k)
    x = H.Dense.create(w, *gnn.buffer_shape(0))
    x.fill(0.01)
    gnn.set_input(x)
    g = H.Dense.create(w, *gnn.buffer_shape(len(layers)))
    g.fill(1.0)
    for mode in modes:  # allocates each score's buffers and warms it up
        gnn.set_score(mode)
        gnn.forwardPass()
        gnn.backwardPass(g)
    w.sync()
    ft, bt = {m: [] for m in modes}, {m: [] for m in modes}
    for _ in range(rounds):  # alternating, every pass between two device synchronisations
        for mode in modes:
            gnn.set_score(mode)
            w.sync()
            t = time.perf_counter()
            gnn.forwardPass()
            w.sync()
            ft[mode].append(time.perf_counter() - t)
            t = time.perf_counter()
            gnn.backwardPass(g)
            w.sync()
            bt[mode].append(time.perf_counter() - t)
    for mode in modes:
        f, b = np.array(ft[mode]) * 1e3, np.array(bt[mode]) * 1e3
        print("GAT [15d_fusion2, attention softmax, score %s] 2^%d vertices, %d nnz, %d heads: forward %.1f .. %.1f ms, backward %.1f .. %.1f ms over %d"
              % (mode, logm, nnz, heads, f.min(), f.max(), b.min(), b.max(), rounds))
    print("transformer / dot: forward %.3f, backward %.3f (of the minima)" % (min(ft["transformer"]) / min(ft["dot"]), min(bt["transformer"]) / min(bt["dot"])))
    for h in (g, x, gnn, op):
        h.free()


def passes(argv):
    from distributed_sddmm_amd import _kernels as K
    from distributed_sddmm_amd import api as H
    reps = option(argv, "--reps", 5)
    logm = int(argv[1]) if len(argv) > 1 else 16
    m = 1 << logm
    ctx = K.Ctx(0)
    lib = ctx.lib
    rows, cols = H.generate_er(m, m, m * 32, 7)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))]).astype(np.int32)
    nnz = len(cols)
    drp, dci = ctx.upload(rowptr), ctx.upload(np.concatenate([cols, [0]]).astype(np.int32))
    blk = K.CsrBlock(m, nnz, m, int(np.diff(rowptr).max()), 0, drp.ptr, dci.ptr, None)
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        ctx.check(lib.hnh_event_create(ctx.h, C.byref(e)), "event")

    def timed(call):
        ctx.check(lib.hnh_event_record(ctx.h, ev[0], K.STREAM_COMPUTE), "record")
        ctx.check(call(), "pass")
        ctx.check(lib.hnh_event_record(ctx.h, ev[1], K.STREAM_COMPUTE), "record")
        ctx.check(lib.hnh_event_sync(ctx.h, ev[1]), "sync")
        ms = C.c_float()
        ctx.check(lib.hnh_event_elapsed_ms(ctx.h, ev[0], ev[1], C.byref(ms)), "elapsed")
        return ms.value * 1e3

    rng = np.random.default_rng(0)
    print("one block, 2^%d rows, %d nnz, %d repetitions alternating; microseconds, min .. max" % (logm, nnz, reps))
    for f in (64, 128, 256):
        pw0, pw1 = K.attn_grad_packed_width(f, False), K.attn_grad_packed_width(f, True)
        own, own2, dz = (ctx.upload(rng.uniform(-1, 1, (m, f)) / np.sqrt(f)) for _ in range(3))
        kv, wide_x = ctx.upload(rng.uniform(-1, 1, (m, pw0)) / np.sqrt(f)), ctx.upload(rng.uniform(-1, 1, (m, pw0)) / np.sqrt(f))
        packed = np.zeros((m, pw1))
        packed[:, :2 * f] = rng.uniform(-1, 1, (m, 2 * f)) / np.sqrt(f)
        packed[:, 2 * f] = 4.0  # lse: weights below one
        pk = ctx.upload(packed)
        lse, delta, rmax, rsum = (ctx.upload(np.full(m, 4.0)) for _ in range(4))
        acc, acc_wide, out, out2, dst, dst_wide = (K.DevArray(ctx, m * w, np.float64) for w in (f, pw0, f, f, f, pw0))
        vals = K.DevArray(ctx, nnz, np.float64)

        def qkv(pas):
            q = K.AttnQKV()
            q.X, q.ld_x, q.X2, q.ld_x2, q.dZ, q.ld_dz, q.lse, q.delta, q.f, q.scale = own.ptr, f, own2.ptr, f, dz.ptr, f, lse.ptr, delta.ptr, f, 1.0 / np.sqrt(f)
            q.row_max, q.row_sum, q.relu_dst, q.relu_ld = rmax.ptr, rsum.ptr, dst.ptr, f
            q.Y, q.ld_y = (pk.ptr, pw1) if pas == 2 else (kv.ptr, pw0)
            q.Out, q.ld_out, q.Out2, q.ld_out2 = (acc.ptr if pas == 0 else out.ptr), f, out2.ptr, f
            if pas == 0:
                q.values = vals.ptr  # (the yardstick stores its scores too: 8 B per nonzero on either side)
            fn = (lib.hnh_attn_qkv_fwd_csr_p, lib.hnh_attn_qkv_row_csr_p, lib.hnh_attn_qkv_col_csr_p)[pas]
            flags = K.FUSED_OUT_OVERWRITE | (K.ATTN_FINISH if pas == 0 else 0)
            return lambda: fn(ctx.h, C.byref(blk), C.byref(q), flags, None, K.STREAM_COMPUTE)

        st = K.AttnState(rmax.ptr, rsum.ptr, lse.ptr, 0.2, dst_wide.ptr, pw0)
        softmax = lambda: lib.hnh_attn_softmax_csr_p(ctx.h, C.byref(blk), vals.ptr, wide_x.ptr, kv.ptr, acc_wide.ptr, pw0,  # noqa: E731
                                                     K.FUSED_VALUES_OVERWRITE | K.FUSED_OUT_OVERWRITE | K.ATTN_FINISH, C.byref(st), None, K.STREAM_COMPUTE)
        ga = K.AttnGrad()
        ga.X, ga.ld_x, ga.Y, ga.ld_y, ga.Out, ga.ld_out, ga.f, ga.softmax, ga.leaky_alpha = own.ptr, f, pk.ptr, pw1, out.ptr, f, f, 1, 0.2
        grad_col = lambda: lib.hnh_attn_grad_col_csr_p(ctx.h, C.byref(blk), C.byref(ga), K.FUSED_OUT_OVERWRITE, None, K.STREAM_COMPUTE)  # noqa: E731
        runs = {"softmax R=2f": softmax, "grad_col": grad_col, "qkv fwd": qkv(0), "qkv row": qkv(1), "qkv col": qkv(2)}
        t = {k: [] for k in runs}
        for k, call in runs.items():  # warm-up: plans, scratch
            timed(call)
            ctx.sync()
        for _ in range(reps):
            for k, call in runs.items():
                t[k].append(timed(call))
                if k in ("qkv fwd", "softmax R=2f"):  # (the finishing call wrote lse: the backward passes read 4.0 again)
                    lse.set(np.full(m, 4.0))
        fp = f + (f & 1)
        gathered = {"qkv fwd": 16 * fp, "qkv row": 16 * fp, "qkv col": 16 * fp + 16, "softmax R=2f": 16 * fp, "grad_col": 16 * fp + 16}
        for k in runs:
            a = np.array(t[k])
            yard = None if not k.startswith("qkv") else ("softmax R=2f" if k == "qkv fwd" else "grad_col")
            line = "f = %3d  %-13s %8.1f .. %8.1f us   %4.1f %% of %d B/nonzero at 8 TB/s" % (f, k, a.min(), a.max(), 100.0 * gathered[k] * nnz / 8e12 / (a.min() * 1e-6),
                                                                                          gathered[k])
            if yard:
                line += "   max %.1f %s the yardstick's max %.1f (%s)" % (a.max(), "within" if a.max() <= max(t[yard]) else "ABOVE", max(t[yard]), yard)
            print(line)
        for d in (own, own2, dz, kv, wide_x, pk, lse, delta, rmax, rsum, acc, acc_wide, out, out2, dst, dst_wide, vals):
            d.free()
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    drp.free()
    dci.free()
    ctx.close()


if __name__ == "__main__":
    args = list(sys.argv)
    if "--passes" in args:
        args.remove("--passes")
        passes(args)
    else:
        model(args)
