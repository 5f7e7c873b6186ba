"""Development tool: time the learned per-edge bias of the GAT's score "transformer" (include/hnh_attn_edge_grad.h,
GAT.set_edge_bias_learned) on one GPU, against the same build's passes with a fixed bias.

    python tools/gat_edge_grad_profile.py [logm] [--rounds N]
                                                    15d_fusion2, c = 1, the layers of benchmark_dist.cpp:93-95 (14 heads of 256
                                                    features), Erdos-Renyi 2^logm vertices (default 18), edge factor 32, score
                                                    "transformer", attention softmax, a bias on every layer (edge_bias_from of a hash of
                                                    the coordinates): not learned and learned on every layer, warmed up, then alternating
                                                    N times (default 2); backwardPass and train_step (Adam) each between two device
                                                    synchronisations; min .. max, and the ratio learned / fixed.
    python tools/gat_edge_grad_profile.py [logm] --passes [--reps N]
                                                    the two backward passes alone, through the kernel ABI, on ONE Erdos-Renyi block of
                                                    2^logm rows (default 16), edge factor 32, at f = 64, 128, 256: each grad pass,
                                                    overwriting and accumulating, next to its yardstick, the hnh_attn_qkv_bias_* pass of
                                                    the same build on the same block and operands.  N repetitions (default 5) alternate
                                                    after one warm-up each; min .. max in microseconds by device events.  The byte model
                                                    per nonzero: (16 fp + 16) / (16 fp + 8) for the row pass and (16 fp + 32) / (16 fp + 24)
                                                    for the column pass, 8 B more in the numerator when accumulating; a pass meets its
                                                    expectation if its minimum is within that ratio times the yardstick's minimum, widened
                                                    by the yardstick's own (max - min) / min of the session.
Under `rocprofv3 --kernel-trace --stats` the grad instances are attn_rows_kernel / attn_segments_kernel<AqPass<.., true, true>, ..>.
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


def hash_bias(rows, cols):
    h = (np.asarray(rows, dtype=np.uint64) * np.uint64(2654435761) + np.asarray(cols, dtype=np.uint64) * np.uint64(40503)) % np.uint64(4093)
    return -2.0 + 4.0 * h.astype(np.float64) / 4093.0


def model(argv):
    from distributed_sddmm_amd import api as H
    rounds = option(argv, "--rounds", 2)
    assert H.load_backend(None) == "hip-gfx950"
    modes = ["fixed", "learned"]
    logm = int(argv[1]) if len(argv) > 1 else 18
    w = H.World.single(0)
    sp = H.SpmatLocal.load_tuples(w, False, logm, 32)
    nnz = sp.info()["dist_nnz"]
    layers = [(256, 256, 4), (1024, 256, 4), (1024, 256, 6)]  # benchmark_dist.cpp:93-95
    heads = sum(l[2] for l in layers)
    op = H.DistributedSparse(w, "15d_fusion2", sp, 256, 1)
    gnn = H.GAT(op, layers, 0.2, attention="softmax", score="transformer")
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
    gnn.edge_bias_from(hash_bias)
    m = 1 << logm
    gnn.set_labels(rng.integers(0, layers[-1][1], m).astype(np.int32), rng.random(m) < 0.3, heads="mean")
    gnn.set_optimizer("adam", 1e-3, weight_decay=5e-4)

    def select(mode):
        for li in range(len(layers)):
            gnn.set_edge_bias_learned(li, mode == "learned")

    for mode in modes:  # warms each mode up
        select(mode)
        gnn.forwardPass()
        gnn.backwardPass(g)
        gnn.train_step()
    w.sync()
    bt, tt = {m: [] for m in modes}, {m: [] for m in modes}
    for _ in range(rounds):  # alternating, every section between two device synchronisations
        for mode in modes:
            select(mode)
            gnn.forwardPass()
            w.sync()
            t = time.perf_counter()
            gnn.backwardPass(g)
            w.sync()
            bt[mode].append(time.perf_counter() - t)
            t = time.perf_counter()
            gnn.train_step()
            w.sync()
            tt[mode].append(time.perf_counter() - t)
    for mode in modes:
        b, t = np.array(bt[mode]) * 1e3, np.array(tt[mode]) * 1e3
        print("GAT [15d_fusion2, attention softmax, score transformer, edge bias %s] 2^%d vertices, %d nnz, %d heads: backward %.1f .. %.1f ms, train_step %.1f .. %.1f ms over %d"
              % (mode, logm, nnz, heads, b.min(), b.max(), t.min(), t.max(), rounds))
    print("learned / fixed: backward %.3f, train_step %.3f (of the minima)" % (min(bt["learned"]) / min(bt["fixed"]), min(tt["learned"]) / min(tt["fixed"])))
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
    bias = ctx.upload(hash_bias(rows, cols))
    dbias = ctx.upload(np.zeros(nnz))
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
    names = ("fwd", "row", "col")
    for f in (64, 128, 256):
        pw0, pw1 = K.attn_grad_packed_width(f, False), K.attn_grad_packed_width(f, True)
        own, own2, dz = (ctx.upload(rng.uniform(-1, 1, (m, f)) / np.sqrt(f)) for _ in range(3))
        kv = ctx.upload(rng.uniform(-1, 1, (m, pw0)) / np.sqrt(f))
        packed = np.zeros((m, pw1))
        fp = f + (f & 1)
        packed[:, :f] = rng.uniform(-1, 1, (m, f)) / np.sqrt(f)
        packed[:, fp:fp + f] = rng.uniform(-1, 1, (m, f)) / np.sqrt(f)
        packed[:, 2 * fp] = 6.0  # lse: weights below one with a bias in [-2, 2)
        pk = ctx.upload(packed)
        lse, delta = (ctx.upload(np.full(m, 6.0)) for _ in range(2))
        out, out2 = (K.DevArray(ctx, m * f, np.float64) for _ in range(2))

        def qkv(pas, mode):
            q = K.AttnQKV()
            q.X, q.ld_x, q.X2, q.ld_x2, q.dZ, q.ld_dz, q.lse, q.delta, q.f, q.scale = own.ptr, f, own2.ptr, f, dz.ptr, f, lse.ptr, delta.ptr, f, 1.0 / np.sqrt(f)
            q.Y, q.ld_y = (pk.ptr, pw1) if pas == 2 else (kv.ptr, pw0)
            q.Out, q.ld_out, q.Out2, q.ld_out2 = out.ptr, f, out2.ptr, f
            flags = K.FUSED_OUT_OVERWRITE
            if mode == "bias":
                fn = (None, lib.hnh_attn_qkv_bias_row_csr_p, lib.hnh_attn_qkv_bias_col_csr_p)[pas]
                return lambda: fn(ctx.h, C.byref(blk), C.byref(q), bias.ptr, flags, None, K.STREAM_COMPUTE)
            fn = (None, lib.hnh_attn_qkv_bias_grad_row_csr_p, lib.hnh_attn_qkv_bias_grad_col_csr_p)[pas]
            return lambda: fn(ctx.h, C.byref(blk), C.byref(q), bias.ptr, dbias.ptr, 1 if mode == "accum" else 0, flags, None, K.STREAM_COMPUTE)

        runs = {}
        for pas in (1, 2):
            for mode in ("bias", "grad", "accum"):
                runs[mode + " " + names[pas]] = qkv(pas, mode)
        t = {k: [] for k in runs}
        for k, call in runs.items():  # warm-up: plans, scratch
            timed(call)
            ctx.sync()
        for _ in range(reps):
            for k, call in runs.items():
                t[k].append(timed(call))
        for pas in (1, 2):
            y = np.array(t["bias " + names[pas]])
            base = 16 * fp + (24 if pas == 2 else 8)
            spread = (y.max() - y.min()) / y.min()
            for mode, more in (("grad", 8), ("accum", 16)):
                b = np.array(t[mode + " " + names[pas]])
                predicted = (base + more) / base
                allowed = predicted * (1.0 + spread)
                ratio = b.min() / y.min()
                print("f = %3d  %s  bias %8.1f .. %8.1f us   %-5s %8.1f .. %8.1f us   ratio of minima %.4f, byte model %.4f, yardstick's spread %.4f: %s (allowed %.4f)"
                      % (f, names[pas], y.min(), y.max(), mode, b.min(), b.max(), ratio, predicted, spread, "meets" if ratio <= allowed else "MISSES", allowed))
        for d in (own, own2, dz, kv, pk, lse, delta, out, out2):
            d.free()
    for e in ev:
        lib.hnh_event_destroy(ctx.h, e)
    for d in (drp, dci, bias, dbias):
        d.free()
    ctx.close()


if __name__ == "__main__":
    args = list(sys.argv)
    if "--passes" in args:
        args.remove("--passes")
        passes(args)
    else:
        model(args)
