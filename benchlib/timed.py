"""The timed path of bench.py: one route's operator and operands (build), one step of the reference's timed loop
(benchmark_dist.cpp:117-141), the measurement (warm-up, K timed steps bracketed by barrier + device synchronise, max over ranks,
the event-bracketed roofline leg, the result check) and the JSON line made from it."""
import os
import time

from . import checks, common
from .common import GAT_LAYERS, HBM_PEAK, route_name


DUMP_LIMIT = 60 << 20  # bytes of array data --dump-outputs writes in one run (with the .npy headers: under 64 MB)


def sample_rows(m, r, n_arrays, limit=DUMP_LIMIT):
    """Global rows of an m x r float64 output that --dump-outputs writes: all of them when the matrix fits its share of `limit`,
    else a fixed seeded sample, sorted (the same rows for every run of the same size)."""
    import numpy as np
    k = min(m, limit // n_arrays // (8 * r))
    if k == m:
        return np.arange(m, dtype=np.int64)
    return np.sort(np.random.default_rng(12345).choice(m, size=k, replace=False)).astype(np.int64)


def operand_b(m, r, nnz):
    """The constant value of B in the timed loop (A = 1, S = 1).  fusedSpMM overwrites A in place, and with constant operands one call
    multiplies row i of A by deg_i * R * b^2: b = sqrt(M / (R nnz)) makes that deg_i / (mean degree), so the values the timed steps carry
    (and --dump-outputs writes) stay of order one over many steps.  The reference's A = B = 0.001 (benchmark_dist.cpp:102-106) shrink
    them about 80-fold per call at the headline size: exactly zero after some 170 calls."""
    return (m / (r * max(1, nnz))) ** 0.5


def dump_outputs(directory, outputs):
    """Rank 0: one DIR/<name>.npy per output of the last timed step, float64."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    for name, arr in outputs.items():
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))


class Bench:
    """Operator + operands of ONE route at a time, on one of several transports; builds, times and checks it."""

    def __init__(self, args, H, torch, dist, rank, n, dog, workload):
        self.args, self.H, self.torch, self.dist, self.rank, self.n, self.dog, self.wl = args, H, torch, dist, rank, n, dog, workload
        self.transports = {}  # name -> {"world", "sync", "sp", "dead"}
        self.route, self.op, self.A, self.B, self.S, self.buf, self.als, self.gat, self.gat_x = None, None, None, None, None, None, None, None, None
        self.nnz, self.m = None, None
        self.setup_s, self.parse_s = None, None

    # -- transports
    def add_transport(self, name, world, device_sync):
        self.transports[name] = {"world": world, "sync": device_sync, "sp": None, "dead": None}

    def usable(self):
        return [k for k, t in self.transports.items() if t["dead"] is None]

    def world(self, name=None):
        return self.transports[name or self.route[0]]["world"]

    def close_transports(self):
        for t in self.transports.values():
            if t["sp"] is not None:
                t["sp"].free()
                t["sp"] = None
            if t["world"] is not None:
                t["world"].close()
                t["world"] = None

    def barrier(self, name=None):
        t = self.transports[name or self.route[0]]
        if self.dist is not None:
            self.dist.barrier()
        t["world"].sync()
        t["sync"]()

    def max_over_ranks(self, v):
        if self.dist is None:
            return v
        t = self.torch.tensor([v], dtype=self.torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def all_ok(self, ok):
        """True iff every rank says so (a candidate that failed on one rank failed)."""
        if self.dist is None:
            return ok
        t = self.torch.tensor([1.0 if ok else 0.0], dtype=self.torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return bool(t.item() > 0.5)

    # -- one route
    def free_current(self):
        for x in (self.A, self.B, self.S, self.buf, self.gat_x):
            if x is not None:
                x.free()
        for x in (self.als, self.gat):
            if x is not None:
                x.free()
        if self.op is not None:
            self.op.free()
        self.route, self.op, self.A, self.B, self.S, self.buf, self.als, self.gat, self.gat_x = None, None, None, None, None, None, None, None, None

    def build(self, route):
        if route == self.route:
            return
        self.free_current()
        H, args = self.H, self.args
        tr, c, mode, q = route
        t = self.transports[tr]
        if mode in ("mesh", "relay"):
            os.environ["HNH_RING_MODE"] = mode
        if q is not None:
            common.set_chunk_spec(q)
        elif mode == "fusion1":  # (its own default chunk shape, not the previous candidate's: the library reads the same two variables)
            os.environ.pop("HNH_MESH_TAPER", None)
            os.environ.pop("HNH_MESH_CHUNKS", None)
        t0 = time.perf_counter()
        if t["sp"] is None:
            t["sp"] = self.wl.load(H, t["world"])
            t["world"].sync()
            self.parse_s = time.perf_counter() - t0  # generator / file parser + duplicate merge (the tuples are on the device)
            info = t["sp"].info()
            self.nnz, self.m = info["dist_nnz"], info["M"]
        r0 = GAT_LAYERS[0][0] if args.app == "gat" else args.r
        self.op = H.DistributedSparse(t["world"], "15d_fusion1" if mode == "fusion1" else args.alg, t["sp"], r0, c)
        self.route = route
        if args.app == "als":
            self.als = H.DistributedALS(self.op, True)
        elif args.app == "gat":
            self.gat = H.GAT(self.op, GAT_LAYERS, 0.2)
            self.op.setRValue(GAT_LAYERS[0][0])
            self.gat_x = H.Dense.create(t["world"], *self.gat.buffer_shape(0))
            self.gat_x.fill(0.001)
            self.gat.set_input(self.gat_x)
        else:
            self.A, self.B = self.op.like_A_matrix(1.0), self.op.like_B_matrix(operand_b(self.m, args.r, self.nnz))
            self.S, self.buf = self.op.like_S_values(1.0), self.op.like_S_values(0.0)
        self.barrier()
        if self.setup_s is None:
            self.setup_s = time.perf_counter() - t0

    def step(self):
        if self.als is not None:
            self.als.run_cg(1)  # benchmark_dist.cpp:134-137
        elif self.gat is not None:
            self.gat.forwardPass()  # benchmark_dist.cpp:131-133
        else:
            self.op.fusedSpMM(self.A, self.B, self.S, self.buf, self.H.AMAT)

    # -- what a caller of the timed step receives (--dump-outputs)
    def _global_rows(self, dense, mode, m, rows):
        """Rows `rows` (sorted global indices) of the distributed matrix `dense`, laid out as op.submatrices(mode) says, in global order;
        on rank 0 (None elsewhere).  Every element has one owner: the others contribute -inf to a MAX reduction."""
        import numpy as np
        got = dense.download().reshape(-1)
        out = np.full((len(rows), self.op.info()["R"]), -np.inf)
        off = 0
        for top, left, rc, cc in self.op.submatrices(mode):
            keep = int(max(0, min(rc, m - top)))
            blk = got[off:off + rc * cc].reshape(rc, cc)
            off += rc * cc
            lo, hi = np.searchsorted(rows, top), np.searchsorted(rows, top + keep)
            out[lo:hi, left:left + cc] = blk[rows[lo:hi] - top]
        if self.dist is not None:
            t = self.torch.from_numpy(out)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            out = t.numpy()
        if self.rank != 0:
            return None
        assert np.isfinite(out).all(), "bench.py --dump-outputs: an element of the output has no owner"
        return out

    def outputs(self):
        """What the last step computed, as a caller of the step receives it (collective; a dict on rank 0): vanilla -> A (fusedSpMM's
        output, Amat), als -> the embeddings A and B, gat -> H, the last layer's output.  A matrix above its share of DUMP_LIMIT is
        reduced to sample_rows()'s rows."""
        H, info = self.H, self.op.info()
        if self.als is not None:
            A, B = self.op.like_A_matrix(0.0), self.op.like_B_matrix(0.0)
            self.als.get_embeddings(A, B)
            mats = [("A", A, H.AMAT, info["M"]), ("B", B, H.BMAT, info["N"])]
        elif self.gat is not None:
            r_now = info["R"]
            self.op.setRValue(GAT_LAYERS[-1][1] * GAT_LAYERS[-1][2])
            out = H.Dense.create(self.world(), *self.gat.buffer_shape(len(GAT_LAYERS)))
            self.gat.get_output(out)
            mats = [("H", out, H.AMAT, info["M"])]
        else:
            mats = [("A", self.A, H.AMAT, info["M"])]
        r = self.op.info()["R"]
        res = {name: self._global_rows(d, mode, m, sample_rows(m, r, len(mats))) for name, d, mode, m in mats}
        if self.als is not None:
            for d in (A, B):
                d.free()
        elif self.gat is not None:
            out.free()
            self.op.setRValue(r_now)
        return res if self.rank == 0 else None

    # -- the full measurement of the current route
    def measure(self):
        """warm-up, K timed steps (barrier + device synchronise on both sides, max over ranks), what the last one computed (--dump-outputs);
        with --full the roofline leg and the check."""
        args = self.args
        self.dog.phase("warm-up steps [%s]" % route_name(self.route))
        for _ in range(args.warmup):
            self.step()
        self.barrier()
        self.dog.phase("timed steps [%s]" % route_name(self.route))
        t0 = time.perf_counter()
        for _ in range(args.steps):
            self.step()
        self.barrier()
        elapsed = self.max_over_ranks(time.perf_counter() - t0)
        outputs = None
        if args.dump_outputs:
            self.dog.phase("outputs of the last timed step [%s]" % route_name(self.route), max(args.watchdog, 600.0))
            outputs = self.outputs()
        transport_kind = self.op.json_algorithm_info().get("transport", "?")  # (collective: every rank asks)
        ranks = self.world().identities()  # (collective) where every rank runs: pid, device ordinal, PCI bus id, the RCCL communicator's view
        res = {"route": self.route, "elapsed": elapsed, "outputs": outputs, "check": None, "transport_kind": transport_kind, "ranks": ranks}
        if args.full:
            res.update(self.roofline_and_check())
        return res

    def roofline_and_check(self):
        """--full: the event-bracketed roofline leg and the closed-form result check, after the timed steps of measure()."""
        args, torch, dist = self.args, self.torch, self.dist
        self.dog.phase("roofline leg and result check [%s]" % route_name(self.route), max(args.watchdog, 600.0))
        # roofline leg (outside the timed region): HIP events around every local kernel launch
        prof_calls = max(2, min(5, args.steps))
        self.op.kernel_profile(1)
        for _ in range(prof_calls):
            self.step()
        self.world().sync()
        kern_ms, launches = self.op.kernel_profile(0)
        info = self.op.info()
        c_now = self.route[1]
        # SURVEY 8(d), per fused call of this rank: per nonzero 8R + 24 bytes, per output row 16R (row operand read + output row written
        # ONCE) — however many launches the implementation uses (it re-reads rows per launch; that is its cost)
        if args.app == "gat":  # one fused head per (layer, head) at R = features per head
            alg_bytes_per_step = sum(h * (info["nS"] * (8 * f + 24) + 16 * f * info["localArows"] * c_now) for _, f, h in GAT_LAYERS)
        elif args.app == "als":  # run_cg(1): two half-steps of (1 + 1 + 10) fused calls (als_conjugate_gradients.cpp:38-141)
            alg_bytes_per_step = 2 * 12 * (info["nS"] * (8 * args.r + 24) + 16 * args.r * info["localArows"] * c_now)
        else:
            alg_bytes_per_step = info["nS"] * (8 * args.r + 24) + 16 * args.r * info["localArows"] * c_now
        kern_ms_slowest = kern_ms
        if dist is not None:  # per-rank means for the kernel-level figures; the slowest rank's kernel time for what the step exposes
            t = torch.tensor([kern_ms, float(launches), float(alg_bytes_per_step)], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            kern_ms, launches, alg_bytes_per_step = float(t[0]) / self.n, int(t[1]) // self.n, float(t[2]) / self.n
            kern_ms_slowest = self.max_over_ranks(kern_ms_slowest)
        self.barrier()
        check = None
        if not args.no_check:
            check = checks.check(self) if args.app == "vanilla" else checks.check_app(self)
            self.barrier()
        return {"kern_ms": kern_ms, "kern_ms_slowest": kern_ms_slowest, "launches": launches, "prof_calls": prof_calls,
                "alg_bytes_per_step": alg_bytes_per_step, "check": check}


def compose_line(args, b, res, extra):
    """The JSON line of one complete measurement (rank 0); `roofline` only when the measurement ran the roofline leg (--full)."""
    H, n = b.H, b.n
    tr, c_now, mode, q = res["route"]
    ms_per_step = res["elapsed"] / args.steps * 1e3
    value = b.nnz * args.r * args.steps / res["elapsed"]
    ring_mode_now = None if (n == 1 or mode == "none") else ("mesh fetch + mesh reduce-scatter" if mode == "fusion1" else mode)
    alg_now = "15d_fusion1" if mode == "fusion1" else args.alg
    step_is = {"vanilla": "fused SDDMM->SpMM (fusedSpMM, Amat)", "als": "one ALS step by batched CG (run_cg(1): 24 fused calls)",
               "gat": "one GAT forward pass (3 layers, 14 heads)"}[args.app]
    # where the ranks ran, from the ranks themselves: a line of N processes that shared fewer than N GPUs says so in its first sentence
    ranks = res.get("ranks") or []
    distinct = len({r["pci_bus_id"] for r in ranks}) or n
    where = ("%d x MI355X" % n) if distinct == n else ("%d PROCESSES SHARING %d x MI355X (time-sliced: not a scaling number)" % (n, distinct))
    how = "" if n == 1 else ", %s (%s)" % (
        {"rccl": "RCCL over xGMI", "ipc": "ipc-pull, copy engines", "ipc-kernel": "ipc-pull, pull kernel"}.get(tr, "transport: " + tr),
        {"relay": "relay ring", "mesh": "chunked mesh fetch", None: "replication only"}.get(ring_mode_now, ring_mode_now))
    out = {
        "backend": H.backend_name(),
        "metric": "fused SDDMM+SpMM nnz*R/s", "value": value, "unit": "nnz*R/s", "n_gpus": n, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic" if b.wl.kind != "mtx" else "file",
        "config": {"workload": "%s, R=%d, %s, %s c=%d on %s%s" % (b.wl.describe(b.nnz), args.r, step_is, alg_now, c_now, where, how),  # (<= 200 characters in the printed line)
                   "nnz": b.nnz, "M": b.m, "R": args.r, "algorithm": alg_now, "app": args.app, "c": c_now,
                   "transport": "none" if n == 1 else res["transport_kind"],
                   "transport_variant": None if n == 1 else tr, "ring_mode": ring_mode_now,
                   # Q symmetric chunks (a number) or the chunk heights (a comma list)
                   "mesh_chunks": (q if ring_mode_now == "mesh" else None),
                   "rccl_channels": (os.environ.get("NCCL_MAX_NCHANNELS", "default") if n > 1 else None),
                   # compute units masked off the compute stream (the library's default, 0, unless HNH_COMM_CUS says otherwise)
                   "comm_cus": int(os.environ.get("HNH_COMM_CUS", "0") or 0),
                   # set-up of the first route: the tuples (generated on the device, or parsed from the file and merged), then redistribution,
                   # CSR blocks and operands; parse_s is the first part alone
                   "setup_s": round(b.setup_s or 0.0, 2), "parse_s": round(b.parse_s or 0.0, 3),
                   # one record per rank: [rank, pid, device ordinal, PCI bus id] + RCCL's own [ncclCommCount, ncclCommUserRank, ncclCommCuDevice]
                   "distinct_devices": distinct,
                   "ranks": [[r["rank"], r["pid"], r["device_ordinal"], r["pci_bus_id"]] + ([r["comm_count"], r["comm_rank"], r["comm_device"]] if "comm_count" in r else [])
                             for r in ranks]},
    }
    if "kern_ms" in res:
        out["roofline"] = roofline(args, b, res, ms_per_step, mode, ring_mode_now)
    if res["check"] is not None:
        out["check"] = res["check"]
    out.update(extra)
    return out


def roofline(args, b, res, ms_per_step, mode, ring_mode_now):
    """`roofline` of a line, from the roofline leg of a --full measurement."""
    n = b.n
    launches_per_step = max(1, res["launches"] // res["prof_calls"])
    dur = res["kern_ms"] / max(1, res["launches"]) * 1e-3  # average launch duration, seconds
    bytes_per_launch = res["alg_bytes_per_step"] / launches_per_step
    achieved_kernel = bytes_per_launch / dur if dur > 0 else 0.0
    # SURVEY 8(d), the whole step: the GLOBAL problem's algorithmic bytes over the driver-timed step (kernels + every exposed shift,
    # replication and wait — what the reference's elapsed time contains, benchmark_dist.cpp:117-149) against n x the HBM peak
    per_call = lambda r_: common.fused_bytes(b.nnz, r_, b.m)  # noqa: E731
    total_bytes = {"vanilla": per_call(args.r), "als": 2 * 12 * per_call(args.r),
                   "gat": sum(h * per_call(f) for _, f, h in GAT_LAYERS)}[args.app]
    achieved_step = total_bytes / (ms_per_step * 1e-3) / n  # B/s per GPU
    kernel_ms_per_step = res["kern_ms_slowest"] / res["prof_calls"]
    # one GPU: the dominant kernel's own rate (its launches are the step); several GPUs: the step's, exposed communication included
    achieved = achieved_kernel if n == 1 else achieved_step
    # `achieved` is an ALGORITHMIC rate (SURVEY 8d byte model / measured launch time), not DRAM utilisation: part of every
    # launch's gathers is served by the 256 MiB Infinity Cache, which sits behind the counters `traffic` comes from
    return {"bound": "hbm", "bound_detail": "HBM gather model, Infinity-Cache assisted (DESIGN.md 3.2)",
            "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s",
            "frac": achieved / HBM_PEAK, "traffic": None, "traffic_source": None,
            # one GPU: the step IS the dominant kernel's launches; several: SURVEY 8d's whole-step figure, exposed communication counts
            "frac_is": "frac_kernel (one GPU)" if n == 1 else "frac_step = total B_fused / ms_per_step / (n_gpus x 8 TB/s)",
            "frac_kernel": achieved_kernel / HBM_PEAK, "achieved_kernel": achieved_kernel / 1e9,
            "frac_step": achieved_step / HBM_PEAK, "achieved_step_per_gpu": achieved_step / 1e9,
            "algorithmic_bytes_per_step_all_gpus": total_bytes,
            # the slowest rank's event-bracketed kernel time per step, and what the timed step spends beyond it
            "kernel_ms_per_step": kernel_ms_per_step, "exposed_comm_ms": ms_per_step - kernel_ms_per_step,
            "kernel": ("row_kernel<fused>, 1 launch per Infinity-Cache panel of B" if n == 1 else
                       "row_kernel<fused>, 1 launch per visiting block (relay ring)" if ring_mode_now == "relay" else
                       "row_kernel<fused>, the rank's one block (replication only)" if ring_mode_now is None else
                       "row_kernel<sddmm> on row ranges + row_kernel<spmm> staging passes (15d_fusion1, mesh)" if mode == "fusion1" else
                       "row_kernel<fused>: own block + adaptive windowed passes over fetched blocks"),
            # device time of a kernel CALL (HIP events around it on the compute stream) divided by the row-kernel launches it made
            # (structure plans are cached: a steady-state call launches row kernels only)
            "avg_launch_ms": dur * 1e3, "avg_launch_ms_is": "HIP-event time of the call / its row-kernel launches",
            "traffic_rate": None,
            "compulsory_bytes_per_call": 8 * args.r * (2 * b.m + b.m) + 24 * b.nnz,
            "launches_per_step": launches_per_step, "algorithmic_bytes_per_launch": bytes_per_launch,
            "model": "nnz*(8R+24) + 16*R*rows per fused call (SURVEY 8d), split evenly over launches"}
