"""What the top-k GPU tests share (tests/test_als_topk_gpu.py, tests/test_als_topk_edges_gpu.py; include/hnh_topk.h): device buffers
between guard zones, the guarded call of hnh_topk_rows_f64 and of hnh_topk_merge_f64, random operands and exclusion lists, and the builders
of item orders that drive the kernel's selection through its cuts (ordered_case; tests/test_als_topk_cpu.py checks on the CPU that they do,
with lazy_cuts).  A plain module, no conftest: nothing here touches a GPU until a function is called with a ctx."""
import re

import numpy as np

from distributed_sddmm_amd import _kernels as K

GUARD = 128  # bytes in front of and behind every buffer (the buffers keep their alignment)
FILL = 0xA5
KINDS = ("ascending", "descending", "flat", "trickle")
ITEM_TILE = 64  # items of one tile of the kernel's walk over Y


class Guarded:
    """A device buffer of any dtype with guard bytes on both sides; the payload starts `shift` (0 or 8) bytes past a 16-byte-aligned
    position"""

    def __init__(self, ctx, arr, shift=0):
        assert shift in (0, 8)
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype, self.nbytes, self.front = arr.shape, arr.dtype, arr.nbytes, GUARD + shift
        flat = np.concatenate([np.full(self.front, FILL, np.uint8), arr.reshape(-1).view(np.uint8),
                               np.full(GUARD + (-arr.nbytes - shift) % 16, FILL, np.uint8)])
        self.dev = ctx.upload(flat)
        self.ptr = self.dev.ptr + self.front
        assert self.dev.ptr % 16 == 0 and self.ptr % 16 == shift

    def get(self):
        flat = self.dev.get()
        assert np.all(flat[:self.front] == FILL) and np.all(flat[self.front + self.nbytes:] == FILL), "guard bytes overwritten"
        return flat[self.front:self.front + self.nbytes].view(self.dtype).reshape(self.shape).copy()

    def free(self):
        self.dev.free()


class Pack:
    """Several buffers of a call in ONE device allocation, each between guard zones of its own (one allocation, one upload and one
    download per call where a Guarded each costs one of every kind): Pack(ctx, name=(array, shift), ...)"""

    def __init__(self, ctx, **arrays):
        pieces, self.where, at = [], {}, 0
        for name, (arr, shift) in arrays.items():
            assert shift in (0, 8)
            arr = np.ascontiguousarray(arr)
            front, behind = GUARD + shift, (-arr.nbytes - shift) % 16
            pieces += [np.full(front, FILL, np.uint8), arr.reshape(-1).view(np.uint8), np.full(behind, FILL, np.uint8)]
            self.where[name] = (at + front, arr.nbytes, arr.dtype, arr.shape)
            at += front + arr.nbytes + behind
        pieces.append(np.full(GUARD, FILL, np.uint8))
        self.dev = ctx.upload(np.concatenate(pieces))
        assert self.dev.ptr % 16 == 0
        for name, (_, shift) in arrays.items():
            assert self.ptr(name) % 16 == shift

    def ptr(self, name):
        return self.dev.ptr + self.where[name][0]

    def get(self):
        """every buffer as it is now, after checking every byte outside them"""
        flat = self.dev.get()
        end = 0  # (the buffers lie in the order of self.where)
        for name, (at, nbytes, _, _) in self.where.items():
            assert np.all(flat[end:at] == FILL), "guard bytes overwritten in front of " + name
            end = at + nbytes
        assert np.all(flat[end:] == FILL) and len(flat) - end >= GUARD, "guard bytes overwritten at the end"
        return {name: flat[at:at + nbytes].view(dtype).reshape(shape).copy() for name, (at, nbytes, dtype, shape) in self.where.items()}

    def free(self):
        self.dev.free()


class Scratch:
    """Device scratch of `nbytes` (16-byte aligned) between guard zones, for a workspace whose contents are undefined after the call: the
    whole allocation is filled with FILL on the device (a kernel that reads what it has not written reads 0xA5A5...), and check() reads back
    the guard zones only, so that a workspace of a hundred megabytes costs no transfer."""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.total = GUARD + nbytes + (-nbytes) % 16 + GUARD
        self.base = ctx.alloc(self.total)
        self.ptr = self.base + GUARD
        assert self.ptr % 16 == 0
        ctx.check(ctx.lib.hnh_memset(ctx.h, self.base, FILL, self.total, K.STREAM_COMPUTE), "hnh_memset")
        ctx.sync()

    def check(self):
        behind = self.total - GUARD - self.nbytes
        for at, size in ((self.base, GUARD), (self.ptr + self.nbytes, behind)):
            zone = np.zeros(size, np.uint8)
            self.ctx.sync()
            self.ctx.check(self.ctx.lib.hnh_memcpy(self.ctx.h, zone.ctypes.data, at, size, K.D2H, K.STREAM_COMPUTE), "d2h")
            self.ctx.sync()
            assert np.all(zone == FILL), "guard bytes overwritten"

    def free(self):
        self.ctx.free(self.base)


def csr_of(excluded, nq):
    ptr = np.zeros(nq + 1, dtype=np.int64)
    for q in range(nq):
        ptr[q + 1] = ptr[q] + len(excluded[q])
    idx = np.concatenate([np.asarray(e, dtype=np.int32) for e in excluded] + [np.zeros(0, np.int32)]).astype(np.int32)
    return ptr, idx


def topk_rows(ctx, Q, Y, k, id_base=0, excluded=None, splits=0, exact_work=False, shift_q=0, shift_y=0, shift_out=0):
    """hnh_topk_rows_f64 with guard zones around every buffer; checks that they are intact and the inputs unchanged.  Returns (ids,
    scores).  exact_work: the workspace's size is asked of the call itself (a first call with 16 bytes is refused and says how many bytes
    it needs with how many splits), the second call gets exactly that many; returns (ids, scores, that number of splits)."""
    lib = K.load()
    nq, R = Q.shape
    n = Y.shape[0]
    need = lib.hnh_topk_rows_f64_workspace(nq, n, R, k)
    assert need >= 0
    arrays = dict(Q=(Q if nq else np.zeros((1, R)), shift_q), Y=(Y if n else np.zeros((1, R)), shift_y), s=(np.full((max(nq, 1), k), 7.5), shift_out),
                  i=(np.full((max(nq, 1), k), -7, np.int64), shift_out), probe=(np.zeros(16, np.uint8), 0))
    ptr = idx = None
    if excluded is not None:
        ptr, idx = csr_of(excluded, nq)
        arrays.update(ptr=(ptr, 0), idx=(idx if len(idx) else np.zeros(1, np.int32), 0))
    bufs = Pack(ctx, **arrays)

    def call(work_ptr, work_bytes):
        return lib.hnh_topk_rows_f64(ctx.h, bufs.ptr("Q"), nq, bufs.ptr("Y"), n, R, id_base, bufs.ptr("ptr") if excluded is not None else None,
                                     bufs.ptr("idx") if excluded is not None else None, k, splits, bufs.ptr("s"), bufs.ptr("i"), work_ptr, work_bytes,
                                     K.STREAM_COMPUTE)

    said = None
    if exact_work:
        assert call(bufs.ptr("probe"), 16) != 0, "16 bytes of workspace are refused"
        text = lib.hnh_last_error(ctx.h).decode()
        found = re.search(r"(\d+) needed with (\d+) splits", text)
        assert found and "the workspace is too small: 16 bytes" in text, text
        need, said = int(found.group(1)), int(found.group(2))
        assert need > 16 and need % 16 == 0
    work = Scratch(ctx, max(need, 16))
    ctx.check(call(work.ptr, need), "hnh_topk_rows_f64")
    got = bufs.get()
    work.check()
    bufs.free()
    work.free()
    assert np.all(got["probe"] == 0), "a refused call writes nothing"
    if nq:
        assert np.array_equal(got["Q"], Q)
    else:
        assert np.all(got["s"] == 7.5) and np.all(got["i"] == -7), "nothing is written without a query"
    if n:
        assert np.array_equal(got["Y"], Y)
    if excluded is not None:
        assert np.array_equal(got["ptr"], ptr) and (len(idx) == 0 or np.array_equal(got["idx"], idx))
    return (got["i"][:nq], got["s"][:nq], said) if exact_work else (got["i"][:nq], got["s"][:nq])


def topk_merge(ctx, in_s, in_i, k):
    """hnh_topk_merge_f64 of lists laid out [part][nq][k] between guard zones; the inputs come back bit for bit.  Returns (ids, scores)."""
    lib = K.load()
    parts, nq = in_i.shape[:2]
    bufs = [Guarded(ctx, a) for a in (in_s, in_i, np.full((nq, k), 7.5), np.full((nq, k), -7, np.int64))]
    ctx.check(lib.hnh_topk_merge_f64(ctx.h, bufs[0].ptr, bufs[1].ptr, parts, nq, k, bufs[2].ptr, bufs[3].ptr, K.STREAM_COMPUTE), "hnh_topk_merge_f64")
    got = [b.get() for b in bufs]
    for b in bufs:
        b.free()
    assert got[0].tobytes() == in_s.tobytes() and got[1].tobytes() == in_i.tobytes()
    return got[3], got[2]


def integers(rng, shape):
    return rng.integers(-4, 5, shape).astype(np.float64)


def random_lists(rng, nq, n):
    return [np.sort(rng.choice(n, size=int(rng.integers(0, n + 1)) if n < 40 else int(rng.integers(0, 40)), replace=False)) if n else np.zeros(0, np.int64)
            for _ in range(nq)]


# ------------------------------------------------------------------------------------------------ item orders that force the cuts
def ordered_values(kind, n):
    """The sequence v of ordered_case"""
    j = np.arange(n, dtype=np.int64)
    if kind == "ascending":
        return j
    if kind == "descending":
        return n - j
    if kind == "flat":
        return np.full(n, 5, dtype=np.int64)
    assert kind == "trickle", kind
    v = -(j + 1)
    t = np.arange((n + ITEM_TILE - 1) // ITEM_TILE, dtype=np.int64)
    at = ITEM_TILE * t + (7 * t) % ITEM_TILE
    v[at[at < n]] = t[at < n] + 1
    return v


def ordered_case(kind, nq, n, R, seed=0):
    """(Q, Y): Q has integer entries in 1..3 and Y[j] = v_j * ones(R), so that score (q, j) = v_j * sum(Q[q]) is an exact integer and all
    queries order the items alike.  ascending (v_j = j): every item beats all before it, every tile passes for every row.  descending
    (v_j = n - j): nothing passes once a threshold stands.  flat (v_j = 5): all ties, the order is the ids'.  trickle (v_j = -(j + 1), but
    t + 1 at j = 64 t + (7 t mod 64) for every tile t): exactly one item per tile beats the running k-th best."""
    rng = np.random.default_rng([seed, nq, n, R, KINDS.index(kind)])
    Q = rng.integers(1, 4, (nq, R)).astype(np.float64)
    Y = np.repeat(ordered_values(kind, n).astype(np.float64)[:, None], R, axis=1)
    return Q, np.ascontiguousarray(Y)


def lazy_cuts(v, k, cap):
    """The (have, add) of every cut when one row's candidate buffer of `cap` entries is fed the scores v (one query; ties go to the smaller
    index) tile by tile: all items of a 64-tile that rank before the STORED threshold are appended; when they would not fit, the buffer is
    first cut to its first k and the threshold becomes its k-th.  This emulates what the inputs are meant to do, not the kernel."""
    before = lambda a, b: a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])  # noqa: E731
    buf, thr, cuts = [], None, set()
    for t0 in range(0, len(v), ITEM_TILE):
        new = [(int(v[j]), j) for j in range(t0, min(t0 + ITEM_TILE, len(v))) if thr is None or before((int(v[j]), j), thr)]
        if new and len(buf) + len(new) > cap:
            cuts.add((len(buf), len(new)))
            buf = sorted(buf, key=lambda c: (-c[0], c[1]))[:k]
            thr = buf[k - 1]
        buf += new
    return cuts
