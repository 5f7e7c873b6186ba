"""What the GAT's CPU test files share: the header scan, the small finite-difference problem, the operator on the test double, and the
recorded results that pin the numpy definition (tests/gat_ref.py)."""
import os
import re

import numpy as np

import hnh_testlib as T
from distributed_sddmm_amd import api as H
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(hnh_[a-z0-9_]+)\s*\(", txt))


def fd_problem():
    """The small ER graph of the CPU tests (32 vertices, 123 nonzeros) plus one repeated pair, T.GAT_LAYERS, weights of the usual
    1 / sqrt(fan-in) scale and a1, a2 of order one.  Seed 5: every pre-activation of the reference is more than 1000 steps from 0."""
    rows, cols = O.erdos_renyi(5, 4)
    rows, cols = np.concatenate([rows, rows[:1]]), np.concatenate([cols, cols[:1]])
    m = 32
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (m, T.GAT_LAYERS[0][0]))
    w = {(li, h): rng.standard_normal((fin, fph)) / np.sqrt(fin) for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS) for h in range(heads)}
    av = {(li, h): (rng.standard_normal(fph), rng.standard_normal(fph)) for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS) for h in range(heads)}
    g = O.dense_fill(m, T.GAT_LAYERS[-1][1] * T.GAT_LAYERS[-1][2], 9) * 16.0  # dL/d(out) of L = <g, out>
    return rows, cols, m, x, w, av, g


def pinned_error(config, out, dws, das, dx):
    """The worst T.rel of a forward output and a backward result on fd_problem() against tests/golden/gat_ref_pinned.npz: what the
    per-feature reference modules that gat_ref.py replaced computed for `config` (output, every dW, da1, da2 and dX).  Their matrix
    products went through that machine's BLAS, so the comparison is to "same maths, other summation order", 1e-13, not to the bit."""
    pin = np.load(os.path.join(ROOT, "tests", "golden", "gat_ref_pinned.npz"))
    got = {"out": out, "dx": dx}
    got.update({"dw_%d_%d" % k: v for k, v in dws.items()})
    got.update({"da%d_%d_%d" % ((i + 1,) + k): v[i] for k, v in das.items() for i in (0, 1)})
    names = {n.split("/")[1] for n in pin.files if n.startswith(config + "/")}
    assert names == set(got), names ^ set(got)
    return max(float(T.rel(v, pin["%s/%s" % (config, n)])) for n, v in got.items())


def make_gat(world, case, alg, c, layers=None, **kw):
    sp = H.SpmatLocal.from_global(world, case["M"], case["N"], case["rows"], case["cols"], np.ones(len(case["rows"])))
    d = H.DistributedSparse(world, alg, sp, case["R"], c)
    return sp, d, H.GAT(d, layers or T.GAT_LAYERS, T.GAT_ALPHA, **kw)


def plain_output(world, case):
    """The output of a GAT that never heard of any option"""
    sp, d, gnn = make_gat(world, case, "15d_fusion2", 1)
    gnn.forwardPass()
    out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
    gnn.get_output(out)
    res = out.download()
    for h in (out, gnn, d, sp):
        h.free()
    return res
