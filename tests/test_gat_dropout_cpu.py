"""The GAT's dropout without a GPU: the generator (numpy restatement in tests/gat_pass_ref.py, the host's hnh_dropout_word) against
the published known answers and against each other, the masks' keep statistics, the numpy definition of the masked forward and backward
pass (tests/gat_ref.py with rates) against central finite differences with the mask held fixed, the operands that carry the ids, the optional kernel group of
include/hnh_attn_dropout.h (declared == bound == exported by the HIP library, disjoint from the five existing tables and headers,
absent from the CPU test double), and on the test double: dropout names a kernel of the new group and its header, score "dot" and rates
outside [0, 1) are refused, and the same object then runs the plain GAT bit for bit.

The statistical bounds are 5 sigma of the binomial / of a sample correlation of n independent pairs (sigma = 1 / sqrt(n)); observed on
these inputs: at most 2.2 sigma for the keep rate, 2.4 sigma for the correlations, 3.3 sigma for the worst row of the 1024 x 1024 grid."""
import ctypes as C
import re

import numpy as np
import pytest

import gat_pass_ref as P
import gat_ref as R
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K
from distributed_sddmm_amd import api as H
from gat_cpu_harness import ROOT, declared, fd_problem, make_gat, pinned_error, plain_output

MODE = dict(attention="softmax", score="additive")
GROUP = {"hnh_attn_drop_fwd_csr_p", "hnh_attn_drop_row_csr_p", "hnh_attn_drop_col_csr_p", "hnh_attn_drop_scores_f64", "hnh_attn_drop_pack_f64",
         "hnh_feat_drop_f64", "hnh_dropout_words_u32"}
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
FD_RATES, FD_SEED = (0.6, 0.3), 2
FD = dict(MODE, rates=FD_RATES, seed=FD_SEED)


def host_word(seed, stream, w2, gi, gj):
    return int(H.lib().hnh_dropout_word(int(seed), int(stream), int(w2), int(gi), int(gj)))


@pytest.mark.parametrize("counter,key,want", KNOWN)
def test_known_answers(counter, key, want):
    got = P.philox4x32_10(counter, key)
    assert tuple(int(v) for v in got) == want
    seed = key[0] | (key[1] << 32)
    assert int(P.word(seed, counter[3], counter[2], counter[0], counter[1])) == want[0]
    assert host_word(seed, counter[3], counter[2], counter[0], counter[1]) == want[0]


def test_numpy_and_host_agree_on_random_keys():
    rng = np.random.default_rng(11)
    n = 100000
    gi, gj, w2 = (rng.integers(0, 1 << 32, n, dtype=np.uint64) for _ in range(3))
    stream = rng.integers(0, 2, n)
    seeds = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    want = P.philox4x32_10((gi, gj, w2, stream), (seeds & np.uint64(0xFFFFFFFF), seeds >> np.uint64(32)))[0]
    fn = H.lib().hnh_dropout_word
    got = np.array([fn(int(s), int(t), int(w), int(a), int(b)) for s, t, w, a, b in zip(seeds, stream, w2, gi, gj)], dtype=np.uint32)
    assert np.array_equal(got, want)
    assert gi.max() >= 1 << 31 and seeds.max() >= 1 << 63


def corr(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


@pytest.mark.parametrize("seed", [0, 1, 0x9E3779B97F4A7C15])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.6, 0.9])
def test_keep_statistics(p, seed):
    """Keep rate within 5 sigma of 1 - T / 2^32; no correlation beyond 5 / sqrt(n) with the transposed key, the next head, seed + 1."""
    n = 1 << 20
    rng = np.random.default_rng(1234)
    gi, gj = rng.integers(0, 1 << 22, n), rng.integers(0, 1 << 22, n)
    w2 = 3 * 65536 + 2
    k = P.keep(seed, 0, w2, gi, gj, p)
    rate = 1.0 - P.threshold(p) / 2.0 ** 32
    sig = abs(k.mean() - rate) / np.sqrt(p * (1 - p) / n)
    others = {"transposed": P.keep(seed, 0, w2, gj, gi, p), "next head": P.keep(seed, 0, w2 + 1, gi, gj, p), "seed + 1": P.keep(seed + 1, 0, w2, gi, gj, p)}
    cs = {name: abs(corr(k, o)) * np.sqrt(n) for name, o in others.items()}
    print("observed p=%.1f seed=%x: rate %.2f sigma, correlations %s" % (p, seed, sig, {a: round(b, 2) for a, b in cs.items()}))
    assert abs(k.mean() - rate) <= 5 * np.sqrt(p * (1 - p) / n)
    assert all(v <= 5.0 for v in cs.values()), cs


def test_every_row_of_a_grid_of_consecutive_ids_keeps_its_share():
    p, n = 0.6, 1024
    gi, gj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    k = P.keep(7, 0, 65536 + 1, gi, gj, p)
    rate = 1.0 - P.threshold(p) / 2.0 ** 32
    sig = np.abs(k.mean(axis=1) - rate) / np.sqrt(p * (1 - p) / n)
    print("observed worst row: %.2f sigma" % sig.max())
    assert sig.max() <= 5.0


def test_threshold_and_rates():
    assert P.threshold(0.0) == 0 and P.threshold(0.5) == 1 << 31 and P.threshold(0.6) == K.dropout_threshold(0.6) == int(np.floor(0.6 * 2.0 ** 32))
    assert P.threshold(np.nextafter(1.0, 0.0)) < 1 << 32
    assert np.all(P.keep(5, 0, 0, np.arange(100), np.arange(100), 0.0)), "p = 0 keeps everything"


def fd_masks(rows, cols, m):
    """(all dropped, all kept) rows per (layer, head) at the test's rates and seed"""
    deg = np.bincount(rows, minlength=m)
    out = {}
    for li, (fin, fph, heads) in enumerate(T.GAT_LAYERS):
        for h in range(heads):
            kept = np.bincount(rows, weights=P.keep(FD_SEED, 0, li * 65536 + h, rows, cols, FD_RATES[0]), minlength=m)
            out[(li, h)] = ((deg > 0) & (kept == 0), (deg > 0) & (kept == deg))
    return out


def test_reference_backward_matches_finite_differences():
    """test_gat_additive_cpu.py's problem, step, bound and margin rule, at rates (0.6, 0.3) with the mask held fixed.  Condition on the
    inputs: some head has a row with every edge dropped and a row with every edge kept."""
    rows, cols, m, x, w, av, g = fd_problem()
    layers, alpha, step = T.GAT_LAYERS, T.GAT_ALPHA, 1e-6
    masks = fd_masks(rows, cols, m)
    assert any(d.any() for d, _ in masks.values()) and any(k.any() for _, k in masks.values())
    dws, das, dx = R.backward(rows, cols, m, x, layers, alpha, g, w, av, **FD)
    out, trace = R.forward(rows, cols, m, x, layers, alpha, w, av, keep_trace=True, **FD)
    for (li, h), (dropped, _) in masks.items():
        o, lse = trace[li][3][h][3], trace[li][3][h][4]
        assert np.all(o[dropped] == 0.0) and np.all(lse[dropped] != 0.0), "a row whose edges are all dropped: o = 0, lse kept"

    def loss(ww, aa, xx):
        return float(np.sum(g * R.forward(rows, cols, m, xx, layers, alpha, ww, aa, **FD)))

    def margin_ok(ww, aa, xx, steps=100):
        pre = R.kinks(rows, m, R.pre_activations(rows, cols, m, xx, layers, alpha, ww, aa, **FD))
        return np.abs(pre[pre != 0]).min() >= steps * step

    assert margin_ok(w, av, x)
    assert all(np.abs(a).max() > 0 and np.abs(b).max() > 0 for a, b in das.values())
    assert np.count_nonzero(dx) > dx.size // 2 and all(np.abs(d).max() > 0 for d in dws.values()), "the gradients must not be vacuous"
    assert np.count_nonzero(dx == 0) > 0, "dropped input features have a zero gradient"

    def fd_of(perturb, probes):
        res = []
        for idx in probes:
            plus, minus = perturb(idx, step), perturb(idx, -step)
            assert margin_ok(*plus, steps=99) and margin_ok(*minus, steps=99)
            res.append((loss(*plus) - loss(*minus)) / (2 * step))
        return np.array(res)

    rng = np.random.default_rng(3)
    for key, wk in w.items():
        probes = [(0, 0), (wk.shape[0] - 1, wk.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in wk.shape) for _ in range(3)]

        def perturb(idx, h, key=key, wk=wk):
            ww = dict(w)
            ww[key] = wk.copy()
            ww[key][idx] += h
            return ww, av, x

        an = np.array([dws[key][idx] for idx in probes])
        err = np.max(np.abs(fd_of(perturb, probes) - an)) / np.max(np.abs(an))
        assert err <= 1e-6, (key, err)
    for key, (a1, a2) in av.items():
        for which in (0, 1):
            def perturb(idx, h, key=key, which=which):
                aa = dict(av)
                pair = [av[key][0].copy(), av[key][1].copy()]
                pair[which][idx] += h
                aa[key] = tuple(pair)
                return w, aa, x

            probes = list(range(len(a1)))
            an = das[key][which]
            err = np.max(np.abs(fd_of(perturb, probes) - an)) / np.max(np.abs(an))
            assert err <= 1e-6, (key, which, err)
    probes = [(0, 0), (m - 1, x.shape[1] - 1)] + [tuple(rng.integers(0, s) for s in x.shape) for _ in range(4)]

    def perturb_x(idx, h):
        xx = x.copy()
        xx[idx] += h
        return w, av, xx

    an = np.array([dx[idx] for idx in probes])
    err = np.max(np.abs(fd_of(perturb_x, probes) - an)) / np.max(np.abs(an))
    assert err <= 1e-6, err


def test_passes_with_the_id_operands_equal_the_definition():
    rows, cols, m, x, w, av, g = fd_problem()
    want = R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, **FD)
    got = R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, by_passes=True, **FD)
    for k in want[0]:
        assert T.rel(got[0][k], want[0][k]) <= T.TOL
        assert T.rel(got[1][k][0], want[1][k][0]) <= T.TOL and T.rel(got[1][k][1], want[1][k][1]) <= T.TOL
    assert T.rel(got[2], want[2]) <= T.TOL
    # the forward pass as the kernel takes it, and its extended-precision twin
    _, trace = R.forward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, w, av, keep_trace=True, **FD)
    f = T.GAT_LAYERS[0][1]
    a_mat = trace[0][3][1][0]
    mm = P.scored(a_mat, *av[(0, 1)], np.arange(m))
    drop = (FD_SEED, 1, FD_RATES[0], 0)
    o, lse, z, ck = P.fwd_pass(rows, cols, m, mm, mm, f, T.GAT_ALPHA, drop)
    assert np.array_equal(ck, trace[0][3][1][5]) and 0 < np.count_nonzero(ck) < len(ck)
    assert T.rel(o, trace[0][3][1][3]) <= T.TOL and T.rel(lse, trace[0][3][1][4]) <= T.TOL
    o_ld, lse_ld = P.fwd_pass_ld(rows, cols, m, mm, mm, f, T.GAT_ALPHA, drop)
    assert o_ld.dtype == np.longdouble and T.rel(np.float64(o_ld), o) <= 1e-13 and T.rel(np.float64(lse_ld), lse) <= 1e-13
    # a block whose rows start at global row 100 and whose gathered rows are relabelled: the ids in the operand decide, not the positions
    perm = np.random.default_rng(0).permutation(m)
    inv = np.argsort(perm)
    o2, _, _, ck2 = P.fwd_pass(rows, inv[cols], m, mm, mm[perm], f, T.GAT_ALPHA, drop)
    assert np.array_equal(ck2, ck) and T.rel(o2, o) <= T.TOL


def test_rates_zero_call_through_to_the_additive_reference():
    """Rates (0, 0), spelled out or left out, with any seed: the recorded results of the additive reference that tests/gat_ref.py replaced
    (output, every dW, da1, da2 and dX)."""
    rows, cols, m, x, w, av, g = fd_problem()
    for kw in ({}, dict(rates=(0.0, 0.0), seed=77)):
        out = R.forward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, w, av, **kw, **MODE)
        assert pinned_error("softmax_additive", out, *R.backward(rows, cols, m, x, T.GAT_LAYERS, T.GAT_ALPHA, g, w, av, **kw, **MODE)) <= 1e-13


@pytest.mark.parametrize("f", [1, 2, 7, 8, 33])
def test_operand_layouts(f):
    """[A (0) | s t | id 0] and [dZ (0) | s lse delta id]: widths, pads and the last slot of M' hold zero, ids are exact."""
    rng = np.random.default_rng(f)
    a, dz = rng.uniform(-1, 1, (5, f)), rng.uniform(-1, 1, (5, f))
    a1, a2 = rng.uniform(-1, 1, f), rng.uniform(-1, 1, f)
    lse, delta = rng.uniform(0, 1, 5), rng.uniform(-1, 1, 5)
    ids = np.array([0, 1, (1 << 31) + 5, (1 << 32) - 1, 12345])
    fp = f + (f & 1)
    assert P.scored_width(f, ids=True) == K.attn_drop_scored_width(f) == fp + 4 == K.attn_add_packed_width(f)
    mm = P.scored(a, a1, a2, ids, ld=fp + 6)
    assert np.array_equal(mm[:, :fp + 2], P.scored(a, a1, a2)) and np.array_equal(mm[:, fp + 2].astype(np.uint64), ids.astype(np.uint64))
    assert np.all(mm[:, fp + 3] == 0.0) and np.all(np.isnan(mm[:, fp + 4:]))
    q = P.pack(dz, mm[:, fp], lse, delta, ids, ld=fp + 6)
    assert np.array_equal(q[:, :fp + 3], P.pack(dz, mm[:, fp], lse, delta)[:, :fp + 3])
    assert np.array_equal(q[:, fp + 3].astype(np.uint64), ids.astype(np.uint64)) and np.all(np.isnan(q[:, fp + 4:]))
    if f & 1:
        assert np.all(mm[:, f] == 0.0) and np.all(q[:, f] == 0.0)
    txt = open(ROOT + "/include/hnh_attn_dropout.h").read()
    assert re.search(r"#define HNH_ATTN_DROP_SCORED_WIDTH\(f\) \(\(f\) \+ \(\(f\) & 1\) \+ 4\)", txt)
    assert "same mask" in txt and "repeated" in txt, "the header says what happens to a repeated pair"


def test_dropout_kernels_are_an_optional_group():
    names = declared("hnh_attn_dropout.h")
    assert names == GROUP
    assert names == set(K.ATTN_DROP_SIGNATURES), names ^ set(K.ATTN_DROP_SIGNATURES)
    for header in ("hnh_kernels.h", "hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_attn_additive.h"):
        assert not names & declared(header), header
    for table in (K.SIGNATURES, K.GRAD_SIGNATURES, K.ATTN_SIGNATURES, K.ATTN_GRAD_SIGNATURES, K.ATTN_ADD_SIGNATURES):
        assert not names & set(table), "disjoint from the five existing tables"
    lib = K.load()  # the HIP library: dlopen needs no GPU
    for n in names:
        assert getattr(lib, n).argtypes == K.ATTN_DROP_SIGNATURES[n][1]
    dbl = C.CDLL(T.ORACLE_BACKEND)
    for n in names:
        assert not hasattr(dbl, n), "the CPU test double does not export %s" % n
    K.load(T.ORACLE_BACKEND)  # ... and binding it still works
    assert C.sizeof(K.AttnDrop) == 32 and C.sizeof(K.AttnAdd) == 144


def test_host_calls_declared_and_exported():
    for n in ("hnh_gat_set_dropout", "hnh_gat_set_dropout_seed", "hnh_dropout_word"):
        assert n in declared("hnh_dist.h") and n in H.SIGNATURES and hasattr(H.lib(), n), n


def test_dropout_on_the_test_double():
    H.load_backend(T.ORACLE_BACKEND)
    case = T.case_inputs("er8_r16")

    def rank(world):
        sp, d, gnn = make_gat(world, case, "15d_fusion2", 1, attention="softmax", score="additive", dropout=(0.6, 0.6), seed=3)
        g = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        for call in (gnn.forwardPass, lambda: gnn.backwardPass(g)):
            with pytest.raises(H.HnhError, match=r"dropout.*(hnh_attn_drop_[a-z0-9_]+|hnh_feat_drop_f64).*include/hnh_attn_dropout\.h") as e:
                call()
            assert re.search(r"hnh_(attn|feat)_drop_[a-z0-9_]+", str(e.value)).group(0) in GROUP
        gnn.set_dropout(0.0, 0.3, 3)  # feature dropout alone names its kernel
        with pytest.raises(H.HnhError, match=r"hnh_feat_drop_f64.*include/hnh_attn_dropout\.h"):
            gnn.forwardPass()
        gnn.set_score("dot")
        gnn.set_dropout(0.6, 0.0, 3)
        with pytest.raises(H.HnhError, match=r"attention dropout.*score additive only.*score dot"):
            gnn.forwardPass()
        for bad in (-0.1, 1.0, 1.5, float("nan")):
            with pytest.raises(ValueError):
                gnn.set_dropout(bad, 0.0, 1)
            with pytest.raises(ValueError):
                gnn.set_dropout(0.0, bad, 1)
            assert H.lib().hnh_gat_set_dropout(gnn.h, bad, 0.0, 1) != 0 and H.lib().hnh_gat_set_dropout(gnn.h, 0.0, bad, 1) != 0
        gnn.set_dropout(0.0, 0.0, 99)  # the process and the operator live on: the plain GAT on the same object
        gnn.set_attention("none")
        gnn.forwardPass()
        out = H.Dense.create(world, *gnn.buffer_shape(len(T.GAT_LAYERS)))
        gnn.get_output(out)
        res = out.download()
        for h in (out, g, gnn, d, sp):
            h.free()
        return res

    per_rank, want = H.run_spmd(2, rank), H.run_spmd(2, lambda world: plain_output(world, case))
    assert all(np.isfinite(r).all() for r in per_rank) and all(np.array_equal(a, b) for a, b in zip(per_rank, want))
