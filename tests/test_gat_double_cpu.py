"""The second CPU test double (oracle/liboracle_backend_gat.so: oracle/hnh_oracle_gat_groups.h behind -DHNH_ORACLE_GAT_GROUPS) at kernel
level: the case list of tests/gat_double_cases.py on plain C restatements of include/hnh_grad.h, hnh_attention.h, hnh_attn_grad.h and
hnh_train.h, under the stream-order checker (oracle/hnh_stream_order.h).  Every operand is a block of hnh_malloc, so a declaration that
runs past the end of its block, or a host pointer among the operands, is a MISUSE report; after each case the report must be empty.
tests/test_gat_double_gpu.py runs the same list on the HIP library."""
import ctypes as C

import pytest

import gat_cpu_harness as CH
import gat_double_cases as D
import hnh_testlib as T
from distributed_sddmm_amd import _kernels as K


@pytest.fixture(scope="module")
def double():
    lib = D.bind(T.ORACLE_GAT_BACKEND)
    assert lib.hnh_backend_name() == b"oracle-cpu-test-double-gat"
    lib.hnh_oracle_order_report.restype = C.c_long
    lib.hnh_oracle_order_accesses.restype = C.c_long
    lib.hnh_oracle_order_enable(1)
    ctx = D.Api(lib)
    yield lib, ctx
    ctx.close()


def drain(lib):
    buf = C.create_string_buffer(16384)
    return lib.hnh_oracle_order_report(buf, 16384), buf.value.decode()


@pytest.mark.parametrize("name,case", D.CASES, ids=D.IDS)
def test_case_on_the_double(double, name, case):
    lib, ctx = double
    assert drain(lib) == (0, ""), "reports left behind by an earlier test"
    before = lib.hnh_oracle_order_accesses()
    case(lib, ctx)
    assert drain(lib) == (0, ""), "no race and no MISUSE"
    assert lib.hnh_oracle_order_accesses() > before, "the case was watched"


def test_the_two_doubles_differ_by_the_four_groups_only():
    """liboracle_backend.so stays the mandatory table; the second one adds exactly the entry points of the four headers."""
    names = set()
    for header in ("hnh_grad.h", "hnh_attention.h", "hnh_attn_grad.h", "hnh_train.h"):
        names |= CH.declared(header) - CH.declared("hnh_kernels.h")
    assert names == set(D.GROUP_SIGNATURES), names ^ set(D.GROUP_SIGNATURES)
    plain, gat = C.CDLL(T.ORACLE_BACKEND), C.CDLL(T.ORACLE_GAT_BACKEND)
    plain.hnh_backend_name.restype = gat.hnh_backend_name.restype = C.c_char_p
    assert plain.hnh_backend_name() == b"oracle-cpu-test-double" and gat.hnh_backend_name() == b"oracle-cpu-test-double-gat"
    for n in names:
        assert hasattr(gat, n) and not hasattr(plain, n), n
    later = set()
    for sigs in (K.ATTN_ADD_SIGNATURES, K.ATTN_DROP_SIGNATURES, K.V2_SIGNATURES, K.ATTN_COEF_SIGNATURES, K.SKIP_SIGNATURES, K.QKV_SIGNATURES,
                 K.EDGE_SIGNATURES, K.EDGE_GRAD_SIGNATURES, K.NORM_SIGNATURES, K.MULTILABEL_SIGNATURES):
        later |= set(sigs)
    assert not [n for n in later if hasattr(gat, n)], "the remaining optional groups are in neither double"
    for n in K.SIGNATURES:
        assert hasattr(gat, n) and hasattr(plain, n), n


def test_workspace_sizes_are_the_hip_library_s():
    """The host sizes its buffers by the _workspace functions: the double returns what the HIP library returns (dlopen needs no GPU)."""
    hip, gat = K.load(), D.bind(T.ORACLE_GAT_BACKEND)
    for shape in list(D.GEMM_SHAPES) + [(1024, 1024, 1 << 18, 0), (64, 64, 511, 0), (64, 64, 512, 0), (8, 300, 70000, 0), (129, 129, 100000, 0),
                                         (2048, 2048, 4096, 0), (1, 1, 1 << 20, 0), (0, 5, 5, 0), (5, 5, -1, 0)]:
        assert gat.hnh_gemm_tn_f64_workspace(*shape[:3]) == hip.hnh_gemm_tn_f64_workspace(*shape[:3]), shape
    for rows in (-1, 0, 1, 5, 4095, 4096, 4097, 1 << 20):
        assert gat.hnh_xent_rows_f64_workspace(rows) == hip.hnh_xent_rows_f64_workspace(rows), rows


def test_a_declaration_past_the_end_of_a_block_is_reported(double):
    """What only the checker sees: an operand whose block is one double short of (rows - 1) * pitch + width.  The call is reported
    and refused (on the host it would read or write the heap behind the block; on the GPU it faults)."""
    import numpy as np
    lib, ctx = double
    rows, f = 16, 6
    pw = K.attn_grad_packed_width(f, True)
    a, dz, lse, p = ctx.upload(np.ones(rows * f)), ctx.upload(np.ones((rows, f))), ctx.upload(np.ones(rows)), ctx.upload(np.zeros((rows, pw)))
    short = ctx.upload(np.ones(rows * f - 1))
    ctx.check(lib.hnh_attn_grad_pack_f64(ctx.h, p.ptr, pw, a.ptr, f, dz.ptr, f, lse.ptr, lse.ptr, rows, f, K.STREAM_COMPUTE), "pack")
    ctx.check(lib.hnh_attn_grad_pack_f64(ctx.h, p.ptr, pw, short.ptr, f, dz.ptr, f, lse.ptr, lse.ptr, rows - 1, f, K.STREAM_COMPUTE), "pack, one row less")
    assert drain(lib) == (0, "")
    before = p.get()
    assert lib.hnh_attn_grad_pack_f64(ctx.h, p.ptr, pw, short.ptr, f, dz.ptr, f, lse.ptr, lse.ptr, rows, f, K.STREAM_COMPUTE) == 1, "A one double short"
    assert b"hnh_attn_grad_pack_f64" in lib.hnh_last_error(ctx.h) and b"past the end" in lib.hnh_last_error(ctx.h)
    assert np.array_equal(p.get(), before), "reported and refused, not performed"
    n, text = drain(lib)
    assert n == 1 and "MISUSE hnh_attn_grad_pack_f64 (read of %d bytes" % (8 * rows * f) in text and "runs past the end of its block" in text, text
    for d in (a, dz, lse, p, short):
        d.free()
