"""CPU-only: the HIP C-ABI library loads here (no GPU needed to dlopen it) and exports every symbol that
include/hnh_kernels.h declares; creating a context without a GPU fails loudly instead of falling back."""
import os
import re

import pytest

from distributed_sddmm_amd import _kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(hnh_[a-z0-9_]+)\s*\(", txt))


def test_kernel_library_exports_every_declared_symbol():
    lib = K.load()
    declared = declared_symbols("hnh_kernels.h")
    assert declared, "no declarations parsed"
    assert declared == set(K.SIGNATURES), (declared ^ set(K.SIGNATURES))
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.hnh_backend_name() == b"hip-gfx950"


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(K.HnhError):
        K.Ctx(0)


FORMER_ATTN_MEMBERS = [  # KernelImplementation::attn_*_local as the headers declared them before hnh::AttnPass (csrc/host/attn_compat.cpp)
    "_ZN20KernelImplementation15attn_grad_localER10SpmatLocaliRK13hnh_attn_gradbjl",
    "_ZN20KernelImplementation19attn_additive_localER10SpmatLocaliRK12hnh_attn_addijlb",
    "_ZN20KernelImplementation19attn_additive_localER10SpmatLocaliRK12hnh_attn_addijlbPK13hnh_attn_drop",
    "_ZN20KernelImplementation13attn_v2_localER10SpmatLocaliRK11hnh_attn_v2ijlb",
    "_ZN20KernelImplementation14attn_qkv_localER10SpmatLocaliRK12hnh_attn_qkvijlb",
    "_ZN20KernelImplementation14attn_qkv_localER10SpmatLocaliRK12hnh_attn_qkvijlbPKd",
    "_ZN20KernelImplementation14attn_qkv_localER10SpmatLocaliRK12hnh_attn_qkvijlbPKdPdb",
    "_ZN20KernelImplementation15attn_coef_localER10SpmatLocaliRK13hnh_attn_coeflPK13hnh_attn_drop",
]


@pytest.mark.parametrize("symbol", FORMER_ATTN_MEMBERS)
def test_host_library_keeps_the_former_attention_members_for_drivers_built_earlier(symbol):
    """A driver compiled against the earlier headers calls these from its own inline schedule code: the library must still resolve them."""
    from distributed_sddmm_amd import api as H
    assert getattr(H.lib(), symbol) is not None
