// Binary compatibility, not API: the eight KernelImplementation::attn_*_local members that sparse_kernels.hpp declared before
// hnh::AttnPass.  The headers no longer have them, but a driver COMPILED against the earlier headers carries the inline schedule code of
// that time (Sparse15D_Dense_Shift::attnQKV_pass and its siblings), which calls them in libhnh_host.so: without these symbols such a
// driver no longer loads (oracle/_ref/mains are such drivers when they were built before this library).  Each symbol is a free function
// under the member's mangled name — on the Itanium C++ ABI a non-static member function is a function whose first argument is `this` —
// that builds the descriptor and calls attn_local.  The names are the PARENT's and therefore frozen: they do not follow later changes of
// the classes, and tests/test_abi_symbols.py pins them.  Delete this file when drivers built before hnh::AttnPass need not load any more.
#include "sparse_kernels.hpp"

namespace {
template <typename Args>
hnh::AttnPass descriptor(int pass, const Args& args, const hnh_attn_drop* drop = nullptr) {
    hnh::AttnPass p;
    p.pass = pass;
    p.args = args;
    p.drop = drop;
    return p;
}

// (the earlier schedule has lent the block the very slices it hands over, so they are not passed on: the descriptor's vectors are never
// read below the schedule and only say which entry point)
bool qkv(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish, bool biased,
         bool graded, bool accumulate) {
    static hnh::VectorXd lent;
    hnh::AttnPass p = descriptor(pass, args);
    p.bias = biased ? &lent : nullptr;
    p.dbias = graded ? &lent : nullptr;
    p.accumulate = accumulate;
    return self->attn_local(S, block, p, flags, rows, finish);
}
}  // namespace

#define HNH_FORMER_MEMBER(name, mangled, ...) bool name(KernelImplementation* self, SpmatLocal& S, int block, __VA_ARGS__) __asm__(mangled)

HNH_FORMER_MEMBER(former_grad, "_ZN20KernelImplementation15attn_grad_localER10SpmatLocaliRK13hnh_attn_gradbjl", const hnh_attn_grad& args, bool column_side,
                  unsigned flags, int64_t rows);
bool former_grad(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_grad& args, bool column_side, unsigned flags, int64_t rows) {
    return self->attn_local(S, block, descriptor(column_side ? 2 : 1, args), flags, rows, false);
}

HNH_FORMER_MEMBER(former_additive, "_ZN20KernelImplementation19attn_additive_localER10SpmatLocaliRK12hnh_attn_addijlb", const hnh_attn_add& args, int pass,
                  unsigned flags, int64_t rows, bool finish);
bool former_additive(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish) {
    return self->attn_local(S, block, descriptor(pass, args), flags, rows, finish);
}

HNH_FORMER_MEMBER(former_additive_drop, "_ZN20KernelImplementation19attn_additive_localER10SpmatLocaliRK12hnh_attn_addijlbPK13hnh_attn_drop",
                  const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish, const hnh_attn_drop* drop);
bool former_additive_drop(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_add& args, int pass, unsigned flags, int64_t rows, bool finish,
                          const hnh_attn_drop* drop) {
    return self->attn_local(S, block, descriptor(pass, args, drop), flags, rows, finish);
}

HNH_FORMER_MEMBER(former_v2, "_ZN20KernelImplementation13attn_v2_localER10SpmatLocaliRK11hnh_attn_v2ijlb", const hnh_attn_v2& args, int pass, unsigned flags,
                  int64_t rows, bool finish);
bool former_v2(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_v2& args, int pass, unsigned flags, int64_t rows, bool finish) {
    return self->attn_local(S, block, descriptor(pass, args), flags, rows, finish);
}

HNH_FORMER_MEMBER(former_qkv, "_ZN20KernelImplementation14attn_qkv_localER10SpmatLocaliRK12hnh_attn_qkvijlb", const hnh_attn_qkv& args, int pass, unsigned flags,
                  int64_t rows, bool finish);
bool former_qkv(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish) {
    return qkv(self, S, block, args, pass, flags, rows, finish, false, false, false);
}

HNH_FORMER_MEMBER(former_qkv_bias, "_ZN20KernelImplementation14attn_qkv_localER10SpmatLocaliRK12hnh_attn_qkvijlbPKd", const hnh_attn_qkv& args, int pass,
                  unsigned flags, int64_t rows, bool finish, const double* bias);
bool former_qkv_bias(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                     const double* bias) {
    return qkv(self, S, block, args, pass, flags, rows, finish, true, false, false);
}

HNH_FORMER_MEMBER(former_qkv_bias_grad, "_ZN20KernelImplementation14attn_qkv_localER10SpmatLocaliRK12hnh_attn_qkvijlbPKdPdb", const hnh_attn_qkv& args, int pass,
                  unsigned flags, int64_t rows, bool finish, const double* bias, double* dbias, bool accumulate);
bool former_qkv_bias_grad(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_qkv& args, int pass, unsigned flags, int64_t rows, bool finish,
                          const double* bias, double* dbias, bool accumulate) {
    return qkv(self, S, block, args, pass, flags, rows, finish, true, true, accumulate);
}

HNH_FORMER_MEMBER(former_coef, "_ZN20KernelImplementation15attn_coef_localER10SpmatLocaliRK13hnh_attn_coeflPK13hnh_attn_drop", const hnh_attn_coef& args,
                  int64_t rows, const hnh_attn_drop* drop);
bool former_coef(KernelImplementation* self, SpmatLocal& S, int block, const hnh_attn_coef& args, int64_t rows, const hnh_attn_drop* drop) {
    return self->attn_local(S, block, descriptor(0, args, drop), 0u, rows, false);
}
