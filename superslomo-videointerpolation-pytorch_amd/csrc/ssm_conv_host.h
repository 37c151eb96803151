// The host half that the fp32 convolution entry points share (ssm_conv.hip, ssm_wino.hip, ssm_wino4.hip, ssm_wino1d.hip, ssm_wino5.hip,
// ssm_wino7.hip; ssm_upgemm.hip where it fits): the forced tile configuration, the checks of a padded-plane source, the binding of the output /
// pooled / addend views into a kernel's params struct with the `vec` decision, and the launch tail.  Host code only, allocation-free and inline
// (inference issues ~60 of these calls per frame pair).  `who` is the prefix of every message ("wino5 conv"): the texts are part of the C ABI's
// behaviour (tests/test_conv_entry_refusals_cpu.py holds them), and so is the ORDER of the checks - the first failing one decides the message -
// which is why the pieces are separate functions that an entry point calls in its own order.
//
// A new convolution form supplies: a params struct with the shared member names (dst,dsb,dsc,dsh, pool,psb,psc,psh, add,asb,asc,ash,adiv,
// slope,lrelu, H,W,Cout; `vec` if its epilogue has a vector path), an OutRules value, its X-macro kind table, and the kernel.
#pragma once
#include "ssm_common.h"

namespace ssm {

// early return of a helper's refusal
#define SSM_TRY(expr)                        \
    do {                                     \
        const int ssm_try_rc_ = (expr);      \
        if (ssm_try_rc_ != SSM_OK) return ssm_try_rc_; \
    } while (0)

// ---- forced tile configuration (tests / tuning only: the *_force_kind entry points) ----------------------------------------------------
struct ForcedKind {
    std::atomic<int> kind{-1};
    int get(int nkinds) const {          // the forced kind, or -1 = automatic
        const int k = kind.load();
        return k >= 0 && k < nkinds ? k : -1;
    }
    int set(int k, int nkinds) {          // out of range = automatic; returns the number of kinds
        kind.store(k >= 0 && k < nkinds ? k : -1);
        return nkinds;
    }
};

// ---- views ---------------------------------------------------------------------------------------------------------------------------
// may the view be moved as aligned pieces of m floats (m = 4: 16 bytes, 2: 8 bytes, 1: always)?
inline bool view_pieces(const ssm_view &v, int m) {
    return (reinterpret_cast<size_t>(v.ptr) & ((size_t)m * 4 - 1)) == 0 && v.sh % m == 0 && v.sc % m == 0 && v.sb % m == 0;
}

// A padded-plane source (LDS-DMA moves it as 16-byte pieces) whose rows keep a zero frame around a map `srcW` wide (W, or W / 2 for the
// fused-upsample forms), and the packed filter.  cat: the form takes two concatenated sources, its messages say "input 1".
inline int check_source(const char *who, bool cat, const ssm_view &x, int srcW, const float *w_packed) {
    SSM_REQUIRE(view_pieces(x, 4), "%s: %s is not a padded-plane view (16-byte alignment)", who, cat ? "input 1" : "the input");
    SSM_REQUIRE(x.sh >= srcW + 2 * SSM_PADX, "%s: %s row stride %d leaves no zero frame for W=%d", who, cat ? "input 1" : "input", x.sh, srcW);
    SSM_REQUIRE(aligned16(w_packed), "%s: packed filter must be 16-byte aligned", who);
    return SSM_OK;
}

// the optional second source of a concatenated input: the kernels walk both with the row / channel strides of the first
inline int check_source2(const char *who, const ssm_view &x1, const ssm_view &x2, int C2) {
    if (C2 <= 0) return SSM_OK;
    SSM_REQUIRE(x2.ptr && aligned16(x2.ptr) && x2.sb % 4 == 0, "%s: input 2 is not a padded-plane view", who);
    SSM_REQUIRE(x2.sh == x1.sh && x2.sc == x1.sc, "%s: cat sources must share row/channel strides", who);
    return SSM_OK;
}

// ---- output side ----------------------------------------------------------------------------------------------------------------------
// What differs between the forms, one value per form next to its kernel:
//   mask     SSM_FLAG_MASK is decoded into bit 1 of `lrelu` (the addend is a mask source).  F(2x2), F(4x4) and wino5 do; wino7, wino1d and
//            the direct kernel have no mask path and DROP the flag silently - an oddity kept as it is (refusing it would change behaviour).
//   piece    floats per vector piece of the epilogue: dst / addend move as `piece`, pooled outputs as `piece / 2` floats; 0 = scalar stores
//            only, no alignment rule (the direct kernel)
//   required false: `vec` is COMPUTED - the params struct has a `vec` member and the kernel an element-wise path for views that do not
//            qualify; true: the alignment is REQUIRED of output and addend (F(2x2): row pairs of 2x2 pixel blocks) and a view without it
//            is refused
struct OutRules {
    bool mask;
    int piece;
    bool required;
};

// F(2x2)'s requirement on its output view; the entry points check it before the second source (bind_outputs is too late for the order)
inline int check_output_pairs(const char *who, const ssm_view &y) {
    SSM_REQUIRE(view_pieces(y, 2), "%s: output view must be 8-byte aligned (2x2 pixel blocks are stored as row pairs)", who);
    return SSM_OK;
}

template <class P>
inline int bind_pool(const char *who, P &p, const ssm_view &pool) {
    p.pool = nullptr;
    p.psb = p.psc = 0;
    p.psh = 0;
    if (!pool.ptr) return SSM_OK;
    SSM_REQUIRE(p.H % 2 == 0 && p.W % 2 == 0, "%s: fused pool needs even H, W", who);
    p.pool = pool.ptr;
    p.psb = pool.sb;
    p.psc = pool.sc;
    p.psh = pool.sh;
    return SSM_OK;
}

template <class P, class = void>
struct has_vec : std::false_type {};
template <class P>
struct has_vec<P, std::void_t<decltype(std::declval<P &>().vec)>> : std::true_type {};

// Fills dst / pool / add (and H, W, Cout, slope, lrelu) of a params struct from the views; checks the addend's batch divisor, then the fused
// pool's even H, W; decides `vec`.
template <class P>
inline int bind_outputs(const char *who, const OutRules &r, P &p, const ssm_view &y, const ssm_view &pool, const ssm_view &add, int add_div, int B,
                        int H, int W, int Cout, float slope, int flags) {
    p.dst = y.ptr;
    p.dsb = y.sb;
    p.dsc = y.sc;
    p.dsh = y.sh;
    p.H = H;
    p.W = W;
    p.Cout = Cout;
    p.slope = slope;
    p.lrelu = ((flags & SSM_FLAG_LRELU) ? 1 : 0) | ((r.mask && (flags & SSM_FLAG_MASK)) ? 2 : 0);
    p.add = nullptr;
    p.asb = p.asc = 0;
    p.ash = 0;
    p.adiv = 1;
    bool vec = !r.required && r.piece > 0 && W % r.piece == 0 && view_pieces(y, r.piece);
    if (add.ptr) {
        SSM_REQUIRE(add_div >= 1 && B % add_div == 0, "%s: the addend serves %d batch entries each, batch %d is no multiple", who, add_div, B);
        if (r.required) SSM_REQUIRE(view_pieces(add, r.piece), "%s: the addend view must be 8-byte aligned (read as row pairs)", who);
        p.add = add.ptr;
        p.asb = add.sb;
        p.asc = add.sc;
        p.ash = add.sh;
        p.adiv = add_div;
        vec = vec && view_pieces(add, r.piece);
    }
    SSM_TRY(bind_pool(who, p, pool));
    if (pool.ptr) vec = vec && view_pieces(pool, r.piece / 2);
    if constexpr (has_vec<P>::value) p.vec = vec ? 1 : 0;
    return SSM_OK;
}

// ---- launch tail ----------------------------------------------------------------------------------------------------------------------
inline int check_grid(const char *who, long long blocks) {
    SSM_REQUIRE(blocks > 0 && blocks <= 0x7fffffffLL, "%s: grid of %lld workgroups out of range", who, blocks);
    return SSM_OK;
}

// One-dimensional grid of `blocks` workgroup tiles of a kernel that asks for more dynamic LDS than the default limit: the grid range, the per
// (kernel, device) opt-in (reserve_lds; its guard is this template's static - one per kernel), the launch and its error check.
template <auto Kern, class P>
inline int launch_tiles(const char *who, const char *entry, long long blocks, int threads, int lds_bytes, hipStream_t st, const P &p) {
    SSM_TRY(check_grid(who, blocks));
    static std::atomic<uint64_t> lds_reserved{0};          // one bit per device: the attribute is per (kernel, device)
    const hipError_t attr_rc = reserve_lds(lds_reserved, (const void *)Kern, lds_bytes);
    if (attr_rc != hipSuccess) {
        set_error("%s: cannot reserve %d bytes of LDS: %s", who, lds_bytes, hipGetErrorString(attr_rc));
        return SSM_E_LAUNCH;
    }
    SSM_LAUNCH(Kern, dim3((unsigned)blocks), dim3(threads), lds_bytes, st, p);
    return check_launch(entry);
}

}  // namespace ssm
