// Host side of the attention entry points (fino_attention.hip, fino_attention_fp8.hip): ONE copy of the operand checks, of
// the AttnParams filling, of the tile-mask / ranges-table checks, of the shape rule behind the *_supported() predicates, of the
// launch setup for kernels that never split a block, and of the dtype x head_dim dispatch.  An entry point's message starts with
// its own name (`fn`); the text behind it and the order in which a call with several faults reports them are the ABI's
// (tests/test_attention_abi_cpu.py).
#pragma once
#include <type_traits>

#include "fino_attention_common.h"

namespace fino_attn_ns {

// what every forward entry point receives, in the order of its C signature (the fp8 ones have no head strides: q_hs = o_hs =
// head_dim, k_hs = v_hs = 0)
struct AttnOperands {
    const void *q, *k, *v;
    void* o;
    int batch, heads;
    int64_t lq, lk;
    int head_dim;
    int64_t q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, v_bs, v_rs, v_hs, o_bs, o_rs, o_hs;
    float scale;
};

// The checks every entry point makes on its operands, in the order all of them report: null pointers, the entry point's own
// shape rule (`shape_rule()`: FINO_OK, or the code of the error it has set), 16-byte alignment of pointers and strides, scale.
// `others`: the entry point's further pointers are there; `aligned`: one more pointer that has to be 16-byte aligned, or nullptr.
template <class ShapeRule>
inline int attn_check_operands(const char* fn, const AttnOperands& a, bool others, const void* aligned, const char* scale_what,
                               ShapeRule&& shape_rule) {
    FINO_CHECK(a.q && a.k && a.v && a.o && others, FINO_ERR_ARG, "%s: null pointer", fn);
    if (int rc = shape_rule()) return rc;
    FINO_CHECK(fino_aligned16(a.q) && fino_aligned16(a.k) && fino_aligned16(a.v) && fino_aligned16(a.o) && fino_aligned16(aligned) &&
                   a.q_rs % 8 == 0 && a.k_rs % 8 == 0 && a.v_rs % 8 == 0 && a.o_rs % 8 == 0 && a.q_hs % 8 == 0 && a.k_hs % 8 == 0 &&
                   a.v_hs % 8 == 0 && a.o_hs % 8 == 0 && a.q_bs % 8 == 0 && a.k_bs % 8 == 0 && a.v_bs % 8 == 0 && a.o_bs % 8 == 0,
               FINO_ERR_ARG, "%s: pointers and strides must be 16-byte aligned", fn);
    FINO_CHECK(a.scale > 0.f || a.scale == FINO_ATTN_SCALE_FOLDED, FINO_ERR_ARG, "%s: %s", fn, scale_what);
    return FINO_OK;
}

// operands, strides, scale_log2 and q-blocks of `q_block` rows; everything optional off (ws, all_partial, tail_n, ranges, vmean),
// one virtual head per head and no tail split until attn_whole_blocks or the launch policy say otherwise
inline void attn_fill_params(AttnParams& p, const AttnOperands& a, int q_block = kQBlock) {
    p = AttnParams{};
    p.q = (const uint16_t*)a.q; p.k = (const uint16_t*)a.k; p.v = (const uint16_t*)a.v; p.o = (uint16_t*)a.o;
    p.batch = a.batch; p.heads = a.heads; p.lq = (int)a.lq; p.lk = (int)a.lk;
    p.q_bs = a.q_bs; p.q_rs = a.q_rs; p.q_hs = a.q_hs; p.k_bs = a.k_bs; p.k_rs = a.k_rs; p.k_hs = a.k_hs;
    p.v_bs = a.v_bs; p.v_rs = a.v_rs; p.v_hs = a.v_hs; p.o_bs = a.o_bs; p.o_rs = a.o_rs; p.o_hs = a.o_hs;
    p.scale_log2 = a.scale == FINO_ATTN_SCALE_FOLDED ? 1.0f : a.scale * 1.4426950408889634f;
    p.nqb = (int)((a.lq + q_block - 1) / q_block);
    p.vsplit = 1; p.nqb_v = p.nqb; p.per = 1;
}

// the device mask of fino_attn_fwd_tiles / fino_attn_fwd_fp8_tiles
inline int attn_check_tile_mask(const char* fn, const uint32_t* mask, int64_t mask_bs, int64_t mask_hs, int words, int64_t lk) {
    FINO_CHECK(mask, FINO_ERR_ARG, "%s: null mask", fn);
    FINO_CHECK(((uintptr_t)mask & 3) == 0, FINO_ERR_ARG, "%s: the mask must be 4-byte aligned", fn);
    FINO_CHECK(lk > 0 && (lk + kKV - 1) / kKV <= kAttnMaxTiles, FINO_ERR_UNSUPPORTED, "%s: Lk=%lld is more than %d key tiles", fn,
               (long long)lk, kAttnMaxTiles);
    FINO_CHECK(words > 0 && (int64_t)words * 32 >= (lk + kKV - 1) / kKV, FINO_ERR_ARG,
               "%s: %d mask words per q-block do not hold %lld key tiles", fn, words, (long long)((lk + kKV - 1) / kKV));
    FINO_CHECK(mask_bs >= 0 && mask_hs >= 0, FINO_ERR_ARG, "%s: negative mask stride", fn);
    return FINO_OK;
}

// the device table of fino_attn_fwd_ranges / fino_attn_fwd_fp8_ranges
inline int attn_check_ranges(const char* fn, const int* ranges) {
    FINO_CHECK(ranges, FINO_ERR_ARG, "%s: null ranges table", fn);
    FINO_CHECK(((uintptr_t)ranges & 3) == 0, FINO_ERR_ARG, "%s: the ranges table must be 4-byte aligned", fn);
    return FINO_OK;
}

// the rule behind the *_supported() predicates: a non-empty problem whose sequences fit the kernels' 32-bit row arithmetic, a
// head_dim out of `head_dims` (64 | 128, or one of them), and, where a tile mask names the key tiles, at most kAttnMaxTiles
inline bool attn_shape_supported(int batch, int heads, int64_t lq, int64_t lk, int head_dim, int head_dims, bool tile_mask) {
    return (head_dim == 64 || head_dim == 128) && (head_dim & head_dims) && batch > 0 && heads > 0 && lq > 0 && lk > 0 &&
           lq < (1ll << 31) - 256 && lk < (1ll << 31) - 64 && (!tile_mask || (lk + kKV - 1) / kKV <= kAttnMaxTiles);
}

// launch setup of the kernels that run whole blocks only: virtual heads, every block in the whole-block part of the grid, no
// tail split.  Returns the grid.  (ws and all_partial are the caller's.)
inline unsigned attn_whole_blocks(AttnParams& p) {
    attn_virtual_heads(p.batch, p.heads, p.nqb, p.vsplit, p.nqb_v);
    const int groups = (p.batch * p.heads * p.vsplit + 7) / 8;
    p.full_x = groups * p.nqb_v; p.rem_x = 0; p.nwg = 0; p.per = 1;
    return (unsigned)(8 * p.full_x);
}

// bytes that ONE buffer resource over a whole operand spans (the walking kernel's addressing; its look-ahead reaches two key
// tiles past the last row), and whether K, V and O each stay below the 2 GiB such a resource can address
inline int64_t attn_span(int batch, int heads, int64_t bs, int64_t hs, int64_t rs, int64_t rows) {
    return (((int64_t)batch - 1) * bs + ((int64_t)heads - 1) * hs + (rows - 1 + 2 * kKV) * rs + 128) * 2;
}
template <class P>                               // AttnOperands or AttnParams: the members go by the same names
inline bool attn_spans_fit(const P& p) {
    return attn_span(p.batch, p.heads, p.k_bs, p.k_hs, p.k_rs, p.lk) < (1ll << 31) &&
           attn_span(p.batch, p.heads, p.v_bs, p.v_hs, p.v_rs, p.lk) < (1ll << 31) &&
           attn_span(p.batch, p.heads, p.o_bs, p.o_hs, p.o_rs, p.lq) < (1ll << 31);
}

// f(T{}, AttnDim<D>{}) for the (BF16 | F16) x (128 | 64) the caller has checked dtype and head_dim to be.  The compiler emits
// the kernels that f launches in the order of the four calls below.
template <int D> using AttnDim = std::integral_constant<int, D>;
template <class F>
inline auto attn_dispatch(int dtype, int head_dim, F&& f) {
    if (dtype == FINO_BF16) return head_dim == 128 ? f(BF16{}, AttnDim<128>{}) : f(BF16{}, AttnDim<64>{});
    return head_dim == 128 ? f(F16{}, AttnDim<128>{}) : f(F16{}, AttnDim<64>{});
}

}  // namespace fino_attn_ns
