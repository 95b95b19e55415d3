// Tile plan of the dynamic block-sparse self-attention: which 64-key tiles each (batch element, head,
// 256-row q-block) keeps, predicted from pooled q and k -- the bitmask fino_attn_fwd_tiles walks.  Two launches, everything on
// the device, no host read:
//
// pool:    qbar[b][h][i][:] = fp32 mean of q over rows [256 i, min(256 (i + 1), lq)),
//          kbar[b][h][t][:] = fp32 mean of k over the real keys of tile t (the ragged last tile: its lk - 64 (ntall - 1) keys).
//          One workgroup per (b, h, q-block or key tile): a lane adds its 16-byte column chunk over its rows in row order, the
//          row groups are added in index order through LDS.  One HBM-bound pass over q and k.
// select:  one workgroup per (b, h, i):  s_t = scale <qbar_i, kbar_t>  (FINO_ATTN_SCALE_FOLDED: s is in log2 units, exp2),
//          w_t = n_t exp(s_t - max s), p_t = w_t / sum w, n_t the real keys of tile t.  F = row i of `keep_ranges` (the table of
//          fino_attn_fwd_ranges, clipped the same way; NULL: empty), m_F = sum_{t in F} p_t.  m_F >= cdf keeps F; otherwise F
//          and every t outside F with p_t >= theta, theta the largest p with m_F + sum_{t not in F, p_t >= theta} p_t >= cdf
//          (none: everything).  Ties at theta are all kept.  theta is found by bisection on the fp32 bit patterns of p (p >= 0:
//          the patterns order as the values do), 31 steps, each one masked sum.
// Deterministic: no atomics, every sum in a fixed order (a thread's tiles in index order, xor butterfly across the wave, waves
// in index order), so two runs -- an eager step and a graph replay -- give the same mask bit for bit.
//
// The gated plan (fino_attn_tile_plan_gated) adds two safeguards, both opt-in, in second instantiations of
// the two kernels, which take a PlanGate as a second kernel argument (the ungated instantiations have the signature and, checked
// on their ISA, the instructions of before):
// similarity: the pool pass also sums the NORMALISED rows, u = (1 / n) sum_r x_r / |x_r| (a zero row adds 0), and stores
//          sim = |u|^2 -- the mean cosine over all ordered row pairs of the block, in [0, 1] -- behind qbar | kbar:
//          sim_q [batch * heads][nqb], then sim_k [batch * heads][ntall].  A row's squared norm is added across the D / 8
//          adjacent lanes that hold its chunks by an xor butterfly; the normalised sums go through LDS in row-group order, the
//          D squares through the waves in index order.
// gate:    theta = sim_threshold > 0.  U = {t : sim_k[t] < theta}.  sim_q[i] < theta keeps every tile.  Otherwise the tiles of U
//          are kept and take no part in the maximum or in sum w (p_t = 0), and the rule above runs over the other tiles with
//          the forced set F (m_F counts F \ U).  sum w = 0 (every tile in U) keeps U and F alone.
// per head: cdf = cdf_heads[h] when the table is given; a value >= 1 keeps every tile of that head, without the bisection.
#include "fino_attention_common.h"
#include "fino_common.h"

namespace {

using namespace fino_attn_ns;

constexpr int kPlanThreads = 256;
constexpr int kPlanPer = kAttnMaxTiles / kPlanThreads;       // tiles per thread of the select kernel: 4

struct PlanParams {
    const uint16_t* q;
    const uint16_t* k;
    int batch, heads, lq, lk, nqb, ntall;
    int64_t q_bs, q_rs, q_hs, k_bs, k_rs, k_hs;
    float scale;            // logits = scale * <qbar, kbar>; folded: 1
    int folded;             // exp2 instead of exp
    float cdf;
    const int* keep;        // [nqb][3][2] or NULL
    uint32_t* mask;         // [batch][heads][nqb][words]
    int words;
    float* ws;              // qbar [batch * heads][nqb][D], then kbar [batch * heads][ntall][D]
};

// the second argument of the gated kernels
struct PlanGate {
    const float* cdf_heads; // [heads] or NULL
    float sim_thr;          // theta; <= 0: the gate is off
    float* sim;             // sim_q [batch * heads][nqb], then sim_k [batch * heads][ntall]: the workspace behind kbar
};

// the one gate argument of a gated instantiation
template <typename G>
__device__ __forceinline__ const G& plan_gate(const G& g) { return g; }

// blockIdx.x: q-blocks first, then key tiles; blockIdx.y: b * heads + h
// G... is empty (the ungated kernel: the signature and the code of before) or PlanGate: then also the similarity of the unit
template <typename T, int D, typename... G>
__global__ __launch_bounds__(kPlanThreads) void attn_plan_pool_kernel(const PlanParams p, const G... gate) {
    constexpr bool kSim = sizeof...(G) != 0;
    constexpr int kC = D / 8;                       // 16-byte chunks per row
    constexpr int kRows = kPlanThreads / kC;        // rows per pass: 16 (head_dim 128) / 32 (64)
    __shared__ float red[kRows][D];
    __shared__ float redn[kSim ? kRows : 1][kSim ? D : 1];
    __shared__ float redw[kPlanThreads / 64];
    const int tid = threadIdx.x;
    const int c = tid % kC, rg = tid / kC;
    const int hb = blockIdx.y;
    const int bi = hb / p.heads, head = hb - bi * p.heads;
    const int u = blockIdx.x;
    const bool is_q = u < p.nqb;
    const int unit = is_q ? u : u - p.nqb;
    const int span = is_q ? kQBlock : kKV;
    const int len = is_q ? p.lq : p.lk;
    const int64_t rs = is_q ? p.q_rs : p.k_rs;
    const uint16_t* base = is_q ? p.q + bi * p.q_bs + head * p.q_hs : p.k + bi * p.k_bs + head * p.k_hs;
    const int r0 = unit * span;
    const int r1 = r0 + span < len ? r0 + span : len;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    float nacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) nacc[j] = 0.f;
    for (int r = r0 + rg; r < r1; r += kRows) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + (int64_t)r * rs + 8 * c);
        float f[8];
        unpack8<T>(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f[j];
        if constexpr (kSim) {
            // the row's kC lanes are adjacent lanes of one wave and run the same trips of this loop
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) ss = fmaf(f[j], f[j], ss);
#pragma unroll
            for (int off = kC / 2; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
            const float inv = ss > 0.f ? 1.0f / sqrtf(ss) : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) nacc[j] = fmaf(f[j], inv, nacc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[rg][8 * c + j] = acc[j];
    if constexpr (kSim) {
#pragma unroll
        for (int j = 0; j < 8; ++j) redn[rg][8 * c + j] = nacc[j];
    }
    __syncthreads();
    float usq = 0.f;
    if (tid < D) {
        float s = red[0][tid];
#pragma unroll
        for (int gi = 1; gi < kRows; ++gi) s += red[gi][tid];
        float* out = is_q ? p.ws + ((int64_t)hb * p.nqb + unit) * D
                          : p.ws + (int64_t)p.batch * p.heads * p.nqb * D + ((int64_t)hb * p.ntall + unit) * D;
        out[tid] = s / (float)(r1 - r0);
        if constexpr (kSim) {
            float sn = redn[0][tid];
#pragma unroll
            for (int gi = 1; gi < kRows; ++gi) sn += redn[gi][tid];
            sn = sn / (float)(r1 - r0);
            usq = sn * sn;
        }
    }
    if constexpr (kSim) {
        usq = wave_sum(usq);
        if ((tid & 63) == 0) redw[tid >> 6] = usq;
        __syncthreads();
        if (tid == 0) {
            float* sim = plan_gate(gate...).sim;
            float* out = is_q ? sim + (int64_t)hb * p.nqb + unit
                              : sim + (int64_t)p.batch * p.heads * p.nqb + (int64_t)hb * p.ntall + unit;
            *out = ((redw[0] + redw[1]) + redw[2]) + redw[3];
        }
    }
}

// every thread gets the workgroup's sum; `red` is [2][4], `flip` alternates so one barrier per call is enough
__device__ __forceinline__ float plan_block_sum(float v, float (*red)[kPlanThreads / 64], int& flip) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[flip][threadIdx.x >> 6] = v;
    __syncthreads();
    float s = red[flip][0];
#pragma unroll
    for (int w = 1; w < kPlanThreads / 64; ++w) s += red[flip][w];
    flip ^= 1;
    return s;
}

// blockIdx.x: q-block i; blockIdx.y: b * heads + h.  Thread tid owns tiles tid + 256 j, j < 4.
// G... is empty (the ungated kernel: the signature and the code of before) or PlanGate: the per-head cdf and the similarity gate
template <int D, typename... G>
__global__ __launch_bounds__(kPlanThreads) void attn_plan_select_kernel(const PlanParams p, const G... gate) {
    constexpr bool kGated = sizeof...(G) != 0;
    __shared__ float qs[D];
    __shared__ float red[2][kPlanThreads / 64];
    __shared__ float redm[kPlanThreads / 64];
    const int tid = threadIdx.x;
    const int hb = blockIdx.y, i = blockIdx.x;
    const int ntall = p.ntall;
    float cdf = p.cdf;
    bool unpred[kPlanPer];
#pragma unroll
    for (int j = 0; j < kPlanPer; ++j) unpred[j] = false;
    bool full = false;
    if constexpr (kGated) {
        // both decisions below are the same for every thread of the workgroup
        const PlanGate& g = plan_gate(gate...);
        const bool gated = g.sim_thr > 0.f;
        if (g.cdf_heads) {
            cdf = g.cdf_heads[hb % p.heads];
            full = cdf >= 1.0f;
        }
        if (gated && g.sim[(int64_t)hb * p.nqb + i] < g.sim_thr) full = true;
        if (gated && !full) {
            const float* simk = g.sim + (int64_t)p.batch * p.heads * p.nqb + (int64_t)hb * ntall;
#pragma unroll
            for (int j = 0; j < kPlanPer; ++j) {
                const int t = tid + kPlanThreads * j;
                unpred[j] = t < ntall && simk[t] < g.sim_thr;
            }
        }
    }
    const float* qbar = p.ws + ((int64_t)hb * p.nqb + i) * D;
    const float* kbar = p.ws + (int64_t)p.batch * p.heads * p.nqb * D + (int64_t)hb * ntall * D;
    if (kGated && full) {                            // every tile, without the prediction
        uint32_t* mrow = p.mask + ((int64_t)hb * p.nqb + i) * p.words;
#pragma unroll
        for (int j = 0; j < kPlanPer; ++j) {
            const int t = tid + kPlanThreads * j;
            const unsigned long long bal = __ballot(t < ntall);
            const int w0 = (t & ~63) >> 5;
            if ((tid & 63) == 0) {
                if (w0 < p.words) mrow[w0] = (uint32_t)bal;
                if (w0 + 1 < p.words) mrow[w0 + 1] = (uint32_t)(bal >> 32);
            }
        }
        for (int w = 2 * kAttnMaxTiles / 64 + tid; w < p.words; w += kPlanThreads) mrow[w] = 0u;
        return;
    }
    if (tid < D) qs[tid] = qbar[tid];
    __syncthreads();

    float s[kPlanPer], pr[kPlanPer];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kPlanPer; ++j) {
        const int t = tid + kPlanThreads * j;
        s[j] = -INFINITY;
        if (t < ntall && !unpred[j]) {
            const float4* kr = reinterpret_cast<const float4*>(kbar + (int64_t)t * D);
            float a = 0.f;
#pragma unroll 8
            for (int d = 0; d < D / 4; ++d) {
                const float4 kv = kr[d];
                a = fmaf(qs[4 * d], kv.x, a);
                a = fmaf(qs[4 * d + 1], kv.y, a);
                a = fmaf(qs[4 * d + 2], kv.z, a);
                a = fmaf(qs[4 * d + 3], kv.w, a);
            }
            s[j] = a * p.scale;
        }
        mx = fmaxf(mx, s[j]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    if ((tid & 63) == 0) redm[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));

    int flip = 0;
    float wsum = 0.f;
#pragma unroll
    for (int j = 0; j < kPlanPer; ++j) {
        const int t = tid + kPlanThreads * j;
        pr[j] = 0.f;
        if (t < ntall && !unpred[j]) {
            const int n = t == ntall - 1 ? p.lk - kKV * (ntall - 1) : kKV;
            pr[j] = (float)n * (p.folded ? exp2f(s[j] - mx) : expf(s[j] - mx));
        }
        wsum += pr[j];
    }
    wsum = plan_block_sum(wsum, red, flip);
#pragma unroll
    for (int j = 0; j < kPlanPer; ++j) pr[j] = kGated && !(wsum > 0.f) ? 0.f : pr[j] / wsum;      // (0: every tile is in U)

    // the forced set: row i of the table, clipped as attn_ppd_kernel<T, D, 2> clips it
    int fb[3] = {0, 0, 0}, fe[3] = {0, 0, 0};
    if (p.keep) {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            int b = p.keep[(int64_t)i * 6 + 2 * g], e = p.keep[(int64_t)i * 6 + 2 * g + 1];
            b = b < 0 ? 0 : (b > ntall ? ntall : b);
            e = e < b ? b : (e > ntall ? ntall : e);
            fb[g] = b;
            fe[g] = e;
        }
    }
    bool forced[kPlanPer];
    float mf = 0.f;
#pragma unroll
    for (int j = 0; j < kPlanPer; ++j) {
        const int t = tid + kPlanThreads * j;
        forced[j] = t < ntall && ((t >= fb[0] && t < fe[0]) || (t >= fb[1] && t < fe[1]) || (t >= fb[2] && t < fe[2]));
        mf += forced[j] ? pr[j] : 0.f;
    }
    mf = plan_block_sum(mf, red, flip);
    if constexpr (kGated) {                          // from here on U is kept as F is (its p is 0: it added nothing to m_F)
#pragma unroll
        for (int j = 0; j < kPlanPer; ++j) forced[j] = forced[j] || unpred[j];
    }

    // theta's bit pattern: the largest in [0, +inf] whose kept mass reaches cdf; 0 (everything) if none does
    uint32_t lo = 0u, hi = 0x7f800001u;
    if (mf >= cdf) lo = 0x7f800000u;                 // F alone: no finite p reaches +inf
    else {
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < kPlanPer; ++j) m += (!forced[j] && __float_as_uint(pr[j]) >= mid) ? pr[j] : 0.f;
            m = mf + plan_block_sum(m, red, flip);
            if (m >= cdf) lo = mid;
            else hi = mid;
        }
    }
    uint32_t* mrow = p.mask + ((int64_t)hb * p.nqb + i) * p.words;
#pragma unroll
    for (int j = 0; j < kPlanPer; ++j) {
        const int t = tid + kPlanThreads * j;
        const bool keep = t < ntall && (forced[j] || __float_as_uint(pr[j]) >= lo);
        const unsigned long long bal = __ballot(keep);
        const int w0 = (t & ~63) >> 5;               // the wave's 64 tiles: two words
        if ((tid & 63) == 0) {
            if (w0 < p.words) mrow[w0] = (uint32_t)bal;
            if (w0 + 1 < p.words) mrow[w0 + 1] = (uint32_t)(bal >> 32);
        }
    }
    for (int w = 2 * kAttnMaxTiles / 64 + tid; w < p.words; w += kPlanThreads) mrow[w] = 0u;
}

// both entry points; with neither a per-head table nor the gate the two ungated kernels are launched, as ever
int plan_run(const char* name, const void* q, const void* k, int batch, int heads, int64_t lq, int64_t lk, int head_dim,
             int64_t q_bs, int64_t q_rs, int64_t q_hs, int64_t k_bs, int64_t k_rs, int64_t k_hs, float scale, int dtype, float cdf,
             const float* cdf_heads, float sim_threshold, bool gated, const int* keep_ranges, uint32_t* mask, int words,
             void* workspace, int64_t workspace_bytes, void* stream) {
    FINO_CHECK(dtype == FINO_BF16 || dtype == FINO_F16, FINO_ERR_ARG, "%s: dtype %d", name, dtype);
    FINO_CHECK(q && k && mask && workspace, FINO_ERR_ARG, "%s: null pointer", name);
    FINO_CHECK(fino_attn_tiles_supported(batch, heads, lq, lk, head_dim), FINO_ERR_UNSUPPORTED,
               "%s: needs head_dim 64 | 128 and at most %d key tiles (got head_dim %d, Lk %lld)", name, kAttnMaxTiles,
               head_dim, (long long)lk);
    const int64_t nqb = (lq + kQBlock - 1) / kQBlock, ntall = (lk + kKV - 1) / kKV;
    FINO_CHECK(words > 0 && (int64_t)words * 32 >= ntall, FINO_ERR_ARG,
               "%s: %d mask words per q-block do not hold %lld key tiles", name, words, (long long)ntall);
    FINO_CHECK(fino_aligned16(q) && fino_aligned16(k) && q_rs % 8 == 0 && k_rs % 8 == 0 && q_hs % 8 == 0 && k_hs % 8 == 0 &&
                   q_bs % 8 == 0 && k_bs % 8 == 0,
               FINO_ERR_ARG, "%s: pointers and strides must be 16-byte aligned", name);
    FINO_CHECK(((uintptr_t)mask & 3) == 0 && ((uintptr_t)keep_ranges & 3) == 0 && fino_aligned16(workspace), FINO_ERR_ARG,
               "%s: mask / keep_ranges must be 4-byte, the workspace 16-byte aligned", name);
    FINO_CHECK(((uintptr_t)cdf_heads & 3) == 0, FINO_ERR_ARG, "%s: cdf_heads must be 4-byte aligned", name);
    FINO_CHECK(sim_threshold == sim_threshold && sim_threshold <= 1.0f, FINO_ERR_ARG,
               "%s: sim_threshold must be in (0, 1] (<= 0: the gate is off)", name);
    const bool sim = gated && sim_threshold > 0.f;
    const int64_t plain = fino_attn_tile_plan_bytes(batch, heads, lq, lk, head_dim);
    const int64_t need = sim ? fino_attn_tile_plan_gated_bytes(batch, heads, lq, lk, head_dim) : plain;
    FINO_CHECK(workspace_bytes >= need, FINO_ERR_ARG, "%s: workspace of %lld bytes needed", name, (long long)need);
    FINO_CHECK(scale > 0.f || scale == FINO_ATTN_SCALE_FOLDED, FINO_ERR_ARG, "%s: scale must be > 0 (or FINO_ATTN_SCALE_FOLDED)",
               name);
    FINO_CHECK(cdf > 0.f, FINO_ERR_ARG, "%s: cdf must be > 0", name);
    FINO_CHECK((int64_t)batch * heads < 65536 && nqb < (1ll << 30), FINO_ERR_UNSUPPORTED, "%s: grid too large", name);
    PlanParams p;
    p.q = (const uint16_t*)q; p.k = (const uint16_t*)k;
    p.batch = batch; p.heads = heads; p.lq = (int)lq; p.lk = (int)lk; p.nqb = (int)nqb; p.ntall = (int)ntall;
    p.q_bs = q_bs; p.q_rs = q_rs; p.q_hs = q_hs; p.k_bs = k_bs; p.k_rs = k_rs; p.k_hs = k_hs;
    p.folded = scale == FINO_ATTN_SCALE_FOLDED;
    p.scale = p.folded ? 1.0f : scale;
    p.cdf = cdf; p.keep = keep_ranges; p.mask = mask; p.words = words; p.ws = (float*)workspace;
    PlanGate g;
    g.cdf_heads = cdf_heads;
    g.sim_thr = sim ? sim_threshold : 0.f;
    g.sim = sim ? (float*)workspace + plain / 4 : nullptr;
    hipStream_t st = (hipStream_t)stream;
    const dim3 gpool((unsigned)(nqb + ntall), (unsigned)(batch * heads)), gsel((unsigned)nqb, (unsigned)(batch * heads));
    const bool bf = dtype == FINO_BF16;
    // the pool pass pays for the normalised sums only under the gate; a per-head table alone needs the gated select only
    if (head_dim == 128) {
        if (sim) {
            if (bf) attn_plan_pool_kernel<BF16, 128><<<gpool, kPlanThreads, 0, st>>>(p, g);
            else attn_plan_pool_kernel<F16, 128><<<gpool, kPlanThreads, 0, st>>>(p, g);
        } else {
            if (bf) attn_plan_pool_kernel<BF16, 128><<<gpool, kPlanThreads, 0, st>>>(p);
            else attn_plan_pool_kernel<F16, 128><<<gpool, kPlanThreads, 0, st>>>(p);
        }
        FINO_LAUNCH_CHECK();
        if (sim || cdf_heads) attn_plan_select_kernel<128><<<gsel, kPlanThreads, 0, st>>>(p, g);
        else attn_plan_select_kernel<128><<<gsel, kPlanThreads, 0, st>>>(p);
    } else {
        if (sim) {
            if (bf) attn_plan_pool_kernel<BF16, 64><<<gpool, kPlanThreads, 0, st>>>(p, g);
            else attn_plan_pool_kernel<F16, 64><<<gpool, kPlanThreads, 0, st>>>(p, g);
        } else {
            if (bf) attn_plan_pool_kernel<BF16, 64><<<gpool, kPlanThreads, 0, st>>>(p);
            else attn_plan_pool_kernel<F16, 64><<<gpool, kPlanThreads, 0, st>>>(p);
        }
        FINO_LAUNCH_CHECK();
        if (sim || cdf_heads) attn_plan_select_kernel<64><<<gsel, kPlanThreads, 0, st>>>(p, g);
        else attn_plan_select_kernel<64><<<gsel, kPlanThreads, 0, st>>>(p);
    }
    FINO_LAUNCH_CHECK();
    return FINO_OK;
}

}  // namespace

extern "C" int64_t fino_attn_tile_plan_bytes(int batch, int heads, int64_t lq, int64_t lk, int head_dim) {
    if (!fino_attn_tiles_supported(batch, heads, lq, lk, head_dim)) return 0;
    return (int64_t)batch * heads * ((lq + kQBlock - 1) / kQBlock + (lk + kKV - 1) / kKV) * head_dim * 4;
}

// qbar | kbar | sim_q | sim_k, the whole a multiple of 16 bytes (head_dim * 4 already is one per pooled row)
extern "C" int64_t fino_attn_tile_plan_gated_bytes(int batch, int heads, int64_t lq, int64_t lk, int head_dim) {
    const int64_t plain = fino_attn_tile_plan_bytes(batch, heads, lq, lk, head_dim);
    if (plain == 0) return 0;
    return plain + (int64_t)batch * heads * ((lq + kQBlock - 1) / kQBlock + (lk + kKV - 1) / kKV) * 4;
}

extern "C" int fino_attn_tile_plan(const void* q, const void* k, int batch, int heads, int64_t lq, int64_t lk, int head_dim,
                                   int64_t q_bs, int64_t q_rs, int64_t q_hs, int64_t k_bs, int64_t k_rs, int64_t k_hs,
                                   float scale, int dtype, float cdf, const int* keep_ranges, uint32_t* mask, int words,
                                   void* workspace, int64_t workspace_bytes, void* stream) {
    return plan_run("fino_attn_tile_plan", q, k, batch, heads, lq, lk, head_dim, q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, scale, dtype,
                    cdf, nullptr, 0.f, false, keep_ranges, mask, words, workspace, workspace_bytes, stream);
}

extern "C" int fino_attn_tile_plan_gated(const void* q, const void* k, int batch, int heads, int64_t lq, int64_t lk,
                                         int head_dim, int64_t q_bs, int64_t q_rs, int64_t q_hs, int64_t k_bs, int64_t k_rs,
                                         int64_t k_hs, float scale, int dtype, float cdf, const float* cdf_heads,
                                         float sim_threshold, const int* keep_ranges, uint32_t* mask, int words, void* workspace,
                                         int64_t workspace_bytes, void* stream) {
    return plan_run("fino_attn_tile_plan_gated", q, k, batch, heads, lq, lk, head_dim, q_bs, q_rs, q_hs, k_bs, k_rs, k_hs, scale,
                    dtype, cdf, cdf_heads, sim_threshold, true, keep_ranges, mask, words, workspace, workspace_bytes, stream);
}
