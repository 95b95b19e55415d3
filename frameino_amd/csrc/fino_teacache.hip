// TeaCache's probe (frameino_amd/step_cache.py): how far the timestep-modulated input of the first block has moved since the
// previous forward, measured before block 0 runs.
//
// fino_teacache_probe, over rows [rows, dim]:
//   m = T(LN(x) * (1 + scale[sel[row]]) + shift[sel[row]])      the bits fino_adaln_modulate writes (plain mode, shift and
//                                                                scale NULL: m = x)
//   stats[0] = sum |float(m) - float(p)|,  stats[1] = sum |float(p)|        p = the row `plane` held (compare != 0)
//   plane = m
// One wave per row at a time with the row in registers: the row loading, the fp32 row statistics and the modulation are
// fino_row_ln.h's, the code ln_modulate_kernel MODE 0 runs.  A lane reads its 16-byte vectors of the previous plane and stores
// m over them: no two lanes share an element, so the plane is updated in place.  Per row the two sums are formed in fp32 from
// the rounded values (a lane adds its elements in order, then the xor butterfly); the wave with global index g takes the rows
// g, g + W, ... (W = the launch's wave count, a function of `rows` alone) and adds their sums in that order, in fp64, into
// partial[2 g], partial[2 g + 1]; a second launch adds the partials in a fixed order.  No atomics: the same inputs give the same
// bits on every run.  HBM-bound: three planes move (x in, p in, m out) where fino_adaln_modulate moves two.
// Built with -ffp-contract=off, like fino_elementwise.hip.
#include "fino_common.h"
#include "fino_host.h"
#include "fino_row_ln.h"

namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kThreads = kWavesPerBlock * 64;
constexpr int kMaxPasses = 8;           // dim <= 8 * 512 = 4096, as the row kernels
constexpr int kMaxBlocks = (int)kFinoGridCap8;

template <typename T, int NP, bool MOD>
__global__ __launch_bounds__(kThreads) void teacache_probe_kernel(
    const uint16_t* __restrict__ x, int64_t ldx, uint16_t* plane, int64_t ldp, int64_t rows, int dim,
    const float* __restrict__ p_shift, const float* __restrict__ p_scale, int64_t mod_stride, const int32_t* __restrict__ sel,
    float eps, int compare, double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    double sum_diff = 0., sum_prev = 0.;
    for (int64_t row = wave; row < rows; row += nwaves) {               // wave-uniform: every lane reaches the butterflies
        float v[NP][8];
        load_row<T, NP>(x + row * ldx, dim, lane, v);
        float mean = 0.f, rstd = 1.f;
        int64_t moff = 0;
        if constexpr (MOD) {
            ln_stats<NP>(v, dim, lane, eps, mean, rstd);
            moff = sel ? (int64_t)sel[row] * mod_stride : 0;
        }
        float a = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c >= dim) continue;
            uint4 m;
            if constexpr (MOD) {
                float o[8], sc[8], sh[8];
                ln_ld8(p_scale + moff + c, sc);
                ln_ld8(p_shift + moff + c, sh);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] = ln_adaln_value(v[i][j], mean, rstd, sc[j], sh[j]);
                m = pack8<T>(o);
            } else {
                m = pack8<T>(v[i]);                                     // (exact: the values came from T)
            }
            uint16_t* dst = plane + row * ldp + c;
            if (compare) {
                float fm[8], fp[8];
                unpack8<T>(m, fm);
                unpack8<T>(*reinterpret_cast<const uint4*>(dst), fp);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    a += fabsf(fm[j] - fp[j]);
                    q += fabsf(fp[j]);
                }
            }
            *reinterpret_cast<uint4*>(dst) = m;
        }
        if (compare) {                                                   // (a launch argument: uniform)
            sum_diff += (double)wave_sum(a);
            sum_prev += (double)wave_sum(q);
        }
    }
    if (lane == 0) {
        partial[2 * wave] = sum_diff;
        partial[2 * wave + 1] = sum_prev;
    }
}

// stats = the sum of the n wave partials: thread t adds the partials t, t + 256, ... in order, then the xor butterfly and the
// waves in index order, all in fp64 -- a fixed order
__global__ __launch_bounds__(kThreads) void teacache_finish_kernel(const double* __restrict__ partial, int64_t n,
                                                                   double* __restrict__ stats) {
    __shared__ double red[2][kWavesPerBlock];
    constexpr int kPer = kMaxBlocks * kWavesPerBlock / kThreads;        // partials per thread at the grid's cap
    const double2* pairs = (const double2*)partial;
    double2 p[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {                // every load in flight before the first add
        const int64_t j = threadIdx.x + (int64_t)k * kThreads;
        p[k] = j < n ? pairs[j] : make_double2(0., 0.);
    }
    double a = 0., q = 0.;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        a += p[k].x;
        q += p[k].y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0];
        q = red[1][0];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) {
            a += red[0][w];
            q += red[1][w];
        }
        stats[0] = a;
        stats[1] = q;
    }
}

// the waves of a probe launch over `rows` rows: one per row up to the grid's cap, whole workgroups
int64_t teacache_waves(int64_t rows) {
    return (int64_t)fino_grid_1d(rows, kMaxBlocks, true, kWavesPerBlock) * kWavesPerBlock;
}

}  // namespace

extern "C" int64_t fino_teacache_workspace_bytes(int64_t rows) {
    return rows < 1 ? 0 : teacache_waves(rows) * 2 * (int64_t)sizeof(double);
}

extern "C" int fino_teacache_probe(const void* x, int64_t ldx, void* plane, int64_t ld_plane, int64_t rows, int dim,
                                   const float* shift, const float* scale, int64_t mod_stride, const int32_t* sel, float eps,
                                   int compare, int dtype, double* stats, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
    const char* who = "fino_teacache_probe";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(rows >= 1 && rows < (1LL << 31), FINO_ERR_ARG, "%s: rows=%lld (1 .. 2^31 - 1)", who, (long long)rows);
    FINO_CHECK(dim > 0 && dim % 8 == 0, FINO_ERR_ARG, "%s: dim=%d must be a multiple of 8", who, dim);
    FINO_CHECK(x && plane && stats && workspace, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_CHECK((shift == nullptr) == (scale == nullptr), FINO_ERR_ARG,
               "%s: shift and scale come together (both NULL: the plain mode)", who);
    FINO_CHECK(shift || !sel, FINO_ERR_ARG, "%s: a selector needs shift and scale", who);
    FINO_TRY(fino_check_strides(who, dim, {ldx, ld_plane}));
    const bool mod_rows_ok = !shift || mod_stride % 4 == 0;     // the fp32 modulation rows are read 16 bytes at a time too
    FINO_TRY(fino_check_aligned16(who, 8, {{x, ldx}, {plane, ld_plane}, {shift, 0}, {scale, 0}, {stats, 0}, {workspace, 0}},
                                  mod_rows_ok));
    FINO_CHECK(x != plane, FINO_ERR_ARG, "%s: the plane is x itself (it is rewritten while x is read)", who);
    FINO_CHECK(workspace_bytes >= fino_teacache_workspace_bytes(rows), FINO_ERR_ARG,
               "%s: workspace of %lld bytes, need %lld (fino_teacache_workspace_bytes)", who, (long long)workspace_bytes,
               (long long)fino_teacache_workspace_bytes(rows));
    FINO_CHECK(dim <= kMaxPasses * 512, FINO_ERR_UNSUPPORTED, "%s: dim %d > %d unsupported", who, dim, kMaxPasses * 512);
    const int64_t nwaves = teacache_waves(rows);
    const int grid = (int)(nwaves / kWavesPerBlock);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    const uint16_t* xp = (const uint16_t*)x;
    uint16_t* pp = (uint16_t*)plane;
    dispatch_np<kMaxPasses>(dim, [&](auto np) {
        fino_dispatch_dtype(dtype, [&](auto t) {
            constexpr int NP = decltype(np)::value;
            if (shift)
                teacache_probe_kernel<decltype(t), NP, true><<<grid, kThreads, 0, st>>>(
                    xp, ldx, pp, ld_plane, rows, dim, shift, scale, mod_stride, sel, eps, compare, partial);
            else
                teacache_probe_kernel<decltype(t), NP, false><<<grid, kThreads, 0, st>>>(
                    xp, ldx, pp, ld_plane, rows, dim, nullptr, nullptr, 0, nullptr, eps, compare, partial);
        });
    });
    FINO_TRY(fino_launch_check(who));
    teacache_finish_kernel<<<1, kThreads, 0, st>>>(partial, nwaves, stats);
    return fino_launch_check(who);
}
