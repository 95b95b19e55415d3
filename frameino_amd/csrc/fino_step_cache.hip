// First-block caching of the Wan DiT (diffusers' FirstBlockCache; frameino_amd/step_cache.py): the per-step probe of the
// first block's residual and the two residual-stream updates around the skipped blocks.
//
// fino_step_cache_probe, per segment s (one CFG branch, or one joint batch):
//   r = T(h1 - h0)                                           written to r (and h1 copied to h1_copy when given)
//   sums[2 s]     = sum |T(r - p)|      sums[2 s + 1] = sum |p|        (fp32; p == NULL counts as zeros)
// The host divides and compares (step_cache.decide).  Deterministic: every segment is cut into FINO_STEP_CACHE_BLOCKS row
// ranges by its row count alone, each workgroup sums its range in a fixed order (per-thread sequential, xor-butterfly across
// the wave, waves in index order) and stores one partial; a second launch adds the partials in index order.  No atomics: the
// same inputs give the same bits on every run, whatever order the workgroups run in.
//
// fino_step_cache_residual: out = T(a - b) or T(a + b) -- bit-exact to torch's `a - b` / `a + b` in T (one fp32 operation,
// one rounding).
//
// fino_pab_broadcast (Pyramid Attention Broadcast): out = T(fma(float(y), gate[sel[row]], float(x))), or T(x + y) without a
// gate -- the arithmetic of the GEMM's FINO_EPI_GATED_RESIDUAL / FINO_EPI_RESIDUAL epilogue on a cached y = T(acc + bias).
// That epilogue compiles to ONE fused multiply-add per element (v_pk_fma_f32 / v_fmac_f32: fino_gemm.hip is built with the
// compiler's default contraction), so the fma is spelled out here: a step that re-uses y gives the bits of the step that
// computed it.  (fino_gated_residual multiplies and adds with two roundings.)
//
// fino_taylor_update / fino_taylor_predict (TaylorSeer): the finite-difference factors of a hooked tensor along the step axis,
// updated in place on a computing step, and the Taylor extrapolation a predicting step writes or adds to the residual stream
// with fino_pab_broadcast's arithmetic (include/frameino_hip.h spells out both).
//
// fino_fastercache_delta / fino_fastercache_apply (FasterCache): the frequency-split difference D = u - c of the two CFG
// predictions of a step that ran both, DL = LP(D) and DH = D - DL (LP: the radial low-pass of every [H, W] plane), and the
// unconditional prediction a later step rebuilds from its conditional one, T((c + aL * DL) + aH * DH).  The low-pass is a
// direct DFT over the half disk of kept bins, one workgroup per plane with the plane in LDS (below).
//
// fino_magcache_calibrate (MagCache's calibration pass): the residual r_new = T(x_out - x_in) of the whole block stack -- the
// bits fino_step_cache_residual writes -- and, in the same pass over HBM, the mean over rows of ||r_new|| / (||r_prev|| + 1e-8)
// and of the cosine distance to r_prev.  Per-row sums in fp32, sums over rows in fp64, one partial per wave and a second
// launch that adds the partials in a fixed order: no atomics.
//
// HBM-bound: 16-byte loads and stores, fp32 arithmetic, no contraction (the file is built with -ffp-contract=off).
#include "fino_common.h"
#include "fino_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 2;

// 16-byte vectors of the storage type as fp32 lanes
template <typename T>
struct Io {
    static constexpr int kElems = 8;
    static constexpr int kBytes = 2;
    static __device__ __forceinline__ void unpack(const uint4& v, float (&f)[8]) { unpack8<T>(v, f); }
    static __device__ __forceinline__ uint4 pack(const float (&f)[8]) { return pack8<T>(f); }
    static __device__ __forceinline__ float rnd(float x) { return round_to<T>(x); }
};
struct F32 {};
template <>
struct Io<F32> {
    static constexpr int kElems = 4;
    static constexpr int kBytes = 4;
    static __device__ __forceinline__ void unpack(const uint4& v, float (&f)[4]) {
        f[0] = __uint_as_float(v.x);
        f[1] = __uint_as_float(v.y);
        f[2] = __uint_as_float(v.z);
        f[3] = __uint_as_float(v.w);
    }
    static __device__ __forceinline__ uint4 pack(const float (&f)[4]) {
        return make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
    }
    static __device__ __forceinline__ float rnd(float x) { return x; }
};

struct ProbeArgs {
    FinoStepCacheSegment seg[FINO_STEP_CACHE_MAX_SEGMENTS];
    uint32_t vpr;                       // 16-byte vectors per row
};

__device__ __forceinline__ const uint4* at(const void* base, int64_t row, int64_t ld, uint32_t col, int esize) {
    return (const uint4*)((const char*)base + (row * ld + col) * esize);
}

// (a, q) of the workgroup: thread 0 gets the sums, in a fixed order
__device__ __forceinline__ void block_sum2(float& a, float& q) {
    __shared__ float red[2][kThreads / 64];
    a = wave_sum(a);
    q = wave_sum(q);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = a;
        red[1][wave] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0];
        q = red[1][0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            a += red[0][w];
            q += red[1][w];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void probe_kernel(ProbeArgs args, float* partial) {
    using IO = Io<T>;
    constexpr int E = IO::kElems;
    const FinoStepCacheSegment& g = args.seg[blockIdx.y];
    const int64_t r0 = g.rows * blockIdx.x / FINO_STEP_CACHE_BLOCKS, r1 = g.rows * (blockIdx.x + 1) / FINO_STEP_CACHE_BLOCKS;
    const uint32_t vpr = args.vpr, nvec = (uint32_t)(r1 - r0) * vpr;
    float sa = 0.f, sq = 0.f;
    for (uint32_t i0 = threadIdx.x; i0 < nvec; i0 += kThreads * kUnroll) {
        uint4 v0[kUnroll], v1[kUnroll], vp[kUnroll];
        int64_t row[kUnroll];
        uint32_t col[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const uint32_t i = i0 + u * kThreads;
            if (i < nvec) {
                row[u] = r0 + i / vpr;
                col[u] = (i % vpr) * E;
                v0[u] = *at(g.h0, row[u], g.ld_h0, col[u], IO::kBytes);
                v1[u] = *at(g.h1, row[u], g.ld_h1, col[u], IO::kBytes);
                vp[u] = g.p ? *at(g.p, row[u], g.ld_p, col[u], IO::kBytes) : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (i0 + u * kThreads >= nvec) break;
            float f0[E], f1[E], fp[E], fr[E];
            IO::unpack(v0[u], f0);
            IO::unpack(v1[u], f1);
            IO::unpack(vp[u], fp);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                fr[e] = IO::rnd(f1[e] - f0[e]);
                sa += fabsf(IO::rnd(fr[e] - fp[e]));
                sq += fabsf(fp[e]);
            }
            *(uint4*)at(g.r, row[u], g.ld_r, col[u], IO::kBytes) = IO::pack(fr);
            if (g.h1_copy) *(uint4*)at(g.h1_copy, row[u], g.ld_h1_copy, col[u], IO::kBytes) = v1[u];
        }
    }
    block_sum2(sa, sq);
    if (threadIdx.x == 0) {
        float* dst = partial + 2 * ((int64_t)blockIdx.y * FINO_STEP_CACHE_BLOCKS + blockIdx.x);
        dst[0] = sa;
        dst[1] = sq;
    }
}

__global__ __launch_bounds__(kThreads) void probe_finish_kernel(const float* partial, float* sums) {
    const float* src = partial + 2 * (int64_t)blockIdx.x * FINO_STEP_CACHE_BLOCKS;
    float sa = 0.f, sq = 0.f;
    for (int j = threadIdx.x; j < FINO_STEP_CACHE_BLOCKS; j += kThreads) {
        sa += src[2 * j];
        sq += src[2 * j + 1];
    }
    block_sum2(sa, sq);
    if (threadIdx.x == 0) {
        sums[2 * blockIdx.x] = sa;
        sums[2 * blockIdx.x + 1] = sq;
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void residual_kernel(const void* a, int64_t lda, const void* b, int64_t ldb, void* out,
                                                            int64_t ldo, uint32_t vpr, uint32_t nvec, int subtract) {
    using IO = Io<T>;
    constexpr int E = IO::kElems;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < nvec; i += gridDim.x * kThreads) {
        const int64_t row = i / vpr;
        const uint32_t col = (i % vpr) * E;
        float fa[E], fb[E], fo[E];
        IO::unpack(*at(a, row, lda, col, IO::kBytes), fa);
        IO::unpack(*at(b, row, ldb, col, IO::kBytes), fb);
#pragma unroll
        for (int e = 0; e < E; ++e) fo[e] = subtract ? fa[e] - fb[e] : fa[e] + fb[e];
        *(uint4*)at(out, row, ldo, col, IO::kBytes) = IO::pack(fo);
    }
}

// ---- MagCache calibration: r_new = T(x_out - x_in) and, per row, ||r_new||, ||r_prev||, <r_new, r_prev> in fp32 from the
// rounded values.  One wave per row at a time: lane l takes the 16-byte vectors l, l + 64, ... of the row in order (the loads
// of kMagUnroll of them per plane in flight), then the xor butterfly; the wave with global index g takes the rows g, g + W,
// ... (W = the launch's wave count, a function of `rows` alone) and adds their ratio and cosine distance in that order, in
// fp64, into partial[2 g], partial[2 g + 1].  Every r_prev vector of a thread is in registers before the thread's first
// store of the chunk, and no two threads share an element: r_new may be r_prev.
constexpr int kMagUnroll = 4;           // (2, 3, 4 and 6 vectors per plane in flight, and a cap of 1024 / 1280 / 2048
constexpr int kMagWavesPerBlock = kThreads / 64;        // workgroups, measure alike at [24640, 3072]: within the run's spread)
constexpr int kMagMaxBlocks = (int)kFinoGridCap8;

template <typename T>
__global__ __launch_bounds__(kThreads) void magcache_kernel(const void* x_out, int64_t ld_out, const void* x_in, int64_t ld_in,
                                                            const void* r_prev, int64_t ld_prev, void* r_new, int64_t ld_new,
                                                            int64_t rows, uint32_t vpr, double* partial) {
    using IO = Io<T>;
    constexpr int E = IO::kElems;
    const uint32_t lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * kMagWavesPerBlock + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * kMagWavesPerBlock;
    double sum_ratio = 0., sum_cos = 0.;
    for (int64_t row = wave; row < rows; row += nwaves) {               // wave-uniform: every lane reaches the butterfly
        float nn = 0.f, pp = 0.f, np = 0.f;
        for (uint32_t v0 = lane; v0 < vpr; v0 += 64 * kMagUnroll) {
            uint4 vo[kMagUnroll], vi[kMagUnroll], vp[kMagUnroll];
#pragma unroll
            for (int u = 0; u < kMagUnroll; ++u) {
                const uint32_t v = v0 + u * 64;
                if (v < vpr) {
                    vo[u] = *at(x_out, row, ld_out, v * E, IO::kBytes);
                    vi[u] = *at(x_in, row, ld_in, v * E, IO::kBytes);
                    vp[u] = *at(r_prev, row, ld_prev, v * E, IO::kBytes);
                }
            }
#pragma unroll
            for (int u = 0; u < kMagUnroll; ++u) {
                const uint32_t v = v0 + u * 64;
                if (v >= vpr) break;
                float fo[E], fi[E], fp[E], fr[E];
                IO::unpack(vo[u], fo);
                IO::unpack(vi[u], fi);
                IO::unpack(vp[u], fp);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    fr[e] = IO::rnd(fo[e] - fi[e]);
                    nn += fr[e] * fr[e];
                    pp += fp[e] * fp[e];
                    np += fr[e] * fp[e];
                }
                *(uint4*)at(r_new, row, ld_new, v * E, IO::kBytes) = IO::pack(fr);
            }
        }
        nn = wave_sum(nn);
        pp = wave_sum(pp);
        np = wave_sum(np);
        const float norm_new = sqrtf(nn), norm_prev = sqrtf(pp);
        const float ratio = norm_new / (norm_prev + 1e-8f);
        const float cos_dist = 1.f - np / fmaxf(norm_new * norm_prev, 1e-8f);
        sum_ratio += (double)ratio;
        sum_cos += (double)cos_dist;
    }
    if (lane == 0) {
        partial[2 * wave] = sum_ratio;
        partial[2 * wave + 1] = sum_cos;
    }
}

// stats = (sum of the n wave partials) / rows: thread t adds the partials t, t + 256, ... in order, then the xor butterfly and
// the waves in index order, all in fp64 -- a fixed order
__global__ __launch_bounds__(kThreads) void magcache_finish_kernel(const double* partial, int64_t n, double rows, double* stats) {
    __shared__ double red[2][kThreads / 64];
    constexpr int kPer = kMagMaxBlocks * kMagWavesPerBlock / kThreads;      // partials per thread at the grid's cap
    const double2* pairs = (const double2*)partial;
    double2 p[kPer];
#pragma unroll
    for (int k = 0; k < kPer; ++k) {                // every load in flight before the first add: one round trip, not kPer
        const int64_t j = threadIdx.x + (int64_t)k * kThreads;
        p[k] = j < n ? pairs[j] : make_double2(0., 0.);
    }
    double a = 0., c = 0.;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        a += p[k].x;
        c += p[k].y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0];
        c = red[1][0];
#pragma unroll
        for (int w = 1; w < kThreads / 64; ++w) {
            a += red[0][w];
            c += red[1][w];
        }
        stats[0] = a / rows;
        stats[1] = c / rows;
    }
}

// the waves of a fino_magcache_calibrate launch over `rows` rows: one per row up to the grid's cap, whole workgroups
int64_t magcache_waves(int64_t rows) {
    return (int64_t)fino_grid_1d(rows, kMagMaxBlocks, true, kMagWavesPerBlock) * kMagWavesPerBlock;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void pab_broadcast_kernel(const void* x, int64_t ldx, const void* y, int64_t ldy, void* out,
                                                                 int64_t ldo, uint32_t vpr, uint32_t nvec, const float* gate,
                                                                 int64_t mod_stride, const int32_t* sel) {
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < nvec; i += gridDim.x * kThreads) {
        const int64_t row = i / vpr;
        const uint32_t col = (i % vpr) * 8;
        float fx[8], fy[8], fo[8];
        unpack8<T>(*at(x, row, ldx, col, 2), fx);
        unpack8<T>(*at(y, row, ldy, col, 2), fy);
        if (gate) {
            const float* g = gate + (sel ? (int64_t)sel[row] * mod_stride : 0) + col;
            const float4 g0 = *reinterpret_cast<const float4*>(g);
            const float4 g1 = *reinterpret_cast<const float4*>(g + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) fo[e] = __builtin_fmaf(fy[e], gg[e], fx[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) fo[e] = fx[e] + fy[e];
        }
        *(uint4*)at(out, row, ldo, col, 2) = pack8<T>(fo);
    }
}

// ---- TaylorSeer: 8 consecutive elements of a factor plane (dtype F) as fp32 lanes: one 16-byte vector, two for fp32 planes
template <typename F>
struct Plane {
    static __device__ __forceinline__ void load(const void* base, int64_t off, float (&f)[8]) {
        unpack8<F>(*(const uint4*)((const char*)base + off * 2), f);
    }
    static __device__ __forceinline__ void store(void* base, int64_t off, const float (&f)[8]) {
        *(uint4*)((char*)base + off * 2) = pack8<F>(f);
    }
    static __device__ __forceinline__ float rnd(float x) { return round_to<F>(x); }
};
template <>
struct Plane<F32> {
    static __device__ __forceinline__ void load(const void* base, int64_t off, float (&f)[8]) {
        const float4* p = (const float4*)((const char*)base + off * 4);
        const float4 a = p[0], b = p[1];
        f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
    }
    static __device__ __forceinline__ void store(void* base, int64_t off, const float (&f)[8]) {
        float4* p = (float4*)((char*)base + off * 4);
        p[0] = make_float4(f[0], f[1], f[2], f[3]);
        p[1] = make_float4(f[4], f[5], f[6], f[7]);
    }
    static __device__ __forceinline__ float rnd(float x) { return x; }
};

constexpr int kTaylorPlanes = FINO_TAYLOR_MAX_PLANES;

// g_0 = F(y), g_{i+1} = F((g_i - f_i) / delta) for i + 1 < n_new; planes 0 .. n_new - 1 are rewritten in place.  Every old
// plane a thread needs (0 .. n_new - 2) is in registers before its first store; no two threads share an element.
template <typename T, typename F>
__global__ __launch_bounds__(kThreads) void taylor_update_kernel(const void* y, int64_t ldy, void* fac, int64_t plane, int64_t ldf,
                                                                 uint32_t vpr, uint32_t nvec, int n_new, float delta) {
    using P = Plane<F>;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < nvec; i += gridDim.x * kThreads) {
        const int64_t row = i / vpr;
        const uint32_t col = (i % vpr) * 8;
        const int64_t off = row * ldf + col;
        float g[8], old[kTaylorPlanes - 1][8];
        unpack8<T>(*at(y, row, ldy, col, 2), g);
#pragma unroll
        for (int k = 0; k < kTaylorPlanes - 1; ++k)
            if (k + 1 < n_new) P::load(fac, k * plane + off, old[k]);
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = P::rnd(g[e]);
        P::store(fac, off, g);
#pragma unroll
        for (int k = 0; k < kTaylorPlanes - 1; ++k) {
            if (k + 1 >= n_new) break;
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = P::rnd((g[e] - old[k][e]) / delta);
            P::store(fac, (k + 1) * plane + off, g);
        }
    }
}

struct TaylorCoef {
    float c[kTaylorPlanes];
};

// p = f_0; p = p + f_i * c_i (i = 1 .. n - 1: the product rounded, then the sum: no contraction in this file); then
// out = T(p) | T(p + x) | T(fma(p, gate[sel[row]], x)) -- the last two as pab_broadcast_kernel writes them
template <typename T, typename F>
__global__ __launch_bounds__(kThreads) void taylor_predict_kernel(const void* fac, int64_t plane, int64_t ldf, int n, TaylorCoef coef,
                                                                  const void* x, int64_t ldx, void* out, int64_t ldo, uint32_t vpr,
                                                                  uint32_t nvec, const float* gate, int64_t mod_stride,
                                                                  const int32_t* sel) {
    using P = Plane<F>;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < nvec; i += gridDim.x * kThreads) {
        const int64_t row = i / vpr;
        const uint32_t col = (i % vpr) * 8;
        const int64_t off = row * ldf + col;
        float p[8], f[kTaylorPlanes - 1][8], fx[8], fo[8];
        P::load(fac, off, p);
#pragma unroll
        for (int k = 1; k < kTaylorPlanes; ++k)
            if (k < n) P::load(fac, k * plane + off, f[k - 1]);
        if (x) unpack8<T>(*at(x, row, ldx, col, 2), fx);
#pragma unroll
        for (int k = 1; k < kTaylorPlanes; ++k) {
            if (k >= n) break;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float t = f[k - 1][e] * coef.c[k];
                p[e] = p[e] + t;
            }
        }
        if (!x) {
#pragma unroll
            for (int e = 0; e < 8; ++e) fo[e] = p[e];
        } else if (gate) {
            const float* g = gate + (sel ? (int64_t)sel[row] * mod_stride : 0) + col;
            const float4 g0 = *reinterpret_cast<const float4*>(g);
            const float4 g1 = *reinterpret_cast<const float4*>(g + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) fo[e] = __builtin_fmaf(p[e], gg[e], fx[e]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) fo[e] = fx[e] + p[e];
        }
        *(uint4*)at(out, row, ldo, col, 2) = pack8<T>(fo);
    }
}

// ---- FasterCache: the radial low-pass of one [H, W] plane of D = float(u) - float(c), one workgroup per plane.
// The kept bins are the disk fy^2 + fx^2 <= r^2 of signed frequencies; r = min(H, W) / 5 < min(H, W) / 2, so a bin and its
// mirror (-fy, -fx) are distinct residues on both axes and only the half disk (fy > 0, or fy == 0 and fx >= 0) is
// transformed: row fy of it holds fx = -w[fy] .. w[fy] (fx = 0 .. w[0] in row 0), w[fy] = floor(sqrt(r^2 - fy^2)), and the
// bins are numbered row by row (`off[fy]` = first bin of row fy; bin 0 is the mean).
//   analysis   X[b] = sum_p D[p] (cos - i sin)(2 pi (fy y / H + fx x / W)): one wave per bin, lane l takes the pixels
//              p = l, l + 64, ... in order, then the xor butterfly -- a fixed order, no atomics
//   synthesis  DL[p] = (X[0] + 2 sum_{b > 0} Re(X[b] e^{+i ..})) / (H W): one thread per pixel over the bins in order
// The twiddle of a pixel is the product of two table entries, cos / sin(2 pi k / H) at k = fy y mod H and cos / sin(2 pi k / W) at
// k = fx x mod W, the residues advanced by integer additions: no sine of a large argument, no division in the loops.
// D is fp32 (and DH = D - DL one fp32 subtraction); the tables, the bins and both sums are fp64, so DL is the exact low-pass
// rounded to fp32 once -- a direct fp32 sum would sit a few 1e-8 of max |D| off, which is above what a butterfly leaves on a
// plane whose spectrum is one line.
constexpr int kFcThreads = 512;
constexpr int kFcMaxRows = 32;          // r + 1 <= 26: H W <= 16384 bounds min(H, W) by 128

struct FcDisk {
    int off[kFcMaxRows + 1];
    int w[kFcMaxRows];
};

template <typename T>
__global__ __launch_bounds__(kFcThreads) void fastercache_delta_kernel(const uint16_t* u, const uint16_t* c, float* d_low,
                                                                       float* d_high, int H, int W, int r, int nbins, FcDisk disk) {
    // all LDS in the dynamic region, fp64 first: a static array in front of it would shift the base off 8-byte alignment
    extern __shared__ __attribute__((aligned(16))) double fc_smem[];
    const int HW = H * W, tid = threadIdx.x;
    const int th = r > 0 ? H : 1, tw = r > 0 ? W : 1;      // r == 0: the mean alone, every residue is 0
    double* cy = fc_smem;               // [th] each ...
    double* sy = cy + th;
    double* cx = sy + th;               // ... and [tw] each
    double* sx = cx + tw;
    double* bins = sx + tw;             // [nbins][re, im]
    float* D = (float*)(bins + 2 * nbins);      // [HW]
    int* off = (int*)(D + HW);                  // [kFcMaxRows + 1]: first bin of every row of the half disk
    int* roww = off + kFcMaxRows + 1;           // [kFcMaxRows]: w[fy]
    const int64_t base = (int64_t)blockIdx.x * HW;
    if (tid <= r + 1) off[tid] = disk.off[tid];
    if (tid <= r) roww[tid] = disk.w[tid];
    if ((HW & 7) == 0) {                // every plane starts on a 16-byte boundary
        const uint4* u4 = (const uint4*)(u + base);
        const uint4* c4 = (const uint4*)(c + base);
        for (int i = tid; i < HW / 8; i += kFcThreads) {
            float fu[8], fc[8];
            unpack8<T>(u4[i], fu);
            unpack8<T>(c4[i], fc);
#pragma unroll
            for (int e = 0; e < 8; ++e) D[i * 8 + e] = fu[e] - fc[e];
        }
    } else {
        for (int p = tid; p < HW; p += kFcThreads) D[p] = T::to_f32(u[base + p]) - T::to_f32(c[base + p]);
    }
    for (int k = tid; k < th; k += kFcThreads) {
        const double a = 2.0 * k / H;
        cy[k] = cospi(a);
        sy[k] = sinpi(a);
    }
    for (int k = tid; k < tw; k += kFcThreads) {
        const double a = 2.0 * k / W;
        cx[k] = cospi(a);
        sx[k] = sinpi(a);
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int dx = 64 % W, dy = 64 / W;
    for (int b = wave; b < nbins; b += kFcThreads / 64) {          // wave-uniform: every lane reaches the butterfly
        int fy = 0;
        while (off[fy + 1] <= b) ++fy;
        const int fx = (fy == 0 ? 0 : -roww[fy]) + (b - off[fy]);
        const int fxm = fx < 0 ? fx + W : fx;                      // residues in [0, W) / [0, H): |fx| <= r < W, fy <= r < H
        int x = lane % W, y = lane / W;
        int ix = (fxm * x) % W, iy = (fy * y) % H;                 // (y may pass H for the lanes beyond the plane: they do not loop)
        const int six = (fxm * dx) % W, siy = (fy * dy) % H;
        double re = 0., im = 0.;
        for (int p = lane; p < HW; p += 64) {
            const double v = (double)D[p];
            const double cc = cy[iy] * cx[ix] - sy[iy] * sx[ix];
            const double ss = sy[iy] * cx[ix] + cy[iy] * sx[ix];
            re += v * cc;
            im -= v * ss;
            x += dx;
            ix += six;
            if (ix >= W) ix -= W;
            iy += siy;
            if (iy >= H) iy -= H;
            if (x >= W) {               // the next pixel of this lane lies one row further down
                x -= W;
                iy += fy;
                if (iy >= H) iy -= H;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {          // the xor butterfly in fp64
            re += __shfl_xor(re, o, 64);
            im += __shfl_xor(im, o, 64);
        }
        if (lane == 0) {
            bins[2 * b] = re;
            bins[2 * b + 1] = im;
        }
    }
    __syncthreads();

    const double norm = (double)HW;
    for (int p = tid; p < HW; p += kFcThreads) {
        const int y = p / W, x = p - y * W;
        double acc = 0.;
        int b = 1, iy = 0, ix = 0;
        for (int fx = 1; fx <= roww[0]; ++fx, ++b) {               // row 0: fx = 1 .. w[0] (bin 0, the mean, is added last)
            ix += x;
            if (ix >= W) ix -= W;
            acc += bins[2 * b] * cx[ix] - bins[2 * b + 1] * sx[ix];
        }
        for (int fy = 1; fy <= r; ++fy) {
            iy += y;
            if (iy >= H) iy -= H;
            const int w = roww[fy];
            ix = ((W - w) * x) % W;
            const double cyv = cy[iy], syv = sy[iy];
            for (int fx = -w; fx <= w; ++fx, ++b) {
                const double cc = cyv * cx[ix] - syv * sx[ix];
                const double ss = syv * cx[ix] + cyv * sx[ix];
                acc += bins[2 * b] * cc - bins[2 * b + 1] * ss;
                ix += x;
                if (ix >= W) ix -= W;
            }
        }
        const float dl = (float)((bins[0] + 2. * acc) / norm);
        d_low[base + p] = dl;
        d_high[base + p] = D[p] - dl;
    }
}

// out = T((float(cond) + a_low * d_low) + a_high * d_high): 8 elements per thread, the last n % 8 by one thread
template <typename T>
__global__ __launch_bounds__(kThreads) void fastercache_apply_kernel(const uint16_t* cond, const float* d_low, const float* d_high,
                                                                     float a_low, float a_high, uint16_t* out, int64_t n) {
    const int64_t nvec = n / 8, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nvec; i += stride) {
        float fc[8], lo[8], hi[8], fo[8];
        unpack8<T>(((const uint4*)cond)[i], fc);
        Plane<F32>::load(d_low, i * 8, lo);
        Plane<F32>::load(d_high, i * 8, hi);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float t0 = a_low * lo[e], t1 = a_high * hi[e];
            fo[e] = (fc[e] + t0) + t1;
        }
        ((uint4*)out)[i] = pack8<T>(fo);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int64_t j = nvec * 8; j < n; ++j) {
            const float t0 = a_low * d_low[j], t1 = a_high * d_high[j];
            out[j] = T::from_f32((T::to_f32(cond[j]) + t0) + t1);
        }
    }
}

// the half disk of radius r: row widths and first bins; -> the number of bins
int fc_disk(int r, FcDisk& disk) {
    int n = 0;
    for (int fy = 0; fy <= r; ++fy) {
        int w = 0;
        while ((w + 1) * (w + 1) + fy * fy <= r * r) ++w;
        disk.off[fy] = n;
        disk.w[fy] = w;
        n += fy == 0 ? w + 1 : 2 * w + 1;
    }
    disk.off[r + 1] = n;
    return n;
}

// the factor planes of a TaylorSeer call: [n planes][rows][dim] of dtype fdtype, 16-byte aligned rows, planes that do not overlap
bool planes_ok(const void* fac, int64_t plane, int64_t ldf, int fdtype, int n, int64_t rows, int64_t dim) {
    const int per16 = fino_per16(fdtype);
    if (!fac || !fino_aligned16(fac) || ldf < dim || ldf % per16 != 0) return false;
    return n <= 1 || (plane % per16 == 0 && (rows == 0 || plane >= (rows - 1) * ldf + dim));
}

// rows x dim walked in 16-byte vectors of per16 elements, fewer than 2^31 of them
int check_rows_dim(const char* who, int64_t rows, int64_t dim, int per16) {
    FINO_CHECK(rows >= 0 && dim > 0 && dim % per16 == 0 && rows * (dim / per16) < (1LL << 31), FINO_ERR_ARG,
               "%s: rows=%lld dim=%lld", who, (long long)rows, (long long)dim);
    return FINO_OK;
}

// the element dtype (two) and, inside it, the factor dtype (three): launch(T{}, F{})
template <typename L>
void taylor_dispatch(int dtype, int fdtype, L&& launch) {
    fino_dispatch_dtype(dtype, [&](auto t) { fino_dispatch_dtype3<F32>(fdtype, [&](auto f) { launch(t, f); }); });
}

}  // namespace

extern "C" int fino_step_cache_probe(const FinoStepCacheSegment* segs, int nseg, int64_t dim, float* sums, float* workspace,
                                     int dtype, void* stream) {
    const char* who = "fino_step_cache_probe";
    FINO_TRY(fino_check_dtype3(who, dtype));
    FINO_CHECK(segs && nseg >= 1 && nseg <= FINO_STEP_CACHE_MAX_SEGMENTS, FINO_ERR_ARG,
               "fino_step_cache_probe: %d segments (1 .. %d)", nseg, FINO_STEP_CACHE_MAX_SEGMENTS);
    FINO_CHECK(sums && workspace && fino_aligned16(sums) && fino_aligned16(workspace), FINO_ERR_ARG,
               "fino_step_cache_probe: sums / workspace missing or not 16-byte aligned");
    const int per16 = fino_per16(dtype);
    FINO_CHECK(dim > 0 && dim % per16 == 0, FINO_ERR_ARG, "fino_step_cache_probe: dim=%lld must be a multiple of %d",
               (long long)dim, per16);
    ProbeArgs args = {};
    args.vpr = (uint32_t)(dim / per16);
    for (int s = 0; s < nseg; ++s) {
        const FinoStepCacheSegment& g = segs[s];
        FINO_CHECK(g.h0 && g.h1 && g.r, FINO_ERR_ARG, "fino_step_cache_probe: segment %d: null h0 / h1 / r", s);
        FINO_CHECK(g.rows >= 0 && (g.rows + FINO_STEP_CACHE_BLOCKS - 1) / FINO_STEP_CACHE_BLOCKS * (dim / per16) < (1LL << 31),
                   FINO_ERR_ARG, "fino_step_cache_probe: segment %d: rows=%lld out of range", s, (long long)g.rows);
        FINO_CHECK(g.ld_h0 >= dim && g.ld_h1 >= dim && g.ld_r >= dim && (!g.p || g.ld_p >= dim) &&
                       (!g.h1_copy || g.ld_h1_copy >= dim),
                   FINO_ERR_ARG, "fino_step_cache_probe: segment %d: a row stride is below dim", s);
        FINO_CHECK(fino_rows_ok(g.h0, g.ld_h0, per16) && fino_rows_ok(g.h1, g.ld_h1, per16) && fino_rows_ok(g.r, g.ld_r, per16) &&
                       (!g.p || fino_rows_ok(g.p, g.ld_p, per16)) && (!g.h1_copy || fino_rows_ok(g.h1_copy, g.ld_h1_copy, per16)),
                   FINO_ERR_ARG, "fino_step_cache_probe: segment %d: 16-byte alignment required", s);
        args.seg[s] = g;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(FINO_STEP_CACHE_BLOCKS, nseg);
    fino_dispatch_dtype3<F32>(dtype, [&](auto t) { probe_kernel<decltype(t)><<<grid, kThreads, 0, st>>>(args, workspace); });
    FINO_TRY(fino_launch_check(who));
    probe_finish_kernel<<<nseg, kThreads, 0, st>>>(workspace, sums);
    return fino_launch_check(who);
}

extern "C" int fino_step_cache_residual(const void* a, int64_t lda, const void* b, int64_t ldb, void* out, int64_t ldo,
                                        int64_t rows, int64_t dim, int subtract, int dtype, void* stream) {
    const char* who = "fino_step_cache_residual";
    FINO_TRY(fino_check_dtype3(who, dtype));
    const int per16 = fino_per16(dtype);
    FINO_TRY(check_rows_dim(who, rows, dim, per16));
    FINO_CHECK(a && b && out, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_TRY(fino_check_strides(who, dim, {lda, ldb, ldo}));
    FINO_TRY(fino_check_aligned16(who, per16, {{a, lda}, {b, ldb}, {out, ldo}}));
    if (rows == 0) return FINO_OK;
    const uint32_t vpr = (uint32_t)(dim / per16), nvec = (uint32_t)(rows * vpr);
    const unsigned grid = fino_grid_1d(nvec, kFinoGridCap8, false, kThreads);
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype3<F32>(dtype, [&](auto t) {
        residual_kernel<decltype(t)><<<grid, kThreads, 0, st>>>(a, lda, b, ldb, out, ldo, vpr, nvec, subtract);
    });
    return fino_launch_check(who);
}

extern "C" int64_t fino_magcache_workspace_bytes(int64_t rows) {
    return rows < 1 ? 0 : magcache_waves(rows) * 2 * (int64_t)sizeof(double);
}

extern "C" int fino_magcache_calibrate(const void* x_out, int64_t ld_out, const void* x_in, int64_t ld_in, const void* r_prev,
                                       int64_t ld_prev, void* r_new, int64_t ld_new, int64_t rows, int64_t dim, int dtype,
                                       double* stats, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "fino_magcache_calibrate";
    FINO_TRY(fino_check_dtype3(who, dtype));
    const int per16 = fino_per16(dtype);
    FINO_CHECK(rows >= 1 && rows < (1LL << 31), FINO_ERR_ARG, "fino_magcache_calibrate: rows=%lld (1 .. 2^31 - 1)",
               (long long)rows);
    FINO_CHECK(dim > 0 && dim % per16 == 0 && dim / per16 < (1LL << 31), FINO_ERR_ARG,
               "fino_magcache_calibrate: dim=%lld must be a multiple of %d", (long long)dim, per16);
    FINO_CHECK(x_out && x_in && r_prev && r_new && stats && workspace, FINO_ERR_ARG, "fino_magcache_calibrate: null pointer");
    FINO_TRY(fino_check_strides(who, dim, {ld_out, ld_in, ld_prev, ld_new}));
    FINO_TRY(fino_check_aligned16(who, per16, {{x_out, ld_out}, {x_in, ld_in}, {r_prev, ld_prev}, {r_new, ld_new}, {stats, 0},
                                               {workspace, 0}}));
    FINO_CHECK(r_new != r_prev || ld_new == ld_prev, FINO_ERR_ARG,
               "fino_magcache_calibrate: r_new aliases r_prev with another row stride (%lld / %lld)", (long long)ld_new,
               (long long)ld_prev);
    const int64_t nwaves = magcache_waves(rows);
    FINO_CHECK(workspace_bytes >= fino_magcache_workspace_bytes(rows), FINO_ERR_ARG,
               "fino_magcache_calibrate: workspace of %lld bytes, need %lld (fino_magcache_workspace_bytes)",
               (long long)workspace_bytes, (long long)fino_magcache_workspace_bytes(rows));
    const uint32_t vpr = (uint32_t)(dim / per16);
    const int grid = (int)(nwaves / kMagWavesPerBlock);
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)workspace;
    fino_dispatch_dtype3<F32>(dtype, [&](auto t) {
        magcache_kernel<decltype(t)><<<grid, kThreads, 0, st>>>(x_out, ld_out, x_in, ld_in, r_prev, ld_prev, r_new, ld_new, rows,
                                                                vpr, partial);
    });
    FINO_TRY(fino_launch_check(who));
    magcache_finish_kernel<<<1, kThreads, 0, st>>>(partial, nwaves, (double)rows, stats);
    return fino_launch_check(who);
}

extern "C" int fino_pab_broadcast(const void* x, int64_t ldx, const void* y, int64_t ldy, void* out, int64_t ldo, int64_t rows,
                                  int64_t dim, const float* gate, int64_t mod_stride, const int32_t* sel, int dtype,
                                  void* stream) {
    const char* who = "fino_pab_broadcast";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_TRY(check_rows_dim(who, rows, dim, 8));
    FINO_CHECK(x && y && out, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_TRY(fino_check_strides(who, dim, {ldx, ldy, ldo}));
    const bool gate_ok = !gate || (fino_aligned16(gate) && mod_stride % 4 == 0);      // (a gate row stride counts only with a gate)
    FINO_TRY(fino_check_aligned16(who, 8, {{x, ldx}, {y, ldy}, {out, ldo}}, gate_ok));
    if (rows == 0) return FINO_OK;
    const uint32_t vpr = (uint32_t)(dim / 8), nvec = (uint32_t)(rows * vpr);
    const unsigned grid = fino_grid_1d(nvec, kFinoGridCap8, false, kThreads);
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        pab_broadcast_kernel<decltype(t)><<<grid, kThreads, 0, st>>>(x, ldx, y, ldy, out, ldo, vpr, nvec, gate, mod_stride, sel);
    });
    return fino_launch_check(who);
}

extern "C" int fino_taylor_update(const void* y, int64_t ldy, void* factors, int64_t plane_stride, int64_t ldf, int64_t rows,
                                  int64_t dim, int n_old, int n_new, int delta, int dtype, int fdtype, void* stream) {
    const char* who = "fino_taylor_update";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(fdtype == FINO_BF16 || fdtype == FINO_F16 || fdtype == FINO_F32, FINO_ERR_ARG, "fino_taylor_update: factor dtype %d",
               fdtype);
    FINO_TRY(check_rows_dim(who, rows, dim, 8));
    FINO_CHECK(n_old >= 0 && n_old <= FINO_TAYLOR_MAX_PLANES && n_new >= 1 && n_new <= FINO_TAYLOR_MAX_PLANES && n_new <= n_old + 1,
               FINO_ERR_ARG, "fino_taylor_update: n_old=%d n_new=%d (n_new in 1 .. %d, at most n_old + 1)", n_old, n_new,
               FINO_TAYLOR_MAX_PLANES);
    FINO_CHECK(delta >= 1 || n_new == 1, FINO_ERR_ARG, "fino_taylor_update: delta=%d must be at least 1", delta);
    FINO_CHECK(y && ldy >= dim, FINO_ERR_ARG, "fino_taylor_update: y missing or its row stride below dim");
    FINO_CHECK(fino_rows_ok(y, ldy, 8) && planes_ok(factors, plane_stride, ldf, fdtype, n_new, rows, dim), FINO_ERR_ARG,
               "fino_taylor_update: 16-byte aligned rows, row strides of at least dim and planes that do not overlap required");
    if (rows == 0) return FINO_OK;
    const uint32_t vpr = (uint32_t)(dim / 8), nvec = (uint32_t)(rows * vpr);
    const unsigned grid = fino_grid_1d(nvec, kFinoGridCap8, false, kThreads);
    hipStream_t st = (hipStream_t)stream;
    taylor_dispatch(dtype, fdtype, [&](auto t, auto f) {
        taylor_update_kernel<decltype(t), decltype(f)><<<grid, kThreads, 0, st>>>(y, ldy, factors, plane_stride, ldf, vpr, nvec,
                                                                                  n_new, (float)delta);
    });
    return fino_launch_check(who);
}

extern "C" int fino_taylor_predict(const void* factors, int64_t plane_stride, int64_t ldf, int n, const float* coef, const void* x,
                                   int64_t ldx, void* out, int64_t ldo, int64_t rows, int64_t dim, const float* gate,
                                   int64_t mod_stride, const int32_t* sel, int dtype, int fdtype, void* stream) {
    const char* who = "fino_taylor_predict";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(fdtype == FINO_BF16 || fdtype == FINO_F16 || fdtype == FINO_F32, FINO_ERR_ARG, "fino_taylor_predict: factor dtype %d",
               fdtype);
    FINO_TRY(check_rows_dim(who, rows, dim, 8));
    FINO_CHECK(n >= 1 && n <= FINO_TAYLOR_MAX_PLANES && coef, FINO_ERR_ARG, "fino_taylor_predict: n=%d planes (1 .. %d) with n "
               "host coefficients", n, FINO_TAYLOR_MAX_PLANES);
    FINO_CHECK(out && ldo >= dim && (!x || ldx >= dim), FINO_ERR_ARG, "fino_taylor_predict: out missing or a row stride below dim");
    FINO_CHECK(x || !gate, FINO_ERR_ARG, "fino_taylor_predict: a gate needs x");
    FINO_CHECK(planes_ok(factors, plane_stride, ldf, fdtype, n, rows, dim) && fino_rows_ok(out, ldo, 8) &&
                   (!x || fino_rows_ok(x, ldx, 8)) && (!gate || (fino_aligned16(gate) && mod_stride % 4 == 0)),
               FINO_ERR_ARG,
               "fino_taylor_predict: 16-byte aligned rows, row strides of at least dim and planes that do not overlap required");
    if (rows == 0) return FINO_OK;
    TaylorCoef c = {};
    for (int i = 0; i < n; ++i) c.c[i] = coef[i];
    const uint32_t vpr = (uint32_t)(dim / 8), nvec = (uint32_t)(rows * vpr);
    const unsigned grid = fino_grid_1d(nvec, kFinoGridCap8, false, kThreads);
    hipStream_t st = (hipStream_t)stream;
    taylor_dispatch(dtype, fdtype, [&](auto t, auto f) {
        taylor_predict_kernel<decltype(t), decltype(f)><<<grid, kThreads, 0, st>>>(factors, plane_stride, ldf, n, c, x, ldx, out, ldo,
                                                                                   vpr, nvec, gate, mod_stride, sel);
    });
    return fino_launch_check(who);
}

extern "C" int fino_fastercache_supported(int64_t planes, int64_t height, int64_t width) {
    return planes >= 1 && height >= 1 && width >= 1 && height <= FINO_FASTERCACHE_MAX_PLANE && width <= FINO_FASTERCACHE_MAX_PLANE &&
           height * width <= FINO_FASTERCACHE_MAX_PLANE;
}

extern "C" int fino_fastercache_delta(const void* uncond, const void* cond, float* d_low, float* d_high, int64_t planes,
                                      int64_t height, int64_t width, int dtype, void* stream) {
    const char* who = "fino_fastercache_delta";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(uncond && cond && d_low && d_high, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_TRY(fino_check_aligned16(who, 8, {{uncond, 0}, {cond, 0}, {d_low, 0}, {d_high, 0}}));
    FINO_CHECK(fino_fastercache_supported(planes, height, width) && planes < (1LL << 31), FINO_ERR_UNSUPPORTED,
               "fino_fastercache_delta: planes=%lld height=%lld width=%lld (each at least 1, height * width at most %d)",
               (long long)planes, (long long)height, (long long)width, (int)FINO_FASTERCACHE_MAX_PLANE);
    const int H = (int)height, W = (int)width, r = (H < W ? H : W) / 5;
    FcDisk disk = {};
    const int nbins = fc_disk(r, disk);
    const size_t smem = sizeof(double) * ((r > 0 ? 2 * (size_t)(H + W) : 4) + 2 * (size_t)nbins) + sizeof(float) * (size_t)H * W +
                        sizeof(int) * (2 * kFcMaxRows + 1);
    constexpr int kMaxSmem = 144 * 1024;        // (the largest supported plane: 64 KiB of D, 53 KiB of tables, 17 KiB of bins)
    FINO_CHECK(r + 1 <= kFcMaxRows && smem <= (size_t)kMaxSmem, FINO_ERR_UNSUPPORTED,
               "fino_fastercache_delta: height=%d width=%d needs %zu bytes of LDS", H, W, smem);
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* u = (const uint16_t*)uncond;
    const uint16_t* c = (const uint16_t*)cond;
    return fino_dispatch_dtype(dtype, [&](auto t) -> int {
        static FinoPerDeviceOnce once;        // one per instantiation: the LDS limit is raised per kernel (and per device)
        FINO_TRY(fino_max_smem_once(once, (const void*)fastercache_delta_kernel<decltype(t)>, kMaxSmem, who));
        fastercache_delta_kernel<decltype(t)><<<(int)planes, kFcThreads, smem, st>>>(u, c, d_low, d_high, H, W, r, nbins, disk);
        return fino_launch_check(who);
    });
}

extern "C" int fino_fastercache_apply(const void* cond, const float* d_low, const float* d_high, float a_low, float a_high,
                                      void* out, int64_t n, int dtype, void* stream) {
    const char* who = "fino_fastercache_apply";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(cond && d_low && d_high && out, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_TRY(fino_check_aligned16(who, 8, {{cond, 0}, {d_low, 0}, {d_high, 0}, {out, 0}}));
    FINO_CHECK(n >= 1, FINO_ERR_ARG, "fino_fastercache_apply: n=%lld must be at least 1", (long long)n);
    const unsigned grid = fino_grid_1d(n / 8, kFinoGridCap8, true, kThreads);
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        fastercache_apply_kernel<decltype(t)><<<grid, kThreads, 0, st>>>((const uint16_t*)cond, d_low, d_high, a_low, a_high,
                                                                         (uint16_t*)out, n);
    });
    return fino_launch_check(who);
}
