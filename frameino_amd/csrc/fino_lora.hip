// fino_lora_merge: W_out = round( float(W_base) + sum_a s_a * (B_a . A_a) ) for one linear weight (LoRA merge on the GPU).
//
// bf16 / fp16 weights: the rank product runs on the MFMA pipe (v_mfma_f32_32x32x16_{bf16,f16}, rank in chunks of 16 with a
// zero-filled tail), fp32 accumulation, s_a applied to each adapter's fp32 partial product, ONE rounding (RNE) at the end.
// HBM-bound: W is read and written once with 16-byte accesses; A and B are small and come from L2.
//
// Orientation: the MFMA computes delta^T tiles, D[i][c] = sum_j A[j][k(i)] * B[n = c][j], so that the accumulator's column
// (the lane) is the weight ROW n and its 16 registers are 16 CONTIGUOUS columns k of that row: the MFMA row index i is mapped to
// column k(i) = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3), which turns the 32x32 C layout (row = (g & 3) + 8 (g >> 2) +
// 4 (lane >> 5)) into k = 16 (lane >> 5) + g.  A lane then reads / writes its 16 weights as two 16-byte vectors.
//
// Grid: x = 64-column strips of K, y = segments of N-tiles.  A workgroup (4 waves) stages A^T of its strip, every adapter,
// in LDS once ([chunk][k 0..63][16 ranks], zero outside the rank / K) and walks its N-tiles of 128 rows (32 per wave).
#include "fino_common.h"
#include "fino_host.h"

namespace {

constexpr int kTK = 64;                 // columns per strip (two 32-column MFMA tiles per wave)
constexpr int kWaves = 4;
constexpr int kTN = 32 * kWaves;        // rows per N-tile

struct LoraArgs {
    const void* a[FINO_LORA_MAX_ADAPTERS];
    const void* b[FINO_LORA_MAX_ADAPTERS];
    int64_t lda[FINO_LORA_MAX_ADAPTERS];
    int64_t ldb[FINO_LORA_MAX_ADAPTERS];
    int rank[FINO_LORA_MAX_ADAPTERS];
    int chunk0[FINO_LORA_MAX_ADAPTERS];  // first 16-rank chunk of adapter a in the LDS image
    float scale[FINO_LORA_MAX_ADAPTERS];
    int n_adapters;
    int b_vec;                           // every B pointer 16-byte aligned and every ldb % 8 == 0
};

__device__ __forceinline__ int kperm(int r) { return 16 * ((r >> 2) & 1) + 4 * (r >> 3) + (r & 3); }

template <typename T>
__global__ __launch_bounds__(256) void lora_merge_mfma(const uint16_t* wb, int64_t ldwb, uint16_t* wo,
                                                       int64_t ldwo, int64_t N, int64_t K, LoraArgs args, int tiles_per_seg,
                                                       int w_vec) {
    extern __shared__ __align__(16) uint16_t lds_at[];   // [chunks][kTK][16]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t k0 = (int64_t)blockIdx.x * kTK;

    // ---- stage A^T of the strip (every adapter) ----
    int chunks = 0;
    for (int a = 0; a < args.n_adapters; ++a) chunks += (args.rank[a] + 15) >> 4;
    for (int e = tid; e < chunks * 16 * kTK; e += 256) {
        const int k = e % kTK, jc = e / kTK;          // consecutive threads: consecutive k (coalesced reads of a row of A)
        const int c = jc >> 4, jj = jc & 15;
        int a = 0;
        while (a + 1 < args.n_adapters && c >= args.chunk0[a + 1]) ++a;
        const int j = (c - args.chunk0[a]) * 16 + jj;
        uint16_t v = 0;
        if (j < args.rank[a] && k0 + k < K) v = ((const uint16_t*)args.a[a])[(int64_t)j * args.lda[a] + k0 + k];
        lds_at[(c * kTK + k) * 16 + jj] = v;
    }
    __syncthreads();

    const int r = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (N + kTN - 1) / kTN;
    const int64_t t_begin = (int64_t)blockIdx.y * tiles_per_seg;
    const int64_t t_end = t_begin + tiles_per_seg < n_tiles ? t_begin + tiles_per_seg : n_tiles;
    for (int64_t t = t_begin; t < t_end; ++t) {
        const int64_t n = t * kTN + wave * 32 + r;       // this lane's weight row
        const bool row_ok = n < N;
        // ---- W: 2 tiles x 16 contiguous columns per lane, issued before the rank product ----
        float w[2][16];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int64_t kc = k0 + 32 * tt + 16 * h;
            if (w_vec && row_ok && kc + 16 <= K) {
                const uint4* p = (const uint4*)(wb + n * ldwb + kc);
                const uint4 v0 = p[0], v1 = p[1];
                float f[8];
                unpack8<T>(v0, f);
#pragma unroll
                for (int i = 0; i < 8; ++i) w[tt][i] = f[i];
                unpack8<T>(v1, f);
#pragma unroll
                for (int i = 0; i < 8; ++i) w[tt][8 + i] = f[i];
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    w[tt][i] = (row_ok && kc + i < K) ? T::to_f32(wb[n * ldwb + kc + i]) : 0.f;
            }
        }
        // ---- delta = sum_a s_a * (B_a . A_a) for the 32 x 64 block of this wave ----
        f32x16_t delta[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int i = 0; i < 16; ++i) delta[tt][i] = 0.f;
        for (int a = 0; a < args.n_adapters; ++a) {
            const uint16_t* bp = (const uint16_t*)args.b[a];
            const int rk = args.rank[a];
            f32x16_t acc[2];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[tt][i] = 0.f;
            for (int c = 0; c * 16 < rk; ++c) {
                const int j0 = c * 16 + 8 * h;
                uint4 bv;
                if (args.b_vec && row_ok && j0 + 8 <= rk) {
                    bv = *(const uint4*)(bp + n * args.ldb[a] + j0);
                } else {
                    uint16_t s[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) s[i] = (row_ok && j0 + i < rk) ? bp[n * args.ldb[a] + j0 + i] : (uint16_t)0;
                    bv = make_uint4(s[0] | ((uint32_t)s[1] << 16), s[2] | ((uint32_t)s[3] << 16),
                                    s[4] | ((uint32_t)s[5] << 16), s[6] | ((uint32_t)s[7] << 16));
                }
                const typename T::vec8 bf = __builtin_bit_cast(typename T::vec8, bv);
                const int cg = args.chunk0[a] + c;
#pragma unroll
                for (int tt = 0; tt < 2; ++tt) {
                    const uint4 av = *(const uint4*)(lds_at + ((cg * kTK + 32 * tt + kperm(r)) * 16 + 8 * h));
                    acc[tt] = T::mfma32(__builtin_bit_cast(typename T::vec8, av), bf, acc[tt]);
                }
            }
            const float s = args.scale[a];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int i = 0; i < 16; ++i) delta[tt][i] += s * acc[tt][i];
        }
        // ---- W_out = round(W + delta): one rounding, vector stores ----
        if (!row_ok) continue;
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int64_t kc = k0 + 32 * tt + 16 * h;
            if (w_vec && kc + 16 <= K) {
                float f0[8], f1[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    f0[i] = w[tt][i] + delta[tt][i];
                    f1[i] = w[tt][8 + i] + delta[tt][8 + i];
                }
                uint4* p = (uint4*)(wo + n * ldwo + kc);
                p[0] = pack8<T>(f0);
                p[1] = pack8<T>(f1);
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (kc + i < K) wo[n * ldwo + kc + i] = T::from_f32(w[tt][i] + delta[tt][i]);
            }
        }
    }
}

// fp32 weights (the fp32-island targets, e.g. time_embedder): 4 contiguous columns per thread, plain FMA from L2.
__global__ __launch_bounds__(256) void lora_merge_f32(const float* wb, int64_t ldwb, float* wo, int64_t ldwo,
                                                      int64_t N, int64_t K, LoraArgs args, int w_vec) {
    const int64_t kq = (K + 3) / 4;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * kq) return;
    const int64_t n = idx / kq, k = (idx % kq) * 4;
    float delta[4] = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < args.n_adapters; ++a) {
        const float* A = (const float*)args.a[a];
        const float* B = (const float*)args.b[a];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < args.rank[a]; ++j) {
            const float bj = B[n * args.ldb[a] + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k + i < K) acc[i] = fmaf(bj, A[(int64_t)j * args.lda[a] + k + i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) delta[i] += args.scale[a] * acc[i];
    }
    if (w_vec && k + 4 <= K) {
        const float4 v = *(const float4*)(wb + n * ldwb + k);
        *(float4*)(wo + n * ldwo + k) = make_float4(v.x + delta[0], v.y + delta[1], v.z + delta[2], v.w + delta[3]);
    } else {
        for (int i = 0; i < 4 && k + i < K; ++i) wo[n * ldwo + k + i] = wb[n * ldwb + k + i] + delta[i];
    }
}

}  // namespace

extern "C" int fino_lora_merge(const void* w_base, int64_t ldw_base, void* w_out, int64_t ldw_out, int64_t n, int64_t k,
                               int n_adapters, const void* const* a, const int64_t* lda, const void* const* b,
                               const int64_t* ldb, const int* rank, const float* scale, int dtype, void* stream) {
    const char* who = "fino_lora_merge";
    FINO_CHECK(dtype == FINO_BF16 || dtype == FINO_F16 || dtype == FINO_F32, FINO_ERR_ARG,
               "fino_lora_merge: dtype %d is not FINO_BF16 / FINO_F16 / FINO_F32", dtype);
    FINO_CHECK(n >= 0 && k >= 0, FINO_ERR_ARG, "fino_lora_merge: negative shape n=%lld k=%lld", (long long)n, (long long)k);
    FINO_CHECK(n_adapters >= 0 && n_adapters <= FINO_LORA_MAX_ADAPTERS, FINO_ERR_ARG,
               "fino_lora_merge: n_adapters = %d (0 .. %d per call)", n_adapters, FINO_LORA_MAX_ADAPTERS);
    FINO_CHECK(ldw_base >= k && ldw_out >= k, FINO_ERR_ARG, "fino_lora_merge: leading dimension < k (ldw_base=%lld ldw_out=%lld k=%lld)",
               (long long)ldw_base, (long long)ldw_out, (long long)k);
    if (n == 0 || k == 0) return FINO_OK;
    FINO_CHECK(w_base && w_out, FINO_ERR_ARG, "fino_lora_merge: null weight pointer");
    FINO_CHECK(n_adapters == 0 || (a && lda && b && ldb && rank && scale), FINO_ERR_ARG,
               "fino_lora_merge: null adapter array");
    LoraArgs args = {};
    args.n_adapters = n_adapters;
    args.b_vec = 1;
    int chunks = 0;
    for (int i = 0; i < n_adapters; ++i) {
        FINO_CHECK(a[i] && b[i], FINO_ERR_ARG, "fino_lora_merge: adapter %d has a null factor", i);
        FINO_CHECK(rank[i] >= 1, FINO_ERR_ARG, "fino_lora_merge: adapter %d has rank %d (>= 1)", i, rank[i]);
        FINO_CHECK(lda[i] >= k && ldb[i] >= rank[i], FINO_ERR_ARG,
                   "fino_lora_merge: adapter %d leading dimension too small (lda=%lld k=%lld, ldb=%lld rank=%d)", i,
                   (long long)lda[i], (long long)k, (long long)ldb[i], rank[i]);
        args.a[i] = a[i];
        args.b[i] = b[i];
        args.lda[i] = lda[i];
        args.ldb[i] = ldb[i];
        args.rank[i] = rank[i];
        args.scale[i] = scale[i];
        args.chunk0[i] = chunks;
        chunks += (rank[i] + 15) / 16;
        if (!fino_aligned16(b[i]) || ldb[i] % 8 != 0) args.b_vec = 0;
    }
    hipStream_t st = (hipStream_t)stream;
    if (dtype == FINO_F32) {
        const int w_vec = fino_aligned16(w_base) && fino_aligned16(w_out) && ldw_base % 4 == 0 && ldw_out % 4 == 0;
        const int64_t threads = n * ((k + 3) / 4);
        const int64_t blocks = (threads + 255) / 256;
        FINO_CHECK(blocks <= 0x7fffffff, FINO_ERR_UNSUPPORTED, "fino_lora_merge: fp32 weight too large (%lld x %lld)",
                   (long long)n, (long long)k);
        lora_merge_f32<<<(unsigned)blocks, 256, 0, st>>>((const float*)w_base, ldw_base, (float*)w_out, ldw_out, n, k, args, w_vec);
        return fino_launch_check(who);
    }
    FINO_CHECK(chunks * 16 <= FINO_LORA_MAX_TOTAL_RANK, FINO_ERR_UNSUPPORTED,
               "fino_lora_merge: total rank %d of one call exceeds %d (ranks are padded to 16)", chunks * 16,
               FINO_LORA_MAX_TOTAL_RANK);
    const int w_vec = fino_aligned16(w_base) && fino_aligned16(w_out) && ldw_base % 8 == 0 && ldw_out % 8 == 0;
    const int64_t strips = (k + kTK - 1) / kTK;
    const int64_t n_tiles = (n + kTN - 1) / kTN;
    FINO_CHECK(strips <= 0x7fffffff, FINO_ERR_UNSUPPORTED, "fino_lora_merge: k = %lld too large", (long long)k);
    // enough workgroups to fill the device (~8 per CU), each walking as many N-tiles as that leaves (A^T staged once)
    const int64_t want_segs = (2048 + strips - 1) / strips;
    const int64_t segs_req = want_segs < n_tiles ? want_segs : n_tiles;
    const int64_t tiles_per_seg = (n_tiles + segs_req - 1) / segs_req;
    const int64_t segs = (n_tiles + tiles_per_seg - 1) / tiles_per_seg;
    FINO_CHECK(segs <= 65535, FINO_ERR_UNSUPPORTED, "fino_lora_merge: n = %lld too large", (long long)n);
    const size_t lds = (size_t)chunks * kTK * 16 * sizeof(uint16_t);
    const dim3 grid((unsigned)strips, (unsigned)segs);
    return fino_dispatch_dtype(dtype, [&](auto t) -> int {
        using T = decltype(t);
        static FinoPerDeviceOnce once;        // one per instantiation: the LDS limit is raised per kernel (and per device)
        FINO_TRY(fino_max_smem_once(once, (const void*)lora_merge_mfma<T>, FINO_LORA_MAX_TOTAL_RANK * kTK * 2, who));
        lora_merge_mfma<T><<<grid, 256, lds, st>>>((const uint16_t*)w_base, ldw_base, (uint16_t*)w_out, ldw_out, n, k, args,
                                                   (int)tiles_per_seg, w_vec);
        return fino_launch_check(who);
    });
}
