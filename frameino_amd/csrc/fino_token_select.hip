// Region-adaptive sampling (frameino_amd/step_cache.py): the kernels that make the list of active token
// rows of a partial forward and move whole rows by it.
//
//   fino_token_score   one wave per token row: the population standard deviation of the row's kept prediction, averaged over
//                      the batch elements of the call, times exp(starvation_scale * sit-out counter)
//   fino_token_select  ONE workgroup: the k largest scores (ties to the lower index) as an ascending int32 list, counters moved on
//   fino_gather_rows / fino_scatter_rows   whole-row copies by an int32 list
// (fino_qkv_rmsnorm_rope_rows, the per-layer kernel of a partial forward, sits beside the arithmetic it repeats bit for bit, in
// fino_elementwise.hip.)
//
// No atomics anywhere, every sum in a fixed order: each kernel is bit-reproducible across launches.  Every index read from a
// list is clamped into [0, n): a bad list gives a wrong answer, never an access outside the indexed buffer.  Built with
// -ffp-contract=off like the other step-cache kernels.
#include <math.h>

#include "fino_common.h"
#include "fino_host.h"

namespace {

constexpr int kScoreWaves = 4;
constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelMaxN = 65536;

// ------------------------------------------------------------------------------------------------ fino_token_score
template <typename T>
__global__ __launch_bounds__(kScoreWaves * 64) void token_score_kernel(const uint16_t* __restrict__ po, int64_t rows, int cols,
                                                                       int64_t ld, int batch,
                                                                       const int32_t* __restrict__ counters, float scale,
                                                                       const uint8_t* __restrict__ eligible,
                                                                       float* __restrict__ score) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kScoreWaves + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int e = eligible ? (int)eligible[row] : 1;
    float acc = 0.f;
    for (int bi = 0; bi < batch; ++bi) {                     // the batch elements in index order
        const uint16_t* p = po + ((int64_t)bi * rows + row) * ld;
        float s = 0.f;
        for (int c = lane; c < cols; c += 64) s += T::to_f32(p[c]);
        const float mean = wave_sum(s) / (float)cols;
        float q = 0.f;
        for (int c = lane; c < cols; c += 64) {
            const float d = T::to_f32(p[c]) - mean;
            q += d * d;
        }
        acc += sqrtf(wave_sum(q) / (float)cols);
    }
    if (lane != 0) return;
    float v = acc / (float)batch;
    if (counters) v *= expf(scale * (float)counters[row]);
    if (e == 0) v = -INFINITY;
    else if (e == 2) v = INFINITY;
    score[row] = v;
}

// ------------------------------------------------------------------------------------------------ fino_token_select
// fp32 -> a key that orders as the floats do (larger score = larger key); -0 is +0, a NaN ranks with -inf
__device__ __forceinline__ uint32_t score_key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) u = 0xff800000u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// exclusive prefix sum of one int per thread over the workgroup, in thread order; `total` = the sum over all threads
__device__ __forceinline__ int block_exclusive_scan(int v, int* __restrict__ wave_tot, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    __syncthreads();                                         // (wave_tot may still be read from the previous scan)
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kSelWaves; ++w) {
        const int t = wave_tot[w];
        if (w < wave) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

__global__ __launch_bounds__(kSelThreads) void token_select_kernel(const float* __restrict__ score, int n, int k,
                                                                   int32_t* __restrict__ idx_out,
                                                                   int32_t* __restrict__ counters) {
    __shared__ int hist[kSelWaves][16];
    __shared__ int wave_tot[kSelWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 1. the threshold: the k-th largest key, 4 bits at a time from the top.  Every thread counts the 16 digits of the keys
    //    that match the prefix so far, the counts are summed over the workgroup (shuffles, then a [waves][16] table), and
    //    every thread walks the 16 totals from the top: all threads hold the same prefix, nothing is broadcast.
    uint32_t prefix = 0, mask = 0;
    int want = k;                                            // how many of the keys that match the prefix are still wanted
    for (int shift = 28; shift >= 0; shift -= 4) {
        int cnt[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) cnt[j] = 0;
        for (int i = tid; i < n; i += kSelThreads) {
            const uint32_t key = score_key(score[i]);
            if ((key & mask) == prefix) {
                const int dgt = (int)((key >> shift) & 15u);
#pragma unroll
                for (int j = 0; j < 16; ++j) cnt[j] += (dgt == j) ? 1 : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int t = wave_sum_i(cnt[j]);
            if (lane == 0) hist[wave][j] = t;
        }
        __syncthreads();
        int digit = 0;
        bool found = false;
        for (int j = 15; j >= 0; --j) {
            int t = 0;
            for (int w = 0; w < kSelWaves; ++w) t += hist[w][j];
            if (!found) {
                if (t >= want) {
                    digit = j;
                    found = true;
                } else {
                    want -= t;
                }
            }
        }
        __syncthreads();                                     // (hist is rewritten by the next pass)
        prefix |= (uint32_t)digit << shift;
        mask |= 15u << shift;
    }
    // prefix = the threshold key; `want` of the keys equal to it are taken, the lowest indices first

    // 2. ordered compaction: thread t owns the indices [t * chunk, (t + 1) * chunk)
    const int chunk = (n + kSelThreads - 1) / kSelThreads;
    const int i0 = tid * chunk, i1 = min(n, i0 + chunk);
    int gt = 0, eq = 0;
    for (int i = i0; i < i1; ++i) {
        const uint32_t key = score_key(score[i]);
        gt += key > prefix ? 1 : 0;
        eq += key == prefix ? 1 : 0;
    }
    int tot_gt, tot_eq;
    const int gt_before = block_exclusive_scan(gt, wave_tot, tot_gt);
    const int eq_before = block_exclusive_scan(eq, wave_tot, tot_eq);
    int eq_rank = eq_before;
    int pos = gt_before + min(eq_before, want);
    for (int i = i0; i < i1; ++i) {
        const uint32_t key = score_key(score[i]);
        bool take = key > prefix;
        if (key == prefix) {
            take = eq_rank < want;
            ++eq_rank;
        }
        if (take) {
            if (pos < k) idx_out[pos] = i;
            ++pos;
        }
        if (counters) counters[i] = take ? 0 : counters[i] + 1;
    }
}

// ------------------------------------------------------------------------------------------------ gather / scatter
// one workgroup per listed row; U = the copy unit (uint4: 16 bytes, uint32_t: 4 bytes).  GATHER: dst[r] = src[idx[r]];
// else dst[idx[r]] = src[r].  n = the rows of the indexed side.
template <typename U, bool GATHER>
__global__ __launch_bounds__(256) void move_rows_kernel(const char* __restrict__ src, int64_t ld_src, const int32_t* __restrict__ idx,
                                                        int64_t k, int64_t n, int units, char* __restrict__ dst, int64_t ld_dst) {
    for (int64_t r = blockIdx.x; r < k; r += gridDim.x) {
        int64_t i = idx[r];
        i = i < 0 ? 0 : (i >= n ? n - 1 : i);
        const U* s = reinterpret_cast<const U*>(src + (GATHER ? i : r) * ld_src);
        U* d = reinterpret_cast<U*>(dst + (GATHER ? r : i) * ld_dst);
        for (int u = threadIdx.x; u < units; u += 256) d[u] = s[u];
    }
}

// fino_gather_rows / fino_scatter_rows (`who`); the copy unit and the direction reach the kernel as tags
int move_rows(const char* who, bool gather, const void* src, int64_t ld_src, const int32_t* idx, int64_t k, int64_t n,
              int64_t row_bytes, void* dst, int64_t ld_dst, void* stream) {
    FINO_CHECK(src && idx && dst, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_CHECK(k >= 0 && k < (1LL << 31) && n >= 1 && n < (1LL << 31), FINO_ERR_ARG, "%s: k=%lld n=%lld", who, (long long)k,
               (long long)n);
    FINO_CHECK(row_bytes >= 4 && row_bytes % 4 == 0 && row_bytes < (1LL << 31), FINO_ERR_ARG,
               "%s: row_bytes=%lld must be a positive multiple of 4", who, (long long)row_bytes);
    FINO_CHECK(ld_src >= row_bytes && ld_dst >= row_bytes, FINO_ERR_ARG, "%s: a row stride is below row_bytes", who);
    FINO_CHECK(ld_src % 4 == 0 && ld_dst % 4 == 0 && ((uintptr_t)src & 3u) == 0 && ((uintptr_t)dst & 3u) == 0, FINO_ERR_ARG,
               "%s: 4-byte alignment required", who);
    if (k == 0) return FINO_OK;
    const bool v16 = row_bytes % 16 == 0 && ld_src % 16 == 0 && ld_dst % 16 == 0 && fino_aligned16(src) && fino_aligned16(dst);
    const unsigned grid = (unsigned)(k < 65536 ? k : 65536);
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](auto unit, auto dir) {
        using U = decltype(unit);
        move_rows_kernel<U, decltype(dir)::value><<<grid, 256, 0, st>>>((const char*)src, ld_src, idx, k, n,
                                                                        (int)(row_bytes / (int64_t)sizeof(U)), (char*)dst, ld_dst);
    };
    auto by_direction = [&](auto unit) { gather ? launch(unit, std::true_type{}) : launch(unit, std::false_type{}); };
    v16 ? by_direction(uint4{}) : by_direction(uint32_t{});
    return fino_launch_check(who);
}

}  // namespace

extern "C" int fino_token_score(const void* po, int64_t rows, int cols, int64_t ld, int batch, const int32_t* counters,
                                float starvation_scale, const uint8_t* eligible, float* score_out, int dtype, void* stream) {
    const char* who = "fino_token_score";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(po && score_out, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_CHECK(rows >= 1 && rows < (1LL << 31) && cols >= 1 && ld >= cols && batch >= 1 && batch <= 64, FINO_ERR_ARG,
               "fino_token_score: rows=%lld cols=%d ld=%lld batch=%d", (long long)rows, cols, (long long)ld, batch);
    const dim3 grid((unsigned)((rows + kScoreWaves - 1) / kScoreWaves)), block(kScoreWaves * 64);
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        token_score_kernel<decltype(t)><<<grid, block, 0, st>>>((const uint16_t*)po, rows, cols, ld, batch, counters,
                                                                starvation_scale, eligible, score_out);
    });
    return fino_launch_check(who);
}

extern "C" int fino_token_select(const float* score, int64_t n, int64_t k, int32_t* idx_out, int32_t* counters, void* stream) {
    FINO_CHECK(score && idx_out, FINO_ERR_ARG, "fino_token_select: null pointer");
    FINO_CHECK(n >= 1 && k >= 1 && k <= n, FINO_ERR_ARG, "fino_token_select: n=%lld k=%lld (1 <= k <= n)", (long long)n,
               (long long)k);
    FINO_CHECK(n <= kSelMaxN, FINO_ERR_UNSUPPORTED, "fino_token_select: n=%lld above %d (one workgroup selects)", (long long)n,
               kSelMaxN);
    token_select_kernel<<<1, kSelThreads, 0, (hipStream_t)stream>>>(score, (int)n, (int)k, idx_out, counters);
    return fino_launch_check("fino_token_select");
}

extern "C" int fino_gather_rows(const void* src, int64_t ld_src, int64_t n, const int32_t* idx, int64_t k, int64_t row_bytes,
                                void* dst, int64_t ld_dst, void* stream) {
    return move_rows("fino_gather_rows", true, src, ld_src, idx, k, n, row_bytes, dst, ld_dst, stream);
}

extern "C" int fino_scatter_rows(const void* src, int64_t ld_src, const int32_t* idx, int64_t k, int64_t row_bytes, void* dst,
                                 int64_t ld_dst, int64_t n, void* stream) {
    return move_rows("fino_scatter_rows", false, src, ld_src, idx, k, n, row_bytes, dst, ld_dst, stream);
}
