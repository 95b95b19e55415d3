// Guiders of the two sampler loops (gfx950): CFG-Zero*, adaptive projected guidance (APG), guidance rescale.
//
// Every guider combines the conditional prediction c and the unconditional prediction u of one sample as v = A c + B u with two
// scalars that depend on five global moments of (c, u) over exactly the n elements the step kernel updates:
//     Sc = sum c, Su = sum u, Scc = sum c^2, Suu = sum u^2, Scu = sum c u         (elements of T read as fp32, sums in fp64)
// fino_guider_coefs is two launches and no host read, so a captured step replays it:
//   1. guider_moments_kernel: workgroup b takes the elements [b * kBlockElems, (b + 1) * kBlockElems) of the flattened sample
//      and writes its five sums to workspace[5 b .. 5 b + 4].  A thread adds its elements in index order, then the xor butterfly
//      of its wave, then the four waves in index order: a fixed order, no atomics, the same bits on every launch.
//   2. guider_finish_kernel, one workgroup: thread t adds the partials t, t + 256, ... in order, the same butterfly, and thread 0
//      evaluates the guider's formulas in fp64 (frameino_amd/guiders.py::coefficients is the same text) and stores {A, B} as fp32.
// The guidance scale g and the zero-init flag are read from device memory: the per-step value is a device copy, as the
// samplers' coefficient rows are.
//
// The sample is `rows` runs of `row_len` contiguous elements, `row_stride` apart:
//     Wan        pred [C, Fg + n_id, H, W], the Fg generated frames: rows = C, row_len = Fg H W, row_stride = (Fg + n_id) H W
//     CogVideoX  pred [2, batch_stride] (u first), the first n_lat of each: rows = 1, row_len = n_lat, uncond = pred,
//                cond = pred + batch_stride
// 16-byte loads (8 elements) when every run starts and ends on a 16-byte boundary, 2-byte loads otherwise; the tensors are
// 1-2 M elements (9 MB read per step), so the cost is the two launches, not the bytes.
//
// The fino_guided_*_step kernels are the fino_cfg_*_step bodies (fino_sampler_step.h) with v formed from {A, B}.
#include "fino_host.h"
#include "fino_sampler_step.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 8;                                             // elements of a 16-byte load
constexpr int kIters = 8;                                           // loads of a thread, all in flight before the first add
constexpr int64_t kBlockElems = (int64_t)kThreads * kVec * kIters;  // 16384 elements per workgroup
constexpr int kMoments = 5;

inline int64_t moment_blocks(int64_t n) { return (n + kBlockElems - 1) / kBlockElems; }

struct Moments {
    double v[kMoments];
    __device__ __forceinline__ void add(float fc, float fu) {
        const double c = (double)fc, u = (double)fu;
        v[0] += c;
        v[1] += u;
        v[2] += c * c;
        v[3] += u * u;
        v[4] += c * u;
    }
};

// wave butterfly, then the waves in index order; the sums are valid in thread 0
__device__ __forceinline__ void block_sum(Moments& m) {
    __shared__ double red[kMoments][kThreads / 64];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m.v[k] += __shfl_xor(m.v[k], o, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = m.v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) {
            double s = red[k][0];
#pragma unroll
            for (int w = 1; w < kThreads / 64; ++w) s += red[k][w];
            m.v[k] = s;
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void guider_moments_kernel(const uint16_t* __restrict__ pc,
                                                                  const uint16_t* __restrict__ pu, int64_t n,
                                                                  int64_t row_len, int64_t row_stride,
                                                                  double* __restrict__ partial) {
    Moments m = {};
    const int64_t base = (int64_t)blockIdx.x * kBlockElems;
    if constexpr (VEC) {
        // (row_len is a multiple of 8: a vector never straddles two runs, and n is a multiple of 8)
        uint4 vc[kIters], vu[kIters];
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const int64_t e = base + ((int64_t)k * kThreads + threadIdx.x) * kVec;
            if (e < n) {
                const int64_t off = (e / row_len) * row_stride + e % row_len;
                vc[k] = *(const uint4*)(pc + off);
                vu[k] = *(const uint4*)(pu + off);
            }
        }
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const int64_t e = base + ((int64_t)k * kThreads + threadIdx.x) * kVec;
            if (e < n) {
                float fc[kVec], fu[kVec];
                unpack8<T>(vc[k], fc);
                unpack8<T>(vu[k], fu);
#pragma unroll
                for (int j = 0; j < kVec; ++j) m.add(fc[j], fu[j]);
            }
        }
    } else {
        for (int k = 0; k < kIters * kVec; ++k) {
            const int64_t e = base + (int64_t)k * kThreads + threadIdx.x;
            if (e < n) {
                const int64_t off = (e / row_len) * row_stride + e % row_len;
                m.add(T::to_f32(pc[off]), T::to_f32(pu[off]));
            }
        }
    }
    block_sum(m);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) partial[(int64_t)blockIdx.x * kMoments + k] = m.v[k];
    }
}

struct GuiderParams {
    int kind;                // FINO_GUIDER_*
    double norm_threshold;   // APG
    double eta;              // APG
    double rescale;          // guidance rescale phi (0: off)
};

// the formulas of frameino_amd/guiders.py::coefficients, term by term, in fp64
__device__ void guider_formulas(const double (&s)[kMoments], double n, double g, bool zero_init, const GuiderParams& p,
                                float* __restrict__ ab) {
    const double Sc = s[0], Su = s[1], Scc = s[2], Suu = s[3], Scu = s[4];
    if (p.kind == FINO_GUIDER_ZERO_STAR && zero_init) {
        ab[0] = 0.f;
        ab[1] = 0.f;
        return;
    }
    double a0, b0;
    if (p.kind == FINO_GUIDER_ZERO_STAR) {
        const double st = Scu / (Suu + 1e-8);
        a0 = g;
        b0 = (1. - g) * st;
    } else if (p.kind == FINO_GUIDER_APG) {
        const double dd = Scc - 2. * Scu + Suu;
        double sc = 1.;
        if (p.norm_threshold > 0. && dd > 0.) sc = fmin(1., p.norm_threshold / sqrt(dd));
        const double par = Scc > 0. ? sc * (Scc - Scu) / Scc : 0.;
        a0 = g * (sc + (p.eta - 1.) * par);
        b0 = 1. - g * sc;
    } else {
        a0 = g;
        b0 = 1. - g;
    }
    double mlt = 1.;
    if (p.rescale > 0.) {
        double f = 1.;
        if (n >= 2.) {
            const double var_c = fmax((Scc - Sc * Sc / n) / (n - 1.), 0.);
            const double var_u = fmax((Suu - Su * Su / n) / (n - 1.), 0.);
            const double cov = (Scu - Sc * Su / n) / (n - 1.);
            const double var_p = a0 * a0 * var_c + b0 * b0 * var_u + 2. * a0 * b0 * cov;
            if (var_p > 0.) f = sqrt(var_c / var_p);
        }
        mlt = p.rescale * f + 1. - p.rescale;
    }
    ab[0] = (float)(mlt * a0);
    ab[1] = (float)(mlt * b0);
}

__global__ __launch_bounds__(kThreads) void guider_finish_kernel(const double* __restrict__ partial, int64_t nblocks,
                                                                 double n, const float* __restrict__ g_dev,
                                                                 const float* __restrict__ zero_dev, GuiderParams p,
                                                                 float* __restrict__ ab) {
    Moments m = {};
    for (int64_t j = threadIdx.x; j < nblocks; j += kThreads) {
#pragma unroll
        for (int k = 0; k < kMoments; ++k) m.v[k] += partial[j * kMoments + k];
    }
    block_sum(m);
    if (threadIdx.x == 0) guider_formulas(m.v, n, (double)*g_dev, zero_dev != nullptr && *zero_dev != 0.f, p, ab);
}

// ---- the guided steps: the sampler-step bodies with v = fl(fl(A c) + fl(B u)) --------------------------------
template <typename T>
__global__ __launch_bounds__(256) void guided_euler_kernel(const uint16_t* __restrict__ pc,
                                                           const uint16_t* __restrict__ pu, float* __restrict__ lat, int C,
                                                           int Fg, int Ft, int HW, const float* __restrict__ ab,
                                                           const float* __restrict__ dt_dev, int round_out) {
    const float a = ab[0], b = ab[1];
    const float dt = *dt_dev;
    const int64_t total = (int64_t)C * Fg * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x)
        euler_step_elem<T>(i, pc, pu, lat, Fg, Ft, HW, GuidedRounded<T>{a, b}, dt, round_out);
}

template <typename T>
__global__ __launch_bounds__(256) void guided_unipc_kernel(const uint16_t* __restrict__ pc,
                                                           const uint16_t* __restrict__ pu, float* __restrict__ x,
                                                           float* __restrict__ last, float* __restrict__ m0,
                                                           float* __restrict__ m1, int C, int Fg, int Ft, int HW,
                                                           const float* __restrict__ coef, const float* __restrict__ ab) {
    const float a = ab[0], b = ab[1];
    const float sigma = coef[1], use_corr = coef[2];
    const float Cx = coef[3], C0 = coef[4], C1 = coef[5], Ct = coef[6], Px = coef[7], P0 = coef[8], P1 = coef[9];
    const int64_t total = (int64_t)C * Fg * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x)
        unipc_step_elem<T>(i, pc, pu, x, last, m0, m1, Fg, Ft, HW, sigma, use_corr, Cx, C0, C1, Ct, Px, P0, P1,
                           GuidedRounded<T>{a, b});
}

template <typename T>
__global__ __launch_bounds__(256) void guided_vpred_kernel(const uint16_t* __restrict__ pred, uint16_t* __restrict__ lat,
                                                           int64_t n_lat, int64_t batch_stride,
                                                           const float* __restrict__ coef, const float* __restrict__ ab) {
    const float a = ab[0], b = ab[1];
    vpred_step_body<T>(pred, lat, n_lat, batch_stride, coef[0], coef[1], coef[2], coef[3], GuidedF32{a, b}, 1,
                       FINO_GRID_STRIDE());
}

template <typename T>
__global__ __launch_bounds__(256) void guided_dpm_kernel(const uint16_t* __restrict__ pred, uint16_t* __restrict__ lat,
                                                         float* __restrict__ x0_old, const uint16_t* __restrict__ noise,
                                                         int64_t n_lat, int64_t batch_stride,
                                                         const float* __restrict__ coef, const float* __restrict__ ab) {
    dpm_step_body<T, GuidedF32>(pred, lat, x0_old, noise, n_lat, batch_stride, coef, ab, 1, FINO_GRID_STRIDE());
}

constexpr int64_t kMaxElems = (int64_t)1 << 40;      // keeps the workgroup count of the moments launch below 2^31

}  // namespace

extern "C" int64_t fino_guider_workspace_bytes(int64_t n) {
    return n < 1 || n > kMaxElems ? 0 : moment_blocks(n) * kMoments * (int64_t)sizeof(double);
}

extern "C" int fino_guider_coefs(const void* cond_pred, const void* uncond_pred, int64_t rows, int64_t row_len,
                                 int64_t row_stride, int kind, double norm_threshold, double eta, double guidance_rescale,
                                 const float* g_dev, const float* zero_init_dev, void* workspace, int64_t workspace_bytes,
                                 float* ab_dev, int dtype, void* stream) {
    const char* who = "fino_guider_coefs";
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(kind == FINO_GUIDER_RESCALE || kind == FINO_GUIDER_ZERO_STAR || kind == FINO_GUIDER_APG, FINO_ERR_ARG,
               "fino_guider_coefs: kind %d", kind);
    FINO_CHECK(cond_pred && uncond_pred && g_dev && workspace && ab_dev, FINO_ERR_ARG, "fino_guider_coefs: null pointer");
    FINO_CHECK(rows >= 1 && row_len >= 1 && row_stride >= row_len && rows <= kMaxElems / row_len, FINO_ERR_ARG,
               "fino_guider_coefs: bad shape rows=%lld row_len=%lld row_stride=%lld", (long long)rows, (long long)row_len,
               (long long)row_stride);
    FINO_CHECK(guidance_rescale >= 0. && guidance_rescale <= 1. && eta == eta && norm_threshold == norm_threshold,
               FINO_ERR_ARG, "fino_guider_coefs: guidance_rescale=%g (0 .. 1), eta=%g, norm_threshold=%g", guidance_rescale,
               eta, norm_threshold);
    FINO_CHECK((((uintptr_t)workspace) & 7u) == 0, FINO_ERR_ARG, "fino_guider_coefs: the workspace must be 8-byte aligned");
    const int64_t n = rows * row_len;
    FINO_CHECK(workspace_bytes >= fino_guider_workspace_bytes(n), FINO_ERR_ARG,
               "fino_guider_coefs: workspace of %lld bytes, need %lld (fino_guider_workspace_bytes)",
               (long long)workspace_bytes, (long long)fino_guider_workspace_bytes(n));
    const int64_t nblocks = moment_blocks(n);
    const bool vec = row_len % kVec == 0 && (rows == 1 || row_stride % kVec == 0) && fino_aligned16(cond_pred) &&
                     fino_aligned16(uncond_pred);
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* pc = (const uint16_t*)cond_pred;
    const uint16_t* pu = (const uint16_t*)uncond_pred;
    double* partial = (double*)workspace;
    const unsigned grid = (unsigned)nblocks;
    fino_dispatch_dtype(dtype, [&](auto t) {
        auto launch = [&](auto v) {
            guider_moments_kernel<decltype(t), decltype(v)::value><<<grid, kThreads, 0, st>>>(pc, pu, n, row_len, row_stride,
                                                                                             partial);
        };
        vec ? launch(std::true_type{}) : launch(std::false_type{});
    });
    FINO_TRY(fino_launch_check(who));
    const GuiderParams p = {kind, norm_threshold, eta, guidance_rescale};
    guider_finish_kernel<<<1, kThreads, 0, st>>>(partial, nblocks, (double)n, g_dev, zero_init_dev, p, ab_dev);
    return fino_launch_check(who);
}

// The guided steps: the checks and the launch shape of the fino_cfg_*_step entry points (fino_host.h), with the pointers
// these kernels read
extern "C" int fino_guided_euler_step(const void* cond_pred, const void* uncond_pred, float* lat, int channels,
                                      int gen_frames, int total_frames, int height, int width, const float* ab_dev,
                                      const float* dt_dev, int round_out, int dtype, void* stream) {
    const char* who = "fino_guided_euler_step";
    FINO_TRY(fino_check_frames_step(who, dtype, cond_pred && uncond_pred && lat && ab_dev && dt_dev, channels, gen_frames,
                                    total_frames, height, width));
    const int64_t total = (int64_t)channels * gen_frames * height * width;
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        guided_euler_kernel<decltype(t)><<<fino_grid_1d(total, kFinoGridCap8, true), 256, 0, st>>>(
            (const uint16_t*)cond_pred, (const uint16_t*)uncond_pred, lat, channels, gen_frames, total_frames, height * width,
            ab_dev, dt_dev, round_out);
    });
    return fino_launch_check(who);
}

extern "C" int fino_guided_unipc_step(const void* cond_pred, const void* uncond_pred, float* x, float* last, float* m0,
                                      float* m1, int channels, int gen_frames, int total_frames, int height, int width,
                                      const float* coef_dev, const float* ab_dev, int dtype, void* stream) {
    const char* who = "fino_guided_unipc_step";
    FINO_TRY(fino_check_frames_step(who, dtype, cond_pred && uncond_pred && x && last && m0 && m1 && coef_dev && ab_dev, channels,
                                    gen_frames, total_frames, height, width));
    const int64_t total = (int64_t)channels * gen_frames * height * width;
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        guided_unipc_kernel<decltype(t)><<<fino_grid_1d(total, kFinoGridCap8, true), 256, 0, st>>>(
            (const uint16_t*)cond_pred, (const uint16_t*)uncond_pred, x, last, m0, m1, channels, gen_frames, total_frames,
            height * width, coef_dev, ab_dev);
    });
    return fino_launch_check(who);
}

extern "C" int fino_guided_vpred_step(const void* pred, void* lat, int64_t n_lat, int64_t batch_stride,
                                      const float* coef_dev, const float* ab_dev, int dtype, void* stream) {
    const char* who = "fino_guided_vpred_step";
    FINO_TRY(fino_check_flat_step(who, dtype, pred && lat && coef_dev && ab_dev, n_lat, true, batch_stride));
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        guided_vpred_kernel<decltype(t)><<<fino_grid_1d(n_lat, kFinoGridCap8, true), 256, 0, st>>>(
            (const uint16_t*)pred, (uint16_t*)lat, n_lat, batch_stride, coef_dev, ab_dev);
    });
    return fino_launch_check(who);
}

extern "C" int fino_guided_dpm_step(const void* pred, void* lat, float* x0_old, const void* noise, int64_t n_lat,
                                    int64_t batch_stride, const float* coef_dev, const float* ab_dev, int dtype,
                                    void* stream) {
    const char* who = "fino_guided_dpm_step";
    FINO_TRY(fino_check_flat_step(who, dtype, pred && lat && x0_old && noise && coef_dev && ab_dev, n_lat, true, batch_stride));
    hipStream_t st = (hipStream_t)stream;
    fino_dispatch_dtype(dtype, [&](auto t) {
        guided_dpm_kernel<decltype(t)><<<fino_grid_1d(n_lat, kFinoGridCap8, true), 256, 0, st>>>(
            (const uint16_t*)pred, (uint16_t*)lat, x0_old, (const uint16_t*)noise, n_lat, batch_stride, coef_dev, ab_dev);
    });
    return fino_launch_check(who);
}
