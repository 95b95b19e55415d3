// The device code of the four fused sampler steps, shared by the fino_cfg_*_step kernels (fino_elementwise.hip) and their
// fino_guided_*_step siblings (fino_guidance.hip).  Every function is templated on V, "how v is formed" from the conditional
// and the unconditional prediction; everything after that point is the same arithmetic for both.  The two Wan steps are
// per-element functions (`*_step_elem`: the kernel keeps its grid-stride loop and the reads of its scalars), the two CogVideoX
// steps whole bodies (`*_step_body`, loop included) -- the split under which the plain-CFG kernels compile to the instructions
// they compiled to before the code was shared.  Both including files are compiled with -ffp-contract=off: every product and
// sum below is its own fp32 rounding.
#pragma once
#include <type_traits>

#include "fino_common.h"

// The grid-stride loop of the two CogVideoX bodies, which keep their loop: the launch's indices are read in the kernel
// (FINO_GRID_STRIDE: there the compiler knows that the workgroups are uniform; read inside a device function, blockDim costs a
// load and a select per kernel) and combined where the loop needs them, which is where the plain kernels combined them.
struct GridStride {
    uint32_t block_idx, thread_idx, grid, block;
    __device__ __forceinline__ int64_t first() const { return (int64_t)block_idx * block + thread_idx; }
    __device__ __forceinline__ int64_t stride() const { return (int64_t)grid * block; }
};
#define FINO_GRID_STRIDE() \
    GridStride { blockIdx.x, threadIdx.x, gridDim.x, blockDim.x }

// ---- how v is formed -----------------------------------------------------------------------------------------
// plain CFG as the Wan pipeline evaluates it on T-typed predictions: v = T(u + T(g * T(c - u)))
template <typename T>
struct CfgRounded {
    float g;
    __device__ __forceinline__ float operator()(float c, float u) const {
        return round_to<T>(u + round_to<T>(g * round_to<T>(c - u)));
    }
};
// plain CFG on the upcast predictions (CogVideoX): v = u + g * (c - u) in fp32
struct CfgF32 {
    float g;
    static __device__ __forceinline__ CfgF32 load(const float* __restrict__ p) { return CfgF32{p[0]}; }
    __device__ __forceinline__ float operator()(float c, float u) const { return u + g * (c - u); }
};
// a guider's pair {A, B} (fino_guider_coefs): v = fl(fl(A c) + fl(B u)) in fp32 ...
struct GuidedF32 {
    float a, b;
    static __device__ __forceinline__ GuidedF32 load(const float* __restrict__ p) { return GuidedF32{p[0], p[1]}; }
    __device__ __forceinline__ float operator()(float c, float u) const { return a * c + b * u; }
};
// ... rounded to T where the plain CFG value is a T value
template <typename T>
struct GuidedRounded {
    float a, b;
    __device__ __forceinline__ float operator()(float c, float u) const { return round_to<T>(a * c + b * u); }
};

// ---- Wan: flow-match Euler -----------------------------------------------------------------------------------
template <typename T, typename V>
__device__ __forceinline__ void euler_step_elem(int64_t i, const uint16_t* __restrict__ pc,
                                                const uint16_t* __restrict__ pu, float* __restrict__ lat, int Fg, int Ft,
                                                int HW, V vf, float dt, int round_out) {
    const int s = (int)(i % HW);
    const int f = (int)((i / HW) % Fg);
    const int c = (int)(i / ((int64_t)HW * Fg));
    const int64_t pi = ((int64_t)c * Ft + f) * HW + s;
    float n = T::to_f32(pc[pi]);
    if (pu) {
        const float u = T::to_f32(pu[pi]);
        n = vf(n, u);
    }
    float v = lat[i] + dt * n;
    if (round_out) v = round_to<T>(v);
    lat[i] = v;
}

// ---- CogVideoX sampler step (pipeline_cogvideox_i2v_motion_FrameINO.py:893-927 with a v-prediction DDIM step):
//   v = u + g*(c - u) in fp32 (the reference upcasts noise_pred, :896);  x0 = T(sa*x) - sb*v;  x' = T(T(ca*x) + cb*x0)
//   (x is the T-typed latent; products of x with the scheduler's 0-dim coefficients stay in T under torch promotion).
// coef = {sa, sb, ca, cb, g} on the device.  pred: [2, Ft, C*HW] (uncond, cond), lat: [Fg, C*HW] in place.
template <typename T, typename V>
__device__ __forceinline__ void vpred_step_body(const uint16_t* __restrict__ pred, uint16_t* __restrict__ lat,
                                                int64_t n_lat, int64_t batch_stride, float sa, float sb, float ca,
                                                float cb, V vf, int has_uncond, GridStride ix) {
    for (int64_t i = ix.first(); i < n_lat; i += ix.stride()) {
        float v;
        if (has_uncond) {
            const float u = T::to_f32(pred[i]);
            const float c = T::to_f32(pred[batch_stride + i]);
            v = vf(c, u);
        } else {
            v = T::to_f32(pred[i]);
        }
        const float x = T::to_f32(lat[i]);
        const float x0 = round_to<T>(sa * x) - sb * v;
        lat[i] = T::from_f32(round_to<T>(ca * x) + cb * x0);
    }
}

// ---- CogVideoXDPMScheduler.step (diffusers, third-party; the sampler the CogVideoX-5B-I2V repo ships and the reference's
// training-time validation builds, train_code/train_cogvideox_motion_FrameINO.py:692; pipeline call site :915-926):
// SDE-DPM-Solver++ (2M) on v-prediction, fused with CFG.  Linear in {x, v, x0_old, noise}; the host folds the step's
// scalars into coef = {sa, sb, m1, m2, m3, m4, mn, g, use_old}:
//   v  = u + g*(c-u) (fp32: the pipeline takes noise_pred.float(), :897);  x0 = T(sa*x) - sb*v            (fp32)
//   d  = use_old ? m3*x0 - m4*x0_old : x0;   x' = T( T(m1*x) - m2*d + T(mn*noise) );   x0_old <- x0
// (products of the T-typed latent / noise with the scheduler's 0-dim coefficients stay in T under torch promotion.)
template <typename T, typename V>
__device__ __forceinline__ void dpm_step_body(const uint16_t* __restrict__ pred, uint16_t* __restrict__ lat,
                                              float* __restrict__ x0_old, const uint16_t* __restrict__ noise,
                                              int64_t n_lat, int64_t batch_stride, const float* __restrict__ coef,
                                              const float* __restrict__ v_src, int has_uncond, GridStride ix) {
    const float sa = coef[0], sb = coef[1], m1 = coef[2], m2 = coef[3], m3 = coef[4], m4 = coef[5], mn = coef[6];
    // (V is loaded HERE, between the reads of coef[6] and coef[8], where the plain kernel read g = coef[7]: the order of the
    // scalar loads is what keeps the plain kernel's instructions; the other three steps take V by value)
    const V vf = V::load(v_src);
    const bool use_old = coef[8] != 0.f;
    for (int64_t i = ix.first(); i < n_lat; i += ix.stride()) {
        float v;
        if (has_uncond) {
            const float u = T::to_f32(pred[i]);
            const float c = T::to_f32(pred[batch_stride + i]);
            v = vf(c, u);
        } else {
            v = T::to_f32(pred[i]);
        }
        const float x = T::to_f32(lat[i]);
        const float x0 = round_to<T>(sa * x) - sb * v;
        const float d = use_old ? m3 * x0 - m4 * x0_old[i] : x0;
        const float nz = round_to<T>(mn * T::to_f32(noise[i]));
        lat[i] = T::from_f32(round_to<T>(m1 * x) - m2 * d + nz);
        x0_old[i] = x0;
    }
}

// ---- UniPC (bh2, predict-x0, flow sigmas) multistep update fused with CFG, one pass over the latents
// (diffusers UniPCMultistepScheduler.step as Wan2.2-TI2V-5B-Diffusers configures it; pipeline :882-891).
// Every tensor op of the published algorithm is linear in {x, last_sample, m0, m1, v}; the host folds the step's
// scalars into coef = {g, sigma, use_corr, Cx, C0, C1, Ct, Px, P0, P1}:
//   v   = T(u + T(g*T(c-u)));  m_t = x - T(sigma*v)                         (convert_model_output, flow prediction)
//   x_c = use_corr ? Cx*last + C0*m0 + C1*m1 + Ct*m_t : x                    (multistep_uni_c_bh_update)
//   x'  = Px*x_c + P0*m_t + P1*m0                                            (multistep_uni_p_bh_update)
//   last <- x_c;  m1 <- m0;  m0 <- m_t;  x <- x'
// `sigma_t * model_output` as torch evaluates it on this device: the exact product rounded ONCE to T.  For fp16 torch's
// compiled elementwise product is one v_fma_mixlo_f16 (no fp32 rounding in between; tests/test_kernels_gpu.py::test_cfg_unipc_step),
// for bf16 the fp32 product rounded to bf16.
template <typename T>
__device__ __forceinline__ float round_product(float a, float b) {
    if constexpr (std::is_same<T, F16>::value) {
        uint32_t r = 0;
        asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "+v"(r) : "v"(a), "v"(b));
        return F16::to_f32((uint16_t)r);
    } else {
        return round_to<T>(a * b);
    }
}

template <typename T, typename V>
__device__ __forceinline__ void unipc_step_elem(int64_t i, const uint16_t* __restrict__ pc,
                                                const uint16_t* __restrict__ pu, float* __restrict__ x,
                                                float* __restrict__ last, float* __restrict__ m0, float* __restrict__ m1,
                                                int Fg, int Ft, int HW, float sigma, float use_corr, float Cx, float C0,
                                                float C1, float Ct, float Px, float P0, float P1, V vf) {
    const int s = (int)(i % HW);
    const int f = (int)((i / HW) % Fg);
    const int c = (int)(i / ((int64_t)HW * Fg));
    const int64_t pi = ((int64_t)c * Ft + f) * HW + s;
    float v = T::to_f32(pc[pi]);
    if (pu) {
        const float u = T::to_f32(pu[pi]);
        v = vf(v, u);
    }
    const float xv = x[i], a0 = m0[i];
    const float mt = xv - round_product<T>(sigma, v);
    const float xc = use_corr != 0.f ? Cx * last[i] + C0 * a0 + C1 * m1[i] + Ct * mt : xv;
    x[i] = Px * xc + P0 * mt + P1 * a0;
    last[i] = xc;
    m1[i] = a0;
    m0[i] = mt;
}
