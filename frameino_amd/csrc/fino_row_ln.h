// One token row in the registers of one 64-lane wave, and the LayerNorm + AdaLN arithmetic on it: what fino_elementwise.hip's
// row kernels and fino_teacache.hip's probe share, so that both write the same bits.  A lane holds the 16-byte vectors
// lane, lane + 64, ... of the row (NP of them, zeros beyond `dim`).  Both units are built with -ffp-contract=off: the
// rounding points are the reference's (mul, mul, sub -- not fma).
#pragma once
#include "fino_common.h"

template <typename T, int NP, bool NT = false>
__device__ __forceinline__ void load_row(const uint16_t* __restrict__ p, int dim, int lane, float (&v)[NP][8]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < dim) {
            uint4 u;
            if constexpr (NT) {
                const u32x4_t t4 = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p + c));
                u = make_uint4(t4[0], t4[1], t4[2], t4[3]);
            } else {
                u = *reinterpret_cast<const uint4*>(p + c);
            }
            unpack8<T>(u, v[i]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
        }
    }
}

template <int NP>
__device__ __forceinline__ void ln_stats(const float (&v)[NP][8], int dim, int lane, float eps, float& mean,
                                         float& rstd) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
    mean = wave_sum(s) / (float)dim;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < dim) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float d = v[i][j] - mean;
                q += d * d;
            }
        }
    }
    const float var = wave_sum(q) / (float)dim;
    rstd = 1.0f / sqrtf(var + eps);
}

// 8 consecutive fp32 values of a modulation / affine row
__device__ __forceinline__ void ln_ld8(const float* p, float (&o)[8]) {
    const float4 a0 = *reinterpret_cast<const float4*>(p);
    const float4 a1 = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a0.x; o[1] = a0.y; o[2] = a0.z; o[3] = a0.w; o[4] = a1.x; o[5] = a1.y; o[6] = a1.z; o[7] = a1.w;
}

// the Wan AdaLN-zero value of one element before its one rounding to T: LN(x) * (1 + scale) + shift
__device__ __forceinline__ float ln_adaln_value(float x, float mean, float rstd, float scale, float shift) {
    const float n = (x - mean) * rstd;
    return n * (1.0f + scale) + shift;
}
