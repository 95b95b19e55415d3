// Host launch path shared by the row, sampler, step-cache, token, guider, LoRA, condition and VAE kernels (and the dtype
// dispatcher of the GEMM family): the tag dispatchers, the 1-D and row-per-wave launch shapes, the argument checks whose
// sentences repeat from entry point to entry point, and a launch check that is told whose launch it checks.
// Plain inline functions and generic lambdas: nothing here is looked up at run time, and everything inlines.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "fino_common.h"

// `expr` is a check that returns FINO_OK or has set the error text: leave the entry point with its code
#define FINO_TRY(expr)                       \
    do {                                     \
        if (const int rc__ = (expr)) return rc__; \
    } while (0)

// ---- run-time choices -> template arguments ------------------------------------------------------------------------
// A dispatcher calls `launch` with the choice as a tag value and `launch` is a generic lambda that names the instantiation
// (the rule of fino_gemm_common.h: a lambda is instantiated for EVERY tag its dispatcher can pass, so an entry point that
// accepts two dtypes uses the two-way dispatcher).  The caller has validated `dtype`.
template <typename F>
inline auto fino_dispatch_dtype(int dtype, F&& launch) {
    return dtype == FINO_BF16 ? launch(BF16{}) : launch(F16{});
}
// ... and FINO_F32; the fp32 tag is the translation unit's own (its kernels are specialised on it)
template <typename F32Tag, typename F>
inline auto fino_dispatch_dtype3(int dtype, F&& launch) {
    if (dtype == FINO_BF16) return launch(BF16{});
    if (dtype == FINO_F16) return launch(F16{});
    return launch(F32Tag{});
}
// the 512-column passes a row of `dim` elements takes in one wave (8 elements per lane): 1 .. 8, false beyond NPmax * 512
template <int NPmax, typename F>
inline bool dispatch_np(int dim, F&& f) {
    const int np = (dim + 511) / 512;
    switch (np) {
        case 1: f(std::integral_constant<int, 1>{}); return true;
        case 2: f(std::integral_constant<int, 2>{}); return true;
        case 3: f(std::integral_constant<int, 3>{}); return true;
        case 4: f(std::integral_constant<int, 4>{}); return true;
        case 5: f(std::integral_constant<int, 5>{}); return true;
        case 6: f(std::integral_constant<int, 6>{}); return true;
        case 7: f(std::integral_constant<int, 7>{}); return true;
        case 8: f(std::integral_constant<int, 8>{}); return true;
        default: return false;
    }
}

// ---- launch shapes -------------------------------------------------------------------------------------------------
constexpr int64_t kFinoGridCap8 = 256 * 8;        // ~8 blocks per CU, grid-stride the rest
constexpr int64_t kFinoGridCap16 = 256 * 16;      // the Wan VAE's elementwise kernels
constexpr int64_t kFinoGridCapWide = 262144;      // the CogVideoX VAE's and the condition builders'
// workgroups of `block` threads for `total` items, at most `cap`, and at least one where the call site asks for it
inline unsigned fino_grid_1d(int64_t total, int64_t cap, bool at_least_one, int block = 256) {
    int64_t g = (total + block - 1) / block;
    if (g > cap) g = cap;
    return (unsigned)(at_least_one && g < 1 ? 1 : g);
}

// `who`: launch failed?
inline int fino_launch_check(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fino_set_error("%s: launch failed: %s", who, hipGetErrorString(e));
        return FINO_ERR_LAUNCH;
    }
    return FINO_OK;
}

// One wave per row, `waves` rows per workgroup, `parts` row segments in grid.y: launch(T{}, np, grid, block) with the element
// type and the pass count as tags.  `dim_who` prefixes the refusal of a dim beyond NPmax passes, `who` a failed launch.
template <int NPmax, typename F>
inline int fino_launch_rows(const char* who, const char* dim_who, int64_t rows, unsigned parts, int waves, int dim, int dtype,
                            F&& launch) {
    const dim3 grid((unsigned)((rows + waves - 1) / waves), parts), block(waves * 64);
    const bool ok = dispatch_np<NPmax>(dim, [&](auto np) {
        fino_dispatch_dtype(dtype, [&](auto t) { launch(t, np, grid, block); });
    });
    FINO_CHECK(ok, FINO_ERR_UNSUPPORTED, "%s: dim %d > %d unsupported", dim_who, dim, NPmax * 512);
    return fino_launch_check(who);
}

// ---- the argument checks that repeat ---------------------------------------------------------------------------------
inline int fino_check_dtype(const char* who, int dtype) {
    FINO_CHECK(dtype == FINO_BF16 || dtype == FINO_F16, FINO_ERR_ARG, "%s: dtype %d", who, dtype);
    return FINO_OK;
}
inline int fino_check_dtype3(const char* who, int dtype) {
    FINO_CHECK(dtype == FINO_BF16 || dtype == FINO_F16 || dtype == FINO_F32, FINO_ERR_ARG, "%s: dtype %d", who, dtype);
    return FINO_OK;
}
// dtype, then the rows x dim of a row kernel (the caller returns FINO_OK for rows == 0 behind it)
inline int fino_check_rows_dim(const char* who, int64_t rows, int dim, int dtype) {
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(rows >= 0 && dim > 0 && dim % 8 == 0, FINO_ERR_ARG, "%s: rows=%lld dim=%d (dim %% 8 != 0)", who, (long long)rows,
               dim);
    return FINO_OK;
}
inline int fino_check_strides(const char* who, int64_t dim, std::initializer_list<int64_t> strides) {
    bool ok = true;
    for (const int64_t ld : strides) ok = ok && ld >= dim;
    FINO_CHECK(ok, FINO_ERR_ARG, "%s: a row stride is below dim", who);
    return FINO_OK;
}
// elements per 16 bytes
inline int fino_per16(int dtype) { return dtype == FINO_F32 ? 4 : 8; }
// rows that 16-byte accesses can walk: an aligned base and a stride that is a multiple of `per16` elements
inline bool fino_rows_ok(const void* p, int64_t ld, int per16) { return fino_aligned16(p) && ld % per16 == 0; }
struct FinoRows {
    const void* p;
    int64_t ld;          // 0: a plain pointer (a NULL one passes, as in fino_aligned16)
};
// ... for every (pointer, stride) listed, and whatever else the entry point folds into the same sentence
inline int fino_check_aligned16(const char* who, int per16, std::initializer_list<FinoRows> rows, bool also = true) {
    bool ok = also;
    for (const FinoRows& r : rows) ok = ok && fino_rows_ok(r.p, r.ld, per16);
    FINO_CHECK(ok, FINO_ERR_ARG, "%s: 16-byte alignment required", who);
    return FINO_OK;
}

// The sampler steps, plain (fino_cfg_*_step) and guided (fino_guided_*_step): one check per sampler, the caller says
// whether the pointers ITS kernel reads are there.  Both sets launch fino_grid_1d(total, kFinoGridCap8, true) x 256.
// ... over [channels, gen_frames of total_frames, height, width] (Euler, UniPC)
inline int fino_check_frames_step(const char* who, int dtype, bool pointers, int channels, int gen_frames, int total_frames,
                                  int height, int width) {
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(pointers, FINO_ERR_ARG, "%s: null pointer", who);
    FINO_CHECK(channels > 0 && gen_frames > 0 && total_frames >= gen_frames && height > 0 && width > 0, FINO_ERR_ARG,
               "%s: bad shape", who);
    return FINO_OK;
}
// ... over n_lat flat elements, the unconditional half batch_stride behind where there is one (v-prediction, DPM++)
inline int fino_check_flat_step(const char* who, int dtype, bool pointers, int64_t n_lat, bool two_halves, int64_t batch_stride) {
    FINO_TRY(fino_check_dtype(who, dtype));
    FINO_CHECK(pointers && n_lat > 0 && (!two_halves || batch_stride >= n_lat), FINO_ERR_ARG, "%s: bad arguments", who);
    return FINO_OK;
}
