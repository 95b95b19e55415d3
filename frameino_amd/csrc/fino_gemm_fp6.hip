// MXFP6 (OCP e2m3 + one e8m0 scale per 32 elements along K) linear layers: the rung below MXFP8 on the reduced-precision
// ladder.  e2m3 keeps e4m3's three mantissa bits (the block scale supplies the range) and CDNA4 runs FP6 operands at the
// FP4 matrix rate: v_mfma_scale_f32_16x16x128_f8f6f4 with cbsz = blgp = 2 takes 16 cycles where the e4m3 form takes 32.
//   fino_quantize_mxfp6 : [rows, cols] bf16|fp16 -> packed e2m3 fragments + e8m0 block scales
//   fino_quantize_mxfp6_rot : the same of the blocks rotated by the 32-point Walsh-Hadamard matrix (outlier-robust; the GEMM
//                         of an ACT image and a WEIGHT image is the product of the unrotated operands)
//   fino_gemm_mxfp6     : C = epilogue(dequant(A) . dequant(W)^T + bias), fp32 accumulate, the fused epilogues of fino_gemm
//
// Operand layout (probed on hardware, tools/fp6/mfma_scale_probe_fp6.hip, result in profiles/mxfp6_probe.txt): the FP6 form
// reads the first 6 operand dwords of a lane as 32 six-bit fields at bits [6j, 6j + 6), multiplies field j of lane (row r =
// lane & 15, group g = lane >> 4) of one operand with field j of lane (row c, group g) of the other, and applies the scale
// operand of lane group g to exactly the 32 products of that lane pair -- so a lane must hold ONE whole 32-element scale block
// (here block g: k = 32g + j), and which block and which order inside it are the kernel's choice as long as both operands make
// the same one.  The e4m3 split of a lane into two 16-element halves 64 apart, each with its own scale block, does not match.
//
// The quantiser therefore writes the image the GEMM reads, not a row-major matrix.  A FRAGMENT is 16 rows x 128 K-elements
// = 64 lanes x 24 bytes = 1536 bytes, stored as [64 lanes][dwords 0..3] (1024 B) followed by [64 lanes][dwords 4..5] (512 B):
// a wave reads it with one ds_read_b128 and one ds_read_b64 at lane-linear addresses (conflict-free, full LDS rate; 96-byte
// rows would need ds_read_b96 at 3/8 of it).  Fragments are ordered [K / 128][rows_pad / 16] with rows_pad = rows rounded up
// to 256, so the 256 rows x 128 K of one block tile are 24 contiguous KiB in HBM and in LDS: the LDS-DMA is linear, 16 bytes
// per lane, with no swizzle and no per-row address arithmetic.  Rows beyond `rows` are never written by the quantiser and
// only feed accumulator rows / columns the epilogue does not store.
//
// The GEMM is the ping-pong kernel of fino_gemm_fp8.hip (256 x 256 tile, 8 waves as two groups half a K-tile apart, wave
// tile 128 x 64 = 8 x 4 fragments, operands held in registers through the 32 MFMAs of a K-tile) with two changes: the FP6
// matrix phase, and THREE LDS stages of 50 KiB where MXFP8 has two of 66: the matrix phase of a K-tile is half as long, so a
// tile requested one iteration ahead would not have arrived; tile t + 2 is requested during tile t.
#include <stdlib.h>

#include <type_traits>

#include "fino_gemm_common.h"

using namespace fino_gemm_ns;

namespace {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x2_t __attribute__((ext_vector_type(2)));

constexpr int kFragBytes = 1536;                          // 16 rows x 128 e2m3 elements
constexpr int kTile6 = 16 * kFragBytes;                   // 24 KiB: 256 rows of one K-tile
constexpr int kScale6 = 2048;                             // A scales 1 KiB + W scales 1 KiB per stage
constexpr int kStage6 = 2 * kTile6 + kScale6;             // 50 KiB
constexpr int kStages = 3;
constexpr int kSmem6 = (kStages * kStage6 > BM * kCsStride) ? kStages * kStage6 : BM * kCsStride;
static_assert(kSmem6 <= 160 * 1024, "LDS budget");

// ---------------------------------------------------------------------------------------------------- quantize
// One e2m3 code (sign, 2 exponent bits of bias 1, 3 mantissa bits) of y, |y| <= 7.5: round-to-nearest-even onto the grid
// whose step is 1/8 below 2, 1/4 below 4 and 1/2 below 8.  Adding 2^(23 + s) makes the fp32 adder round to a multiple of 2^s.
__device__ __forceinline__ uint32_t e2m3_code(float y) {
    const uint32_t yb = __float_as_uint(y);
    const uint32_t ab = yb & 0x7fffffffu;
    const uint32_t eb = ab & 0x7f800000u;
    const float big = __uint_as_float((eb > 0x3f800000u ? eb : 0x3f800000u) + (20u << 23));      // 2^(23 + max(ex, 0) - 3)
    const float r = (__uint_as_float(ab) + big) - big;
    const uint32_t normal = (__float_as_uint(r) >> 20) - 1008u;      // ((ex + 1) << 3) | mantissa for r in [1, 8)
    const uint32_t sub = (uint32_t)(r * 8.0f);                       // r in [0, 1): multiples of 1/8
    return (r < 1.0f ? sub : normal) | ((yb >> 26) & 32u);
}

// 16 codes -> 96 bits, code j at bit 6j
__device__ __forceinline__ void pack16(const uint32_t* c, uint32_t& d0, uint32_t& d1, uint32_t& d2) {
    d0 = c[0] | (c[1] << 6) | (c[2] << 12) | (c[3] << 18) | (c[4] << 24) | (c[5] << 30);
    d1 = (c[5] >> 2) | (c[6] << 4) | (c[7] << 10) | (c[8] << 16) | (c[9] << 22) | (c[10] << 28);
    d2 = (c[10] >> 4) | (c[11] << 2) | (c[12] << 8) | (c[13] << 14) | (c[14] << 20) | (c[15] << 26);
}

// y = H v, H the 32-point Walsh-Hadamard matrix (symmetric, H H = 32 I): five butterfly stages, strides 1, 2, 4, 8, 16 in that
// order, adds and subtracts only -- the order is the rule (include/frameino_hip.h), a plain fp32 restatement is bit-equal.
// Constant indices throughout: the block stays in the registers it was loaded into.
__device__ __forceinline__ void hadamard32(float* v) {
#pragma unroll
    for (int s = 1; s < 32; s <<= 1)
#pragma unroll
        for (int i = 0; i < 32; ++i)
            if ((i & s) == 0) {
                const float a = v[i], b = v[i + s];
                v[i] = a + b;
                v[i + s] = a - b;
            }
}

// wave = one fragment (16 rows x 128 columns); lane (r, g) owns the whole 32-element block g of row r
// ROT (fino_quantize_mxfp6_rot): 0 = none; FINO_MX_ROT_ACT: the block is rotated by H before the rule; FINO_MX_ROT_WEIGHT: the
// same codes, and the stored exponent is e - 5 (the 1/32 of H H, so the GEMM needs no factor)
template <typename T, int ROT = 0>
__global__ __launch_bounds__(256) void mxfp6_quantize_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ q,
                                                             uint8_t* __restrict__ scales, int64_t rows, int64_t cols,
                                                             int64_t ldx, int64_t rows_pad) {
    const int lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    const int64_t ktiles = cols >> 7;
    const int64_t total = ((rows + 15) >> 4) * ktiles;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t f = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); f < total; f += nwaves) {
        const int64_t rg = f / ktiles, kt = f - rg * ktiles;
        const int64_t row = rg * 16 + r;
        const int64_t srow = row < rows ? row : rows - 1;
        const int64_t col = kt * 128 + g * 32;
        const uint4* src = reinterpret_cast<const uint4*>(x + srow * ldx + col);
        float v[32];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float t[8];
            unpack8<T>(src[c], t);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[c * 8 + j] = t[j];
        }
        if constexpr (ROT != 0) hadamard32(v);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) amax = fmaxf(amax, fabsf(v[j]));
        // smallest e with amax <= 7.5 * 2^e: amax = m * 2^ex, m in [0.5, 1) -> ex - 3 while m <= 0.9375 (= 7.5 / 8), else ex - 2
        int e = -127;
        if (amax > 0.f) {
            int ex;
            const float m = frexpf(amax, &ex);
            e = ex - (m <= 0.9375f ? 3 : 2);
            e = e < -127 ? -127 : (e > 127 ? 127 : e);
        }
        uint32_t code[32];
#pragma unroll
        for (int j = 0; j < 32; ++j) code[j] = e2m3_code(__builtin_amdgcn_ldexpf(v[j], -e));      // exact: a power of two
        uint32_t d[6];
        pack16(code, d[0], d[1], d[2]);
        pack16(code + 16, d[3], d[4], d[5]);
        uint8_t* frag = q + (kt * (rows_pad >> 4) + rg) * kFragBytes;
        *reinterpret_cast<uint4*>(frag + lane * 16) = make_uint4(d[0], d[1], d[2], d[3]);
        *reinterpret_cast<uint2*>(frag + 1024 + lane * 8) = make_uint2(d[4], d[5]);
        if constexpr (ROT == FINO_MX_ROT_WEIGHT) e = e < -122 ? -127 : e - 5;
        if (row < rows) scales[mx_scale_index(row, col, rows_pad)] = (uint8_t)(e + 127);
    }
}

// ---------------------------------------------------------------------------------------------------- GEMM
// One 1-KiB LDS-DMA piece: 16 bytes per lane from buf[voff + soff] to LDS bytes [lds_dst + 16 lane, + 16).  Written as the
// instruction because the pieces of tile t + 2 stay in flight across barriers behind a counted s_waitcnt vmcnt(N): the
// compiler orders every LDS read after every LDS-DMA it knows of (vmcnt(0) at the top of the loop), which would cut the
// prefetch distance back to one tile.  M0 (the LDS base of the piece) is written in the statement that uses it and restored.
__device__ __forceinline__ void dma16(const u32x4_t rsrc, uint32_t voff, uint32_t soff, uint32_t lds_dst) {
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(rsrc), "s"(lds_dst), "s"(soff)
                 : "memory");
}
// raw buffer descriptor over [ptr, ptr + bytes): out-of-range lanes read nothing
__device__ __forceinline__ u32x4_t buffer_desc(const void* ptr, uint32_t bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(ptr);
    return u32x4_t{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a),
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)((uint32_t)(a >> 32) & 0xffffu)), bytes, 0x00020000u};
}

// KEEP (fino_gemm_mxfp6_keep; residual epilogues): the shared epilogue also stores its staged y = T(acc + bias) to g.c2
template <typename T, int EPI, bool KEEP = false>
__global__ __launch_bounds__(kThreads, 2) void gemm_mxfp6_kernel(const MxGemmParams fp) {   // g.a / w = fragment images
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const GemmParams& p = fp.g;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2;  // group
    const int wn = wave & 3;
    int tm, tn;
    tile_coords(p, tm, tn);
    const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

    // ---- LDS-DMA pieces: a K-tile of an operand is 24 contiguous KiB = 24 wave pieces of 1 KiB ----
    const int nk = (int)(p.k / 128);
    const uint32_t a_tile = (uint32_t)(fp.m_pad * 96), w_tile = (uint32_t)(fp.n_pad * 96);       // bytes between K-tiles
    const uint32_t sa_tile = (uint32_t)(fp.m_pad * 4), sw_tile = (uint32_t)(fp.n_pad * 4);
    const u32x4_t a_rsrc = buffer_desc(p.a, (uint32_t)nk * a_tile);
    const u32x4_t w_rsrc = buffer_desc(p.w, (uint32_t)nk * w_tile);
    // the K-tile's scales (1 KiB per operand): even waves of group 0 bring A's, odd waves W's (each twice: one count for all)
    const bool s_is_w = (wn & 1) != 0;
    const u32x4_t s_rsrc = buffer_desc(s_is_w ? fp.sw : fp.sa, (uint32_t)nk * (s_is_w ? sw_tile : sa_tile));
    const uint32_t s_tile = s_is_w ? sw_tile : sa_tile;
    const uint32_t s_off = (uint32_t)((s_is_w ? n0 : m0) * 4 + lane * 16);
    const uint32_t s_lds = 2 * kTile6 + (s_is_w ? 1024 : 0);
    // group wm brings its own 128 rows of A (pieces wm * 12 + q * 4 + wn, q = 0..2); W is pieces q * 4 + wn, q = 0..5
    const uint32_t a_off = (uint32_t)(m0 * 96 + (wm * 12 + wn) * 1024 + lane * 16);
    const uint32_t w_off = (uint32_t)(n0 * 96 + wn * 1024 + lane * 16);
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>((FINO_LDS char*)smem);
    const uint32_t a_lds = lds0 + (wm * 12 + wn) * 1024, w_lds = lds0 + kTile6 + wn * 1024;
#define F6_DMA_A(STAGE_, KT_, Q_) dma16(a_rsrc, a_off + (Q_) * 4096, (uint32_t)(KT_) * a_tile, a_lds + (STAGE_) * kStage6 + (Q_) * 4096);
#define F6_DMA_W(STAGE_, KT_, Q_) dma16(w_rsrc, w_off + (Q_) * 4096, (uint32_t)(KT_) * w_tile, w_lds + (STAGE_) * kStage6 + (Q_) * 4096);
#define F6_DMA_S(STAGE_, KT_) dma16(s_rsrc, s_off, (uint32_t)(KT_) * s_tile, lds0 + (STAGE_) * kStage6 + s_lds);

    const int frow = lane & 15;
    const int g4 = lane >> 4;
    const int a_base = wm * 8 * kFragBytes;
    const int w_base = kTile6 + wn * 4 * kFragBytes;
    const int sa_base = 2 * kTile6 + g4 * 256 + frow * 16 + wm * 8;            // 8 bytes: fragments i = 0..7
    const int sw_base = 2 * kTile6 + 1024 + g4 * 256 + frow * 16 + wn * 4;     // 4 bytes: fragments j = 0..3

    f32x4_t acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // prologue: tiles 0 and 1 whole (W split between the groups here: both wait for everything)
    const int wq0 = 3 * wm;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        F6_DMA_A(0, 0, q)
        F6_DMA_W(0, 0, wq0 + q)
    }
    F6_DMA_S(0, 0)
    if (nk > 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            F6_DMA_A(1, 1, q)
            F6_DMA_W(1, 1, wq0 + q)
        }
        F6_DMA_S(1, 1)
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();

    // Group 1 runs one barrier behind group 0: while one group reads LDS the other multiplies.  Stage reuse: tile t + 2
    // overwrites tile t - 1, whose last reader (group 1) finished before the barrier that opens group 0's iteration t.
    // Arrival: every wave waits for ITS pieces of tile t + 1 before the barrier that closes its iteration t (only the pieces
    // of tile t + 2, issued in this iteration, may stay in flight: 10 per wave of group 0, 3 per wave of group 1); group 0
    // brings all of W and the scales, which group 1 reads one barrier later, and each group brings the A rows only it reads.
    // The body is instantiated per group and for the last two tiles (nothing left to request, wait for everything) so that
    // no branch stands between the barriers: the MFMAs stay in their phase.
    u32x4_t af[8], wf[4];
    uint2 ah[8], wh[4];
    uint32_t sa_pk[2], sw_pk;
    int cur = 0, nxt = 2;          // stage of tile t, stage of tile t + 2
    auto iteration = [&](const int t, auto group_c, auto more_c) __attribute__((always_inline)) {
        constexpr int kGroup = decltype(group_c)::value;
        constexpr bool kMore = decltype(more_c)::value;
        const char* sb = smem + cur * kStage6;
        // ---------------- LOAD(t) ----------------
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            wf[j] = *reinterpret_cast<const u32x4_t*>(sb + w_base + j * kFragBytes + lane * 16);
            wh[j] = *reinterpret_cast<const uint2*>(sb + w_base + j * kFragBytes + 1024 + lane * 8);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            af[i] = *reinterpret_cast<const u32x4_t*>(sb + a_base + i * kFragBytes + lane * 16);
            ah[i] = *reinterpret_cast<const uint2*>(sb + a_base + i * kFragBytes + 1024 + lane * 8);
        }
        {   // e8m0 scales of my (row, K-block g4): byte b of a register serves fragment 4*reg + b (op_sel)
            const uint2 sa2 = *reinterpret_cast<const uint2*>(sb + sa_base);
            sa_pk[0] = sa2.x;
            sa_pk[1] = sa2.y;
            sw_pk = *reinterpret_cast<const uint32_t*>(sb + sw_base);
        }
        if constexpr (kMore) {
#pragma unroll
            for (int q = 0; q < 3; ++q) F6_DMA_A(nxt, t + 2, q)
            if constexpr (kGroup == 0) {
#pragma unroll
                for (int q = 0; q < 6; ++q) F6_DMA_W(nxt, t + 2, q)
                F6_DMA_S(nxt, t + 2)
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // ---------------- COMPUTE(t): 32 scaled FP6 MFMAs (K = 128 each) from registers ----------------
#define F6_OPERAND(LO_, HI_)                                                                                      \
    __builtin_shufflevector(__builtin_bit_cast(i32x4_t, LO_),                                                     \
                            __builtin_shufflevector(__builtin_bit_cast(i32x2_t, HI_),                             \
                                                    __builtin_bit_cast(i32x2_t, HI_), 0, 1, -1, -1),              \
                            0, 1, 2, 3, 4, 5, -1, -1)
#define F6_MMA(I_, J_)                                                                                            \
    {                                                                                                             \
        const i32x8_t wv_ = F6_OPERAND(wf[J_], wh[J_]);                                                           \
        const i32x8_t av_ = F6_OPERAND(af[I_], ah[I_]);                                                           \
        acc[I_][J_] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wv_, av_, acc[I_][J_], 2, 2, (J_), sw_pk,  \
                                                                       (I_) & 3, sa_pk[(I_) >> 2]);               \
    }
        // serpentine over the columns: exactly one operand register set changes between consecutive MFMAs
#define F6_ROW(I_) F6_MMA(I_, 0) F6_MMA(I_, 1) F6_MMA(I_, 2) F6_MMA(I_, 3)
#define F6_WOR(I_) F6_MMA(I_, 3) F6_MMA(I_, 2) F6_MMA(I_, 1) F6_MMA(I_, 0)
        F6_ROW(0) F6_WOR(1) F6_ROW(2) F6_WOR(3) F6_ROW(4) F6_WOR(5) F6_ROW(6) F6_WOR(7)
#undef F6_ROW
#undef F6_WOR
#undef F6_MMA
#undef F6_OPERAND
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!kMore) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if constexpr (kGroup == 0) {
            asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        cur = cur == kStages - 1 ? 0 : cur + 1;
        nxt = nxt == kStages - 1 ? 0 : nxt + 1;
    };
    using G0 = std::integral_constant<int, 0>;
    using G1 = std::integral_constant<int, 1>;
    int t = 0;
    if (wm == 0) {
        for (; t < nk - 2; ++t) iteration(t, G0{}, std::true_type{});
        for (; t < nk; ++t) iteration(t, G0{}, std::false_type{});
        __builtin_amdgcn_s_barrier();
    } else {
        for (; t < nk - 2; ++t) iteration(t, G1{}, std::true_type{});
        for (; t < nk; ++t) iteration(t, G1{}, std::false_type{});
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef F6_DMA_A
#undef F6_DMA_W
#undef F6_DMA_S
    gemm_epilogue<T, EPI, false, 8, KEEP>(acc, p, smem, m0, n0, tid, lane, wm, wn);
}

template <typename T, int EPI, bool KEEP = false>
int launch_mxfp6(const MxGemmParams& fp, hipStream_t st) {
    static FinoPerDeviceOnce once;
    if (int rc = fino_max_smem_once(once, reinterpret_cast<const void*>(&gemm_mxfp6_kernel<T, EPI, KEEP>), kSmem6, "fino_gemm_mxfp6")) return rc;
    gemm_mxfp6_kernel<T, EPI, KEEP><<<dim3((unsigned)(fp.g.tiles_m * fp.g.tiles_n)), kThreads, kSmem6, st>>>(fp);
    FINO_LAUNCH_CHECK();
    return FINO_OK;
}

}  // namespace

extern "C" int64_t fino_mxfp6_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || cols % 128) return 0;
    return (cols / 128) * ((rows + 255) / 256 * 16) * kFragBytes;
}

extern "C" int64_t fino_mxfp6_scale_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || cols % 128) return 0;
    return (cols / 128) * ((rows + 255) / 256 * 256) * 4;
}

namespace {

// the two quantiser entries: `fn` names the caller in the messages, ROT is its rotation (0 for fino_quantize_mxfp6)
template <int ROT>
int quantize_mxfp6_launch(const char* fn, const void* x, void* q, void* scales, int64_t rows, int64_t cols, int64_t ldx,
                          int dtype, void* stream) {
    FINO_CHECK(dtype == FINO_BF16 || dtype == FINO_F16, FINO_ERR_ARG, "%s: dtype %d", fn, dtype);
    FINO_CHECK(x && q && scales, FINO_ERR_ARG, "%s: null pointer", fn);
    FINO_CHECK(rows > 0 && cols > 0 && cols % 128 == 0 && ldx % 8 == 0 && ldx >= cols, FINO_ERR_ARG,
               "%s: cols must be a multiple of 128 (rows=%lld cols=%lld)", fn, (long long)rows, (long long)cols);
    FINO_CHECK(fino_aligned16(x) && fino_aligned16(q), FINO_ERR_ARG, "%s: alignment", fn);
    const int64_t rows_pad = (rows + 255) / 256 * 256;
    const int64_t total = ((rows + 15) / 16) * (cols / 128);      // fragments = waves
    int64_t grid = (total + 3) / 4;
    if (grid > 262144) grid = 262144;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == FINO_BF16)
        mxfp6_quantize_kernel<BF16, ROT><<<(unsigned)grid, 256, 0, st>>>((const uint16_t*)x, (uint8_t*)q, (uint8_t*)scales,
                                                                         rows, cols, ldx, rows_pad);
    else
        mxfp6_quantize_kernel<F16, ROT><<<(unsigned)grid, 256, 0, st>>>((const uint16_t*)x, (uint8_t*)q, (uint8_t*)scales,
                                                                        rows, cols, ldx, rows_pad);
    const hipError_t err = hipGetLastError();
    FINO_CHECK(err == hipSuccess, FINO_ERR_LAUNCH, "%s: launch failed: %s", fn, hipGetErrorString(err));
    return FINO_OK;
}

}  // namespace

extern "C" int fino_quantize_mxfp6(const void* x, void* q, void* scales, int64_t rows, int64_t cols, int64_t ldx,
                                   int dtype, void* stream) {
    return quantize_mxfp6_launch<0>("fino_quantize_mxfp6", x, q, scales, rows, cols, ldx, dtype, stream);
}

extern "C" int fino_quantize_mxfp6_rot(const void* x, void* q, void* scales, int64_t rows, int64_t cols, int64_t ldx,
                                       int dtype, int mode, void* stream) {
    FINO_CHECK(mode == FINO_MX_ROT_ACT || mode == FINO_MX_ROT_WEIGHT, FINO_ERR_ARG,
               "fino_quantize_mxfp6_rot: mode %d (FINO_MX_ROT_ACT = 1 | FINO_MX_ROT_WEIGHT = 2)", mode);
    return mode == FINO_MX_ROT_ACT
               ? quantize_mxfp6_launch<FINO_MX_ROT_ACT>("fino_quantize_mxfp6_rot", x, q, scales, rows, cols, ldx, dtype, stream)
               : quantize_mxfp6_launch<FINO_MX_ROT_WEIGHT>("fino_quantize_mxfp6_rot", x, q, scales, rows, cols, ldx, dtype,
                                                           stream);
}

extern "C" int fino_gemm_mxfp6(const void* aq, const void* a_scales, const void* wq, const void* w_scales,
                               const void* bias, void* c, int64_t m, int64_t n, int64_t k, int64_t ldc, int epilogue,
                               const void* r, int64_t ldr, const float* gate, int64_t mod_stride, const int32_t* sel,
                               int out_dtype, void* stream) {
    MxGemmParams fp;
    if (int rc = mx_gemm_params(fp, "fino_gemm_mxfp6", false, aq, a_scales, wq, w_scales, bias, c, m, n, k, ldc, epilogue, r,
                                ldr, gate, mod_stride, sel, out_dtype))
        return rc;
    if (m == 0) return FINO_OK;
    FINO_CHECK(fp.m_pad * k < (1ll << 31) && fp.n_pad * k < (1ll << 31), FINO_ERR_UNSUPPORTED,
               "fino_gemm_mxfp6: operand > 2 GiB");
    hipStream_t st = (hipStream_t)stream;
    return gemm_dispatch_dtype(out_dtype, [&](auto t) {
        return gemm_dispatch_epilogue(epilogue, [&](auto e) { return launch_mxfp6<decltype(t), decltype(e)::value>(fp, st); });
    });
}

extern "C" int fino_gemm_mxfp6_keep(const void* aq, const void* a_scales, const void* wq, const void* w_scales,
                                    const void* bias, void* c, int64_t m, int64_t n, int64_t k, int64_t ldc, int epilogue,
                                    const void* r, int64_t ldr, const float* gate, int64_t mod_stride, const int32_t* sel,
                                    int out_dtype, void* keep, int64_t ldk, void* stream) {
    MxGemmParams fp;
    if (int rc = mx_gemm_params(fp, "fino_gemm_mxfp6_keep", false, aq, a_scales, wq, w_scales, bias, c, m, n, k, ldc, epilogue,
                                r, ldr, gate, mod_stride, sel, out_dtype))
        return rc;
    if (int rc = mx_gemm_keep_params(fp, "fino_gemm_mxfp6_keep", epilogue, keep, ldk)) return rc;
    if (m == 0) return FINO_OK;
    FINO_CHECK(fp.m_pad * k < (1ll << 31) && fp.n_pad * k < (1ll << 31), FINO_ERR_UNSUPPORTED,
               "fino_gemm_mxfp6_keep: operand > 2 GiB");
    hipStream_t st = (hipStream_t)stream;
    return gemm_dispatch_dtype(out_dtype, [&](auto t) {
        return gemm_dispatch_keep_epilogue(
            epilogue, [&](auto e) { return launch_mxfp6<decltype(t), decltype(e)::value, true>(fp, st); });
    });
}
