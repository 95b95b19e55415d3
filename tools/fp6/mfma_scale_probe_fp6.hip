// Layout probe for v_mfma_scale_f32_16x16x128_f8f6f4 with e2m3 operands (cbsz = blgp = 2, gfx950): one wave computes
// D = A.B^T for a 16x128 A and a 16x128 B of 6-bit codes with per-(row, 32-k block) e8m0 scales, and the host checks the
// hypotheses about which elements, in which bit order, and which scale a lane must hold.
// Build: hipcc --offload-arch=gfx950 -O2 mfma_scale_probe_fp6.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// element order inside a lane:
// variant 0: lane l holds row l&15, k = 32*(l>>4) + j, j = 0..31, code j in bits [6j, 6j+6) of its 6 dwords
// variant 1: the e4m3 form's split: codes 0..15 are k = 16*(l>>4) + j, codes 16..31 are k = 64 + 16*(l>>4) + (j-16)
// variant 2: as 0 with the bit string big-endian inside each dword group (code j in bits [186-6j, 192-6j))
__global__ void probe(const uint8_t* A, const uint8_t* B, const uint8_t* sA, const uint8_t* sB, float* D, int variant) {
    const int l = threadIdx.x, row = l & 15, g = l >> 4;
    uint32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 32; ++j) {
        const int k = variant == 1 ? (j < 16 ? 16 * g + j : 64 + 16 * g + (j - 16)) : 32 * g + j;
        const int bit = variant == 2 ? 186 - 6 * j : 6 * j;
        const uint64_t ca = A[row * 128 + k], cb = B[row * 128 + k];
        const int w = bit >> 5, sh = bit & 31;
        a[w] |= (uint32_t)(ca << sh); b[w] |= (uint32_t)(cb << sh);
        if (sh > 26) { a[w + 1] |= (uint32_t)(ca >> (32 - sh)); b[w + 1] |= (uint32_t)(cb >> (32 - sh)); }
    }
    i32x8 av, bv;
    for (int i = 0; i < 8; ++i) { av[i] = (int)a[i]; bv[i] = (int)b[i]; }
    const int sa = sA[row * 4 + g], sb = sB[row * 4 + g];      // scale block g of my row
    f32x4 c = {0, 0, 0, 0};
    c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 2, 2, 0, sa, 0, sb);
    for (int i = 0; i < 4; ++i) D[l * 4 + i] = c[i];
}

static float e2m3(uint8_t v) {   // OCP e2m3: sign, 2 exponent bits (bias 1), 3 mantissa bits
    const int s = (v >> 5) & 1, e = (v >> 3) & 3, m = v & 7;
    const float x = e == 0 ? m / 8.0f : ldexpf(1.0f + m / 8.0f, e - 1);
    return s ? -x : x;
}

int main() {
    uint8_t hA[16 * 128], hB[16 * 128], hsA[64], hsB[64];
    srand(1);
    for (int i = 0; i < 16 * 128; ++i) { hA[i] = rand() % 64; hB[i] = rand() % 64; }      // every code, subnormals included
    for (int i = 0; i < 64; ++i) { hsA[i] = 126 + rand() % 3; hsB[i] = 127 + rand() % 2; }
    uint8_t *dA, *dB, *dsA, *dsB; float* dD;
    if (hipMalloc(&dA, sizeof hA) != hipSuccess) { printf("no device\n"); return 1; }
    hipMalloc(&dB, sizeof hB); hipMalloc(&dsA, 64); hipMalloc(&dsB, 64); hipMalloc(&dD, 1024);
    hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice); hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
    hipMemcpy(dsA, hsA, 64, hipMemcpyHostToDevice); hipMemcpy(dsB, hsB, 64, hipMemcpyHostToDevice);
    int matches = 0;
    for (int variant = 0; variant < 3; ++variant) {
        float hD[256];
        probe<<<1, 64>>>(dA, dB, dsA, dsB, dD, variant);
        if (hipMemcpy(hD, dD, 1024, hipMemcpyDeviceToHost) != hipSuccess) { printf("kernel failed\n"); return 1; }
        // reference: D[m][n] = sum_k A[m][k] B[n][k] 2^(sA[m][blk]-127) 2^(sB[n][blk]-127); blk by hypothesis
        for (int blkmode = 0; blkmode < 2; ++blkmode) {       // 0: blk = k/32; 1: blk = (k%64)/16 (the e4m3 form's grouping)
            for (int cd = 0; cd < 2; ++cd) {                  // C/D map: 0: col=lane&15,row=4*(lane>>4)+reg ; 1: transposed
                double err = 0, mag = 0;
                for (int l = 0; l < 64; ++l) for (int r = 0; r < 4; ++r) {
                    const int col = l & 15, rw = 4 * (l >> 4) + r;
                    const int m = cd == 0 ? rw : col, n = cd == 0 ? col : rw;
                    double ref = 0;
                    for (int k = 0; k < 128; ++k) {
                        const int blk = blkmode == 0 ? k / 32 : (k % 64) / 16;
                        ref += (double)e2m3(hA[m * 128 + k]) * e2m3(hB[n * 128 + k]) * ldexp(1.0, hsA[m * 4 + blk] - 127) *
                               ldexp(1.0, hsB[n * 4 + blk] - 127);
                    }
                    err += fabs(ref - hD[l * 4 + r]); mag += fabs(ref);
                }
                const bool ok = err < 1e-3 * mag;
                matches += ok;
                printf("operand variant %d, scale-block mode %d, C/D map %d: sum|err| = %.3f (sum|ref| = %.1f)%s\n", variant,
                       blkmode, cd, err, mag, ok ? "   <-- MATCH" : "");
            }
        }
    }
    return matches ? 0 : 2;
}
