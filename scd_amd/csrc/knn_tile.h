// What scd_knn (knn.hip) and scd_mr_nearest (hdbscan.hip) share: the shape of the two MFMA passes and their 128 x 128 x d tile
// (docs/design/knn.md, docs/design/hdbscan.md).
#pragma once
#include "common.h"

#define KNN_BM 128
#define KNN_BN 128
#define KNN_BK 64
#define KNN_LDK 72                              // LDS row stride in halfs (144 bytes), as FN_LDK
#define KNN_THREADS 256
#define KNN_YMAX 32
#define KNN_TARGET_BLOCKS 1024
#define KNN_LDS_BYTES (2 * (KNN_BM + KNN_BN) * KNN_LDK * 2)
#define KNN_DP_MAX 1024
#define KNN_KMAX 64
#define KNN_SLOTS 512                           // candidate slots per row; 16 * KNN_YMAX kept values fit them too
#define KNN_CHUNK (KNN_SLOTS - KNN_KMAX)        // columns per step of the exact pass: the best so far ride in front

// ------------------------------------------------------------------------------------------------ one 128 x 128 x d tile
// acc[mt][nt][r] <- HQ row (row0 + wave * 32 + mt * 16 + lq * 4 + r) . HX row (j0 + nt * 16 + lr).  fn_main_kernel's loop.
__device__ __forceinline__ void knn_tile(const half_t* __restrict__ gA, const half_t* __restrict__ gB, int ld, int dp, half_t* sA, half_t* sB,
                                         int a_frag, int b_frag, int st_off, f32x4 (&acc)[2][8]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = ld / KNN_BK;
    half8 ra[4], rb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ra[i] = *reinterpret_cast<const half8*>(gA + (size_t)i * 32 * ld);
        rb[i] = *reinterpret_cast<const half8*>(gB + (size_t)i * 32 * ld);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<half8*>(sA + st_off + i * 32 * KNN_LDK) = ra[i];
        *reinterpret_cast<half8*>(sB + st_off + i * 32 * KNN_LDK) = rb[i];
    }
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
        const int cur = kc & 1;
        const bool more = kc + 1 < nk;
        if (more) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ra[i] = *reinterpret_cast<const half8*>(gA + (size_t)i * 32 * ld + (kc + 1) * KNN_BK);
                rb[i] = *reinterpret_cast<const half8*>(gB + (size_t)i * 32 * ld + (kc + 1) * KNN_BK);
            }
        }
        const half_t* cA = sA + cur * (KNN_BM * KNN_LDK) + a_frag;
        const half_t* cB = sB + cur * (KNN_BN * KNN_LDK) + b_frag;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if (kc * KNN_BK + ks * 32 < dp) {
                const half8 fa0 = *reinterpret_cast<const half8*>(cA + ks * 32);
                const half8 fa1 = *reinterpret_cast<const half8*>(cA + 16 * KNN_LDK + ks * 32);
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) {
                    const half8 fb = *reinterpret_cast<const half8*>(cB + nt * 16 * KNN_LDK + ks * 32);
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa0, fb, acc[0][nt], 0, 0, 0);
                    acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa1, fb, acc[1][nt], 0, 0, 0);
                }
            }
        }
        if (more) {
            half_t* nA = sA + (cur ^ 1) * (KNN_BM * KNN_LDK) + st_off;
            half_t* nB = sB + (cur ^ 1) * (KNN_BN * KNN_LDK) + st_off;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<half8*>(nA + i * 32 * KNN_LDK) = ra[i];
                *reinterpret_cast<half8*>(nB + i * 32 * KNN_LDK) = rb[i];
            }
        }
        __syncthreads();
    }
}
