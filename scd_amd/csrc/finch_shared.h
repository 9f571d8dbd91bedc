// What scd_first_neighbor (finch.hip) and scd_knn (knn.hip) share: the float64 dot that gives a pair its one value, and the preparation
// of the fp16 operand of the filter passes with the terms of their error bound (docs/design/finch.md, docs/design/knn.md).
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------------ the float64 dot
// One lane per dot: four partial sums, element c into sum c mod 4 in increasing c (fma), then (s0 + s1) + (s2 + s3).  `vec`: both rows
// are 16-byte aligned and d is a multiple of 4, so the elements come as float4 - the same sums in the same order, a quarter of the loads.
__device__ __forceinline__ double fn_dot64(const float* __restrict__ a, const float* __restrict__ b, int d, bool vec) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int c = 0;
    if (vec) {
        for (; c < d; c += 4) {
            const float4 x = *reinterpret_cast<const float4*>(a + c), y = *reinterpret_cast<const float4*>(b + c);
            s0 = fma((double)x.x, (double)y.x, s0);
            s1 = fma((double)x.y, (double)y.y, s1);
            s2 = fma((double)x.z, (double)y.z, s2);
            s3 = fma((double)x.w, (double)y.w, s3);
        }
        return (s0 + s1) + (s2 + s3);
    }
    for (; c + 4 <= d; c += 4) {
        s0 = fma((double)a[c], (double)b[c], s0);
        s1 = fma((double)a[c + 1], (double)b[c + 1], s1);
        s2 = fma((double)a[c + 2], (double)b[c + 2], s2);
        s3 = fma((double)a[c + 3], (double)b[c + 3], s3);
    }
    if (c < d) s0 = fma((double)a[c], (double)b[c], s0);
    if (c + 1 < d) s1 = fma((double)a[c + 1], (double)b[c + 1], s1);
    if (c + 2 < d) s2 = fma((double)a[c + 2], (double)b[c + 2], s2);
    return (s0 + s1) + (s2 + s3);
}
__device__ __forceinline__ bool fn_vec_ok(const float* U, int d) { return (d & 3) == 0 && ((uintptr_t)U & 15) == 0; }

// ------------------------------------------------------------------------------------------------ prep
// gstat: [0] bits of max h_i, [1] bits of max e_i (non-negative floats order as their bits), [2] a value that does not fit fp16
static __global__ void __launch_bounds__(256) fn_prep_kernel(const float* __restrict__ U, long long n, int d, int ld, long long n_alloc,
                                                      half_t* __restrict__ H, float* __restrict__ e_out, float* __restrict__ h_out,
                                                      unsigned* __restrict__ gstat) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_alloc) return;
    half_t* dst = H + (size_t)row * ld;
    if (row >= n) {
        for (int c = lane; c < ld; c += 64) dst[c] = (half_t)0.f;
        return;
    }
    const float* src = U + (size_t)row * d;
    double e2 = 0.0, h2 = 0.0;
    int bad = 0;
    for (int c = lane; c < ld; c += 64) {
        half_t hv = (half_t)0.f;
        if (c < d) {
            const float x = src[c];
            hv = (half_t)x;
            float hf = (float)hv;
            if (!(fabsf(hf) <= 65504.f)) {                      // infinity or NaN
                bad = 1;
                hv = (half_t)0.f;
                hf = 0.f;
            } else if (fabsf(hf) < 6.103515625e-05f) {          // a subnormal half: flushed, the bound carries it in e_i
                hv = (half_t)0.f;
                hf = 0.f;
            }
            const double r = (double)x - (double)hf;
            e2 = fma(r, r, e2);
            h2 = fma((double)hf, (double)hf, h2);
        }
        dst[c] = hv;
    }
    e2 = wave_sum_f64(e2);
    h2 = wave_sum_f64(h2);
    bad = __any(bad);
    if (lane == 0) {
        const float ef = (float)(sqrt(e2) * 1.000001), hf = (float)(sqrt(h2) * 1.000001);
        e_out[row] = ef;
        h_out[row] = hf;
        if (ef == ef) atomicMax(&gstat[1], __float_as_uint(ef));
        if (hf == hf) atomicMax(&gstat[0], __float_as_uint(hf));
        if (bad || !(ef == ef)) atomicOr(&gstat[2], 1u);
    }
}
