// Image x text similarity with fused top-k for gfx950.  The N x V logit matrix is never written.
//
// Replaces (paths under /root/reference):
//   100*(F @ W) -> softmax -> topk x2      main_unsup.py:504-531   (unsup, softmax values)
//   100*(F @ W) -> topk x2                 main_ptsup.py:526-545   (ptsup, raw values)
//   argmax(100*F_u @ W_sel)                main_unsup.py:601-614, main_ptsup.py:668-676
//
// Decision semantics (shared with oracle/naming_oracle.py): order = (float64 dot product desc, index asc).
// Pass 1 (MFMA, fp32 accumulate) keeps 2 x 8 approximate candidates per image in registers; pass 2
// recomputes the candidates' dot products in float64, sorts them, and certifies that no non-candidate
// could reach rank k given the accumulation error bound; uncertified rows take an exact full-row pass.
#include "common.h"
#include <stdlib.h>
#include <type_traits>

#define TOPM 8

__device__ __forceinline__ void topm_insert(float (&lv)[TOPM], int (&li)[TOPM], float v, int idx) {
#pragma unroll
    for (int j = TOPM - 1; j >= 1; --j) {
        const bool up = v > lv[j - 1];
        const bool here = v > lv[j];
        lv[j] = up ? lv[j - 1] : (here ? v : lv[j]);
        li[j] = up ? li[j - 1] : (here ? idx : li[j]);
    }
    if (v > lv[0]) {
        lv[0] = v;
        li[0] = idx;
    }
}


template <int TM>
__device__ __forceinline__ void topm_insert_n(float (&lv)[TM], int (&li)[TM], float v, int idx) {
#pragma unroll
    for (int j = TM - 1; j >= 1; --j) {
        const bool up = v > lv[j - 1];
        const bool here = v > lv[j];
        lv[j] = up ? lv[j - 1] : (here ? v : lv[j]);
        li[j] = up ? li[j - 1] : (here ? idx : li[j]);
    }
    if (v > lv[0]) {
        lv[0] = v;
        li[0] = idx;
    }
}

// bf[dc*4 + k16] for a runtime d-chunk dc (0..7) and a compile-time k16: a switch over constants keeps the fragment
// array in registers (a runtime-indexed array would be demoted to scratch)
__device__ __forceinline__ half8 bf_sel(const half8 (&bf)[32], int dc, int k16) {
    switch (dc) {
        case 0: return bf[0 + k16];
        case 1: return bf[4 + k16];
        case 2: return bf[8 + k16];
        case 3: return bf[12 + k16];
        case 4: return bf[16 + k16];
        case 5: return bf[20 + k16];
        case 6: return bf[24 + k16];
        default: return bf[28 + k16];
    }
}

// Block = 8 waves = 256 images; wave w keeps the B fragments (F rows, K <= 512) of its 32 images in registers for the
// whole kernel and sweeps the vocabulary in tiles of 128 names.  W^T tiles are streamed by LDS-DMA (global_load_lds,
// 16 B/lane) in sub-tiles of [128 names][64 d] (128-B rows, 16-B chunk XOR (row>>1)&7 applied to the DMA source address
// and to the ds_read side) through a 4-slot ring; one flattened software pipeline runs over (tile, d-chunk): the DMAs of
// sub-step s+3 are issued after the mid-sub-step barrier that publishes slot s+1, waits are counted, fragment reads run
// one MFMA group ahead (same schedule as gemm_dma_kernel).
// v_mfma_f32_32x32x16_f16: A[row = name][k] from LDS, B[k][col = image] from registers,
// D[row = (reg&3)+8(reg>>2)+4h][col = image]: every lane sees 16 logits of ONE image per 32-name block, so the
// running top-8 list, its threshold and the online-softmax statistics are lane-private registers.
typedef __attribute__((address_space(3))) void* sim_lds_ptr_t;

// NW = 8 (default): one 512-thread block (256 images) per CU.  NW = 4 (SCD_SIM_NW=4, same speed): TWO independent 256-thread blocks (128 images each)
// per CU: their tile epilogues (the divergent top-8 maintenance, ~1/3 of the kernel) drift apart, so one block's MFMAs run
// under the other's epilogue - with eight waves behind one barrier all of them reach the epilogue together.
// NDC = 12 (d = 768, the ViT-L/14 embedding; NW = 4): 44 of the 48 image fragments in registers, which takes the register file of a
// wave that is alone on its SIMD (512 registers): one 256-thread block (128 images) per CU.
template <bool SOFTMAX, int NW, int NDC = 8>
__global__ void __launch_bounds__(NW * 64, NW == 4 && NDC == 8 ? 2 : 1) sim_topk_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt,
                                                          long long n, int d, long long v, float scale,
                                                          float* __restrict__ cand_val, int* __restrict__ cand_idx,
                                                          float* __restrict__ stats, int xmode) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // 4 x 16 KB ring + 8 x 4 KB parked fragments
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r = lane & 31, hh = lane >> 5;
    constexpr int IPW = 16 / NW;                                      // ring-fill instructions per wave and sub-step
    const long long img = (long long)blockIdx.x * (NW * 32) + wave * 32 + r;
    const long long irow = img < n ? img : n - 1;
    const half_t* frow = F + irow * d + 8 * hh;

    // 28 of the 32 image fragments stay in registers; the last four (d-chunk 7) are parked in a per-wave LDS
    // patch and re-read once per tile: with all 32 resident hipcc spills some of them to scratch, and every scratch reload
    // is a vmcnt(0) that drains the fill ring
    constexpr int NBF = 4 * NDC - 4;                                 // fragments in registers; d-chunk NDC - 1 is parked
    half8 bf[NBF];
    char* bfl = smem + 65536 + wave * 4096 + lane * 16;
#pragma unroll
    for (int s = 0; s < 4 * NDC; ++s) {
        half8 t;
        if (16 * s < d) {
            t = *(const half8*)(frow + 16 * s);
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) t[q] = (half_t)0.f;
        }
        if (s < NBF) bf[s] = t;
        else *(half8*)(bfl + (s - NBF) * 1024) = t;
    }
    // the image fragments are complete before the loop: a load still pending at the loop header makes hipcc put a
    // vmcnt(0) in front of the first use of every fragment in every sub-step, which drains the fill ring each time
#pragma unroll
    for (int s = 0; s < NBF; ++s) asm volatile("" : "+v"(bf[s]));
    float lv[TOPM];
    int li[TOPM];
#pragma unroll
    for (int j = 0; j < TOPM; ++j) {
        lv[j] = -INFINITY;
        li[j] = -1;
    }
    float sm_m = -INFINITY, sm_z = 0.f;

    const int nd = d >> 6;                                  // 64-deep sub-steps per tile
    const int ntiles = (int)((v + 127) / 128);
    const int steps = ntiles * nd;
    // DMA source of this lane: wave w stages rows w*16 .. w*16+15 (2 instructions x 8 rows); lane -> (row lane/8, chunk lane%8)
    // Every fill address = wave-uniform base (tile, d-chunk: scalar) + a per-lane 32-bit byte offset that never changes
    // (row, swizzled chunk), so a fill costs no vector arithmetic; only the last tile, whose padded names re-read row v-1,
    // has its own offsets.  (Computed per fill, the 64-bit address took ~14 VALU instructions with two quarter-rate
    // multiplies: several hundred issue cycles per wave and sub-step.)
    unsigned voff[IPW], voff_last[IPW];
    const int ntiles_ = (int)((v + 127) / 128);
#pragma unroll
    for (int p = 0; p < IPW; ++p) {
        const int rowl = wave * (8 * IPW) + p * 8 + (lane >> 3);
        const int col = ((lane & 7) ^ ((rowl >> 1) & 7)) << 3;
        long long vr = (long long)(ntiles_ - 1) * 128 + rowl;
        vr = vr < v ? vr : v - 1;
        voff[p] = (unsigned)((rowl * d + col) * 2);
        voff_last[p] = (unsigned)(((int)(vr - (long long)(ntiles_ - 1) * 128) * d + col) * 2);
    }
    const unsigned sbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    auto issue = [&](int tile, int dc, int slot) {
        const half_t* base = Wt + (size_t)tile * 128 * d + dc * 64;
        const bool lastt = tile == ntiles_ - 1;
#pragma unroll
        for (int p = 0; p < IPW; ++p) {
            // asm, not the builtin: for the builtin hipcc assumes the fill may alias every later ds_read and drains the whole
            // ring (s_waitcnt vmcnt(0)) in the middle of each sub-step; the counted waits below are the synchronisation
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                         ::"s"(sbase + slot * 16384 + wave * (1024 * IPW) + p * 1024), "v"(lastt ? voff_last[p] : voff[p]), "s"(base) : "memory");
        }
    };
    auto off128 = [](int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); };

    f32x16 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;

    int ntile = 0, ndc = 0;
#pragma unroll
    for (int pre = 0; pre < 3; ++pre) {
        if (pre < steps) issue(ntile, ndc, pre);
        if (++ndc == nd) { ndc = 0; ++ntile; }
    }
    if (steps >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * IPW) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    half8 fa[4], fb[4];                                     // two fragment sets, alternating between the four k16 groups
    auto rd = [&](const char* slot, int k16, half8 (&f)[4]) {
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) f[cb] = *(const half8*)(slot + off128(cb * 32 + r, 2 * k16 + hh));
    };
    auto mm = [&](const half8 (&f)[4], const half8 b) {
        if (xmode & 2) return;                               // timing ablation: no MFMAs
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[cb], b, acc[cb], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    rd(smem, 0, fa);
    int s = 0;                                              // flattened sub-step counter (ring slot = s & 3)
    for (int tile = 0; tile < ntiles; ++tile) {
#pragma unroll
        for (int dcc = 0; dcc < NDC; ++dcc) {               // d-chunk index is a compile-time constant: bf[] stays in registers
            if (dcc < nd) {
                const char* cur = smem + (s & 3) * 16384;
                half8 b0, b1, b2, b3;
                if (dcc == NDC - 1) {
                    b0 = *(const half8*)bfl; b1 = *(const half8*)(bfl + 1024);
                    b2 = *(const half8*)(bfl + 2048); b3 = *(const half8*)(bfl + 3072);
                } else {
                    b0 = bf[dcc * 4 + 0 < NBF ? dcc * 4 + 0 : 0]; b1 = bf[dcc * 4 + 1 < NBF ? dcc * 4 + 1 : 0];
                    b2 = bf[dcc * 4 + 2 < NBF ? dcc * 4 + 2 : 0]; b3 = bf[dcc * 4 + 3 < NBF ? dcc * 4 + 3 : 0];
                }
                rd(cur, 1, fb);
                mm(fa, b0);
                rd(cur, 2, fa);
                mm(fb, b1);
                if (s + 1 < steps) {
                    if (s + 2 >= steps) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPW) : "memory");
                }
                __builtin_amdgcn_s_barrier();               // slot s+1 visible; slot s-1 free
                asm volatile("" ::: "memory");
                if (s + 3 < steps) issue(ntile, ndc, (s + 3) & 3);
                if (++ndc == nd) { ndc = 0; ++ntile; }
                rd(cur, 3, fb);
                mm(fa, b2);
                if (s + 1 < steps) rd(smem + ((s + 1) & 3) * 16384, 0, fa);
                mm(fb, b3);
                ++s;
            }
        }
        {
            // tile epilogue on UNSCALED dot products (scale > 0 is applied when the lists are written): one max3 tree per
            // 32-name block decides whether any of its 16 values can enter the list; only the last tile has padded names.
            const long long vbase = (long long)tile * 128 + 4 * hh;
            const bool last = tile == ntiles - 1;
            // List maintenance is the expensive part of this kernel (1.5 of 4.0 ms measured with the insertion run for
            // every value slot in which ANY of the 64 lanes had a candidate: ~2300 wave-wide insertions of ~40 VALU
            // instructions per wave).  Two changes:
            //  * the admission threshold is shared by the two lanes that serve one image (r and r+32 see different names):
            //    a value has to beat the larger of the two lists' 8th entries.  Everything rejected is <= that threshold,
            //    which only grows and ends as max(list_A[7], list_B[7]) - the bound sim_refine_kernel certifies against;
            //  * a candidate is first parked in a one-entry per-lane queue (a 2-instruction conditional move); the wave-wide
            //    insertion runs when some lane needs its queue slot again and once at the end of the tile, and then serves
            //    every lane that has something parked.
            float thr = lv[TOPM - 1];
            {
                const unsigned u = __float_as_uint(thr);
                const auto pr = __builtin_amdgcn_permlane32_swap(u, u, false, false);
                thr = fmaxf(thr, __uint_as_float((lane & 32) ? pr[0] : pr[1]));
            }
            float qv = -INFINITY;
            int qi = -1;
            if ((xmode & 1) && !last) thr = INFINITY;        // timing ablation: nothing is admitted (results are wrong)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                if (last) {
#pragma unroll
                    for (int i = 0; i < 16; ++i)
                        if (vbase + cb * 32 + (i & 3) + 8 * (i >> 2) >= v) acc[cb][i] = -INFINITY;
                }
                float bm = fmaxf(fmaxf(acc[cb][0], acc[cb][1]), acc[cb][2]);
#pragma unroll
                for (int i = 3; i < 15; i += 2) bm = fmaxf(fmaxf(bm, acc[cb][i]), acc[cb][i + 1]);
                bm = fmaxf(bm, acc[cb][15]);
                if (__any(bm > thr)) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float val = acc[cb][i];
                        if (__any(val > thr)) {
                            if (__any(val > thr && qi >= 0)) {         // somebody needs its queue slot: serve everybody
                                if (qi >= 0) topm_insert(lv, li, qv, qi);
                                qi = -1;
                                thr = fmaxf(thr, lv[TOPM - 1]);
                            }
                            if (val > thr) {
                                qv = val;
                                qi = (int)(vbase + cb * 32 + (i & 3) + 8 * (i >> 2));
                            }
                        }
                    }
                }
                if (SOFTMAX) {
                    if (bm > -INFINITY) {
                        const float mn = fmaxf(sm_m, bm);
                        float z = sm_z * __expf((sm_m - mn) * scale);
#pragma unroll
                        for (int i = 0; i < 16; ++i) z += __expf((acc[cb][i] - mn) * scale);
                        sm_z = z;
                        sm_m = mn;
                    }
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[cb][i] = 0.f;
            }
            if (__any(qi >= 0)) {
                if (qi >= 0) topm_insert(lv, li, qv, qi);
            }
        }
    }
    if (img < n) {
        float* cv = cand_val + (img * 2 + hh) * TOPM;
        int* ci = cand_idx + (img * 2 + hh) * TOPM;
#pragma unroll
        for (int j = 0; j < TOPM; ++j) {
            cv[j] = lv[j] * scale;
            ci[j] = li[j];
        }
        if (SOFTMAX) {
            stats[(img * 2 + hh) * 2] = sm_m * scale;
            stats[(img * 2 + hh) * 2 + 1] = sm_z;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Row-block schedule (d == 512, the CLIP embedding width), as round 2's four-wave kernel introduced it; that kernel is gone (git
// history keeps it), its eight-wave successors below keep the units, ring, keys and lists described here.  Same outputs as the
// kernels above, different schedule:
//   * one wave per SIMD (256 threads, 512 registers); wave w owns 64 images (two 32-image sets) whose 2 x 32 B fragments live
//     in 256 AGPRs and feed the MFMAs directly;
//   * the unit of work is a block of 32 NAMES with its whole K = 512: 32 rows x 1 KB of W^T = 32 KB, ONE 1-KB LDS-DMA
//     instruction per row (whole contiguous rows; 16-B chunk c of row r lands at chunk c ^ (r & 15), applied on the DMA source
//     address and on the ds_read address: conflict-free A-fragment reads).  A unit is 32 k16 steps x 2 image sets = 64 MFMAs on
//     ONE accumulator pair (2 x 16 registers), so the accumulators of unit u-1 are complete while unit u is being computed:
//   * the epilogue of unit u-1 is dealt over the 32 MFMA steps of unit u (two accumulator pairs alternate) instead of running
//     behind a barrier with the matrix pipe idle (the eight-wave kernel spends 46 % of its wave time parked), and it is
//     BRANCH-FREE in the common case: each of a lane's 16 values becomes a key (low 4 mantissa bits = position in the unit), a
//     max / med3 network keeps the two largest keys, the largest is widened to a double whose low mantissa word carries the
//     name index and pushed through a min / max chain over the lane's sorted list of TM doubles (no index arrays, no compares).
//     Only when a lane's SECOND key also beats its list (the first units, then ~3 % of the unit-sets) a loop admits the rest;
//   * a 4-slot ring of units: one barrier per unit (64 MFMAs per wave).  At the barrier of unit u the fills of unit u+1 have
//     landed (counted vmcnt), so the first fragments of u+1 are read at the end of u and no MFMA waits behind a barrier for
//     LDS latency; the fills of unit u+3 go into the slot unit u-1 just left, one per 4 k16 steps.
// MFMAs, fragment reads, waits and the min / max / med3 of the selection are asm (AGPR B operands; counted lgkmcnt that carries
// the fragment registers; no IEEE canonicalisation in front of every max).  Hazard the compiler cannot see: an accumulator
// pair is first read >= 2 steps (4 MFMAs, >= 128 cycles) after its last MFMA was issued.
__device__ __forceinline__ float rb_max(float a, float b) { float d; asm("v_max_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ float rb_med3(float a, float b, float c) { float d; asm("v_med3_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c)); return d; }
__device__ __forceinline__ double rb_max64(double a, double b) { double d; asm("v_max_f64 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ double rb_min64(double a, double b) { double d; asm("v_min_f64 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
#define RB_NEG -3.0e38f                    /* masks padded names: finite, so that widening + index bits stays a number */


// ------------------------------------------------------------------------------------------------
// Eight-wave row-block kernel (round 3; default at d == 512).  Same unit structure, ring, keys and lists as the four-wave kernel above described,
// but TWO waves per SIMD with 32 images each (128 AGPRs of B fragments + <= 128 VGPRs): the four-wave kernel's lone wave per SIMD
// has to issue everything itself - 64 MFMAs (8 issue cycles each), ~170-290 vector instructions of epilogue, 32 fragment reads,
// 8 ring fills (60-100 cycles of issue each) and the waits - in ONE in-order stream per unit, ~4,100-4,700 cycles against 2,048
// of matrix work (PMC, profiles/r02_pmc_sim_rb.txt: matrix pipe busy 47 %).  With a partner wave on the SIMD the matrix pipe takes
// the other wave's MFMA while this one sits in a fill, a wait or its epilogue; per wave a unit is 32 MFMAs on ONE accumulator
// set (two sets alternate between units), 4 ring fills, 16 values per lane:
//   step  2..9   two values into the (largest, second) key pair
//   step  10     widen the winner; softmax reference maximum
//   step 11..26  one list entry (max, min on doubles) and one softmax term per step;  step 27: the rare second-key loop
__device__ __forceinline__ float rb_swap32(float v, int lane) {         // the value held by lane l ^ 32
    const unsigned u = __float_as_uint(v);
    const auto p = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __uint_as_float((lane & 32) ? p[0] : p[1]);
}
#define RB8_EMARGIN 4.2f                   /* sim_refine_kernel certifies against (other half's entry KS) - 3.9 E: keep it below this */
template <bool SOFTMAX, int TM, int KS>
__global__ void __launch_bounds__(512) sim_topk_rb8_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt_all, long long n,
                                                           long long v_all, float scale, float* __restrict__ cand_val,
                                                           int* __restrict__ cand_idx, float* __restrict__ stats,
                                                           const unsigned* __restrict__ wmax2_bits, int rb0 = 0, int nparts = 1,
                                                           long long vsplit = 0, long long out_row0 = 0, long long part_rows = 0) {
    // rb0 / nparts / vsplit (round 4): the launch's row blocks are rb0 + blockIdx.x / nparts; with nparts == 2 a row block is served
    // by TWO blocks, names [0, vsplit) and [vsplit, v), whose lists go to side arrays (row (part * part_rows + img - out_row0)) and are
    // merged by sim_split_merge_kernel - the partial last round of row blocks (626 blocks on 256 CUs at the C4 shard: 256 + 256 + 114)
    // then costs half a round instead of a whole one.
    constexpr int D = 512, UB = 32768;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r = lane & 31, hh = lane >> 5;
    const unsigned sbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const int rbi = (int)blockIdx.x / nparts, part = (int)blockIdx.x - rbi * nparts;
    const long long v_lo = part ? vsplit : 0, v_hi = (nparts == 2 && part == 0) ? vsplit : v_all;
    const long long v = v_hi - v_lo;                           // this block's vocabulary: names v_lo .. v_hi - 1, local indices below
    const half_t* Wt = Wt_all + (size_t)v_lo * D;

    half8 bf[32];
    float f2 = 0.f;
    const long long img = (long long)(rb0 + rbi) * 256 + wave * 32 + r;
    {
        // eight fragments at a time (the "memory" clobber keeps the next batch's loads behind the pins): loaded all at once the
        // 32 fragments need 128 VGPRs on their way to the AGPRs, and the kernel has 128 in all
        const half_t* frow = F + (img < n ? img : n - 1) * D + 8 * hh;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int s = 8 * b; s < 8 * b + 8; ++s) bf[s] = *(const half8*)(frow + 16 * s);
#pragma unroll
            for (int s = 8 * b; s < 8 * b + 8; ++s)
#pragma unroll
                for (int q = 0; q < 8; ++q) f2 = fmaf((float)bf[s][q], (float)bf[s][q], f2);
#pragma unroll
            for (int s = 8 * b; s < 8 * b + 8; ++s) asm volatile("" : "+a"(bf[s]) : : "memory");   // resident in AGPRs from here on
        }
    }
    // The two lanes of an image (r, r + 32: different names) share what they know: once the OTHER lane's list holds KS + 1 values of
    // at least t, a value below t - 4 E (E = sim_refine_kernel's bound on |approximate - exact|) cannot be among the image's KS + 1
    // largest exact values, so it is neither listed nor looked at again.  That lifts a lane's admission threshold from its own TM-th
    // best to about the image's (KS + 1)-th best and makes the second-key path below 7 x rarer (it stalls the other seven waves at
    // the unit's barrier whenever one wave takes it).  Everything dropped this way is <= max(list_A[KS], list_B[KS]) - 4 E, which is
    // what sim_refine_kernel adds to its certificate (argument ks).
    f2 += rb_swap32(f2, lane);
    const float e4 = RB8_EMARGIN * 1.5f * ((float)D * 5.9604645e-8f + 2.4e-7f + 2.0e-6f) * sqrtf(f2) * sqrtf(__uint_as_float(*wmax2_bits)) * 1.001f + 1e-30f;

    double L[TM];                                              // the lane's TM best (key | name index), descending
    float thr = -INFINITY;                                     // float view of L[TM-1]
    float tsh = -INFINITY, te = -INFINITY;                     // (other lane's entry KS) - 4 E; te = max(thr, tsh): what a value must beat
    float m1, m2, smm = -INFINITY, smz = 0.f, nmc;
    double tk;
#pragma unroll
    for (int j = 0; j < TM; ++j) L[j] = -INFINITY;
    const float c2 = scale * 1.4426950408889634f;              // exp((a - m) * scale) = exp2((a - m) * c2)

    const int nunits = (int)((v + 31) / 32);
    // ring fill: wave w stages rows 4w .. 4w+3 of a unit, one 1-KB instruction per row; lane l fetches source chunk l ^ (row & 15)
    // = (l ^ (4w & 12)) ^ p for row 4w + p: ONE per-lane register, the row is wave-uniform (four per-row offset registers, and the
    // kernel spills: a scratch reload in the loop is a vmcnt(0) that drains the ring)
    const unsigned bsw = (unsigned)((lane ^ ((4 * wave) & 12)) << 4);
    const half_t* fbase = Wt;
    unsigned fm0 = 0;
    int frows = 32;                                            // valid rows of the unit being filled (< 32 only for the last one)
    auto fill_unit = [&](int unit) {
        fbase = Wt + (size_t)unit * 32 * D;
        fm0 = sbase + (unit & 3) * UB + 4 * wave * 1024;
        const long long left = v - (long long)unit * 32;
        frows = left < 32 ? (int)left : 32;
    };
    auto fill = [&](int p) {
        int srow = 4 * wave + p;                                                // wave-uniform
        srow = srow < frows ? srow : frows - 1;                                 // padded names re-read row v-1; masked in the epilogue
        const unsigned off = (bsw ^ (unsigned)(p << 4)) + (unsigned)srow * 1024u;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                     ::"s"(fm0 + p * 1024), "v"(off), "s"(fbase) : "memory");
    };
    unsigned fa[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) fa[j] = sbase + (unsigned)(r * 1024 + ((32 * j) ^ (16 * (hh ^ (r & 15)))));

#define RB_RD(DST, J, IMM) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(fa[J]), "n"(IMM))
#define RB_WAIT(N, FR) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(FR))
#define RB_MFMA(ACC, A, B) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(ACC) : "v"(A), "a"(B))
#define RB_MFMA0(ACC, A, B) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, 0" : "=&v"(ACC) : "v"(A), "a"(B))

    auto key = [](float a, int i) { return __uint_as_float((__float_as_uint(a) & 0xfffffff0u) | (unsigned)i); };
    auto name_of = [&](int unit, int i) { return unit * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh; };
    auto p_top2 = [&](const f32x16& a, int i) {
        const float k = key(a[i], i);
        if (i == 0) {
            m1 = k;
            m2 = -INFINITY;
        } else {
            const float n1 = rb_max(m1, k);
            m2 = rb_med3(m1, m2, k);
            m1 = n1;
        }
    };
    auto widen = [&](float k, int unit) {
        const int i = (int)(__float_as_uint(k) & 15u);
        return __hiloint2double(__double2hiint((double)k), name_of(unit, i));
    };
    auto p_ins = [&](int j) {
        const double hi = rb_max64(L[j], tk);
        if (j + 1 < TM) tk = rb_min64(L[j], tk);
        L[j] = hi;
        if (j + 1 == TM) {
            thr = (float)L[TM - 1];
            te = rb_max(thr, tsh);
        }
    };
    auto p_ins_all = [&]() {
#pragma unroll
        for (int j = 0; j < TM; ++j) p_ins(j);
    };
    auto p_share = [&]() {
        tsh = rb_swap32((float)L[KS], lane) - e4;
        te = rb_max(thr, tsh);
    };
    auto p_rest = [&](const f32x16& a, int unit) {             // rare: the lane's second key beats what it has to beat as well
        if (!__any(m2 > te)) return;
        tk = m2 > te ? widen(m2, unit) : (double)-INFINITY;
        p_ins_all();
        int cnt = 0;                                           // a third one?  (keys, as everywhere: the key bits are part of E)
#pragma unroll
        for (int i = 0; i < 16; ++i) cnt += key(a[i], i) > te ? 1 : 0;
        if (!__any(cnt > 2)) return;
        float bound = m2;
        for (;;) {
            float c = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float kk = key(a[i], i);
                c = (kk < bound && kk > c) ? kk : c;
            }
            if (!__any(c > te)) break;
            if (c > te) {
                tk = widen(c, unit);
                p_ins_all();
            }
            bound = c;
        }
    };
    auto p_sm_begin = [&]() {
        const float mref = rb_max(smm, m1);
        smz = smz * __builtin_amdgcn_exp2f((smm - mref) * c2);
        smm = mref;
        nmc = -mref * c2;
    };
    auto p_sm_add = [&](const f32x16& a, int i) { smz += __builtin_amdgcn_exp2f(fmaf(a[i], c2, nmc)); };

    f32x16 acc[2];
    half8 fr[4];
    auto body = [&](auto has_prev, auto parity, int u) {
        constexpr int P = decltype(parity)::value;
        constexpr bool EPI = decltype(has_prev)::value;
        // my fills of unit u+1 have landed (those of u+2 may fly); after the barrier everybody's have, and slot (u-1)&3 is free
        if (u + 2 < nunits) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool more = u + 1 < nunits;
        const bool fills = u + 3 < nunits;
        if (fills) fill_unit(u + 3);
        static_for<0, 32>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            if (s == 29) {
                const unsigned delta = ((u + 1) & 3) ? (unsigned)UB : (unsigned)(-3 * UB);      // wave-uniform
#pragma unroll
                for (int j = 0; j < 8; ++j) fa[j] += delta;
            }
            if constexpr (s < 29) RB_RD(fr[(s + 3) & 3], (s + 3) & 7, ((s + 3) >> 3) * 256);
            else if (more) RB_RD(fr[(s + 3) & 3], (s + 3 - 32) & 7, 0);
            if (s < 29 || more) RB_WAIT(2, fr[(s + 1) & 3]);
            else if (s == 29) RB_WAIT(1, fr[(s + 1) & 3]);
            else if (s == 30) RB_WAIT(0, fr[(s + 1) & 3]);
            if (s == 0) RB_MFMA0(acc[P], fr[s & 3], bf[s]);
            else RB_MFMA(acc[P], fr[s & 3], bf[s]);
            if ((s & 7) == 7 && fills) fill(s >> 3);
            if constexpr (EPI) {
                if constexpr (s >= 2 && s < 10) {
                    p_top2(acc[1 - P], 2 * (s - 2));
                    p_top2(acc[1 - P], 2 * (s - 2) + 1);
                } else if constexpr (s == 10) {
                    tk = widen(m1, u - 1);
                    if (SOFTMAX) p_sm_begin();
                } else if constexpr (s >= 11 && s < 27) {
                    if constexpr (s - 11 < TM) p_ins(s - 11);
                    if (SOFTMAX) p_sm_add(acc[1 - P], s - 11);
                } else if constexpr (s == 27) {
                    p_rest(acc[1 - P], u - 1);
                } else if constexpr (s == 28 && P == 0) {
                    p_share();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    };
    using yes = std::true_type;
    using no = std::false_type;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;

    // prologue: units 0..2 in flight, the first three fragments of unit 0
#pragma unroll 1
    for (int pre = 0; pre < 3; ++pre)
        if (pre < nunits) {
            fill_unit(pre);
#pragma unroll
            for (int p = 0; p < 4; ++p) fill(p);
        }
    if (nunits > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");            // unit 0 has landed
    else if (nunits > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    RB_RD(fr[0], 0, 0);
    RB_RD(fr[1], 1, 0);
    RB_RD(fr[2], 2, 0);
    RB_WAIT(2, fr[0]);

    body(no{}, P0{}, 0);
    int u = 1;
    for (; u + 1 < nunits; u += 2) {
        body(yes{}, P1{}, u);
        body(yes{}, P0{}, u + 1);
    }
    const bool odd_tail = u < nunits;
    if (odd_tail) body(yes{}, P1{}, u);
    // epilogue of the last unit (the only one with padded names), not hidden behind anything; in place on its accumulator set
    auto tail = [&](auto parity) {
        constexpr int P = decltype(parity)::value;
        asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc[P]));                  // MFMA -> VALU read
        const int lu = nunits - 1;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((long long)name_of(lu, i) >= v) acc[P][i] = RB_NEG;
#pragma unroll
        for (int i = 0; i < 16; ++i) p_top2(acc[P], i);
        tk = widen(m1, lu);
        p_ins_all();
        p_rest(acc[P], lu);
        if (SOFTMAX) {
            p_sm_begin();
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if ((long long)name_of(lu, i) < v) smz += __builtin_amdgcn_exp2f(fmaf(acc[P][i], c2, nmc));
        }
    };
    if (odd_tail) tail(P1{});
    else tail(P0{});
    if (img < n) {
        const long long orow = (long long)part * part_rows + (img - out_row0);
        float* cv = cand_val + (orow * 2 + hh) * TM;
        int* ci = cand_idx + (orow * 2 + hh) * TM;
#pragma unroll
        for (int j = 0; j < TM; ++j) {
            const int idx = __double2loint(L[j]);
            const bool ok = L[j] > -INFINITY && (long long)idx < v;
            cv[j] = ok ? (float)L[j] * scale : -INFINITY;
            ci[j] = ok ? idx + (int)v_lo : -1;
        }
        if (SOFTMAX) {
            stats[(orow * 2 + hh) * 2] = smm * scale;
            stats[(orow * 2 + hh) * 2 + 1] = smz;
        }
    }
#undef RB_RD
#undef RB_WAIT
#undef RB_MFMA
#undef RB_MFMA0
}
// The two vocabulary parts of a split row block into the image's two half lists: list h = the TM best of (part 0's list h, part 1's
// list h), (value desc, index asc).  Everything a part dropped is bounded by ITS lists' entries, and the merged list dominates both
// parts' lists entry by entry, so sim_refine4_kernel's certificate (list_h[TM-1], max(list_A[KS], list_B[KS]) - 3.9 E) holds for the
// merged lists as it does for a block that saw the whole vocabulary.  Softmax (max, sum) pairs are combined per half.
__global__ void __launch_bounds__(256) sim_split_merge_kernel(const float* __restrict__ pval, const int* __restrict__ pidx,
                                                              const float* __restrict__ pstats, long long row0, long long n, long long part_rows,
                                                              int tm, int softmax, float* __restrict__ cand_val, int* __restrict__ cand_idx,
                                                              float* __restrict__ stats) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long img = row0 + (t >> 1);
    const int hh = (int)(t & 1);
    if (img >= n) return;
    const long long o0 = ((img - row0) * 2 + hh), o1 = ((part_rows + img - row0) * 2 + hh);
    const float* a = pval + o0 * tm; const int* ai = pidx + o0 * tm;
    const float* b = pval + o1 * tm; const int* bi = pidx + o1 * tm;
    float* cv = cand_val + (img * 2 + hh) * tm;
    int* ci = cand_idx + (img * 2 + hh) * tm;
    int x = 0, y = 0;
    for (int j = 0; j < tm; ++j) {
        const bool ha = x < tm && ai[x] >= 0, hb = y < tm && bi[y] >= 0;
        const bool take_a = ha && (!hb || a[x] > b[y] || (a[x] == b[y] && ai[x] < bi[y]));
        if (take_a) { cv[j] = a[x]; ci[j] = ai[x]; ++x; }
        else if (hb) { cv[j] = b[y]; ci[j] = bi[y]; ++y; }
        else { cv[j] = -INFINITY; ci[j] = -1; }
    }
    if (softmax) {
        const float m0 = pstats[o0 * 2], z0 = pstats[o0 * 2 + 1], m1 = pstats[o1 * 2], z1 = pstats[o1 * 2 + 1];
        const float mm = fmaxf(m0, m1);
        stats[(img * 2 + hh) * 2] = mm;
        stats[(img * 2 + hh) * 2 + 1] = (m0 > -INFINITY ? z0 * __expf(m0 - mm) : 0.f) + (m1 > -INFINITY ? z1 * __expf(m1 - mm) : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------
// Row-block kernel on 16x16x32 tiles (round 3; default at d == 512 for k <= 3).  Ring, fills, keys and lists as in
// sim_topk_rb8_kernel (eight waves, 32 images per wave, units of 32 names x K = 512, one barrier per unit), different matrix
// instruction: on random operands this chip holds 1.65 GHz through a v_mfma_f32_16x16x32_f16 loop fed by ds_read_b128 and 1.41 GHz
// through the 32x32x16 loop at the same cycles per FLOP (tools/micro/mfma_rate.hip: 1616 vs 1439 TFLOP/s), and the bare loop of the
// rb8 kernel runs 8 % faster on it (profiles/r03_sim_ablations.txt).  What changes with the tile:
//   * a unit is 16 k32-steps x (2 name tiles x 2 image tiles) = 64 MFMAs per wave on four 4-register accumulators; the A fragment of
//     name tile tj / step ks is row 16 tj + (l & 15), 16-B chunk 4 ks + (l >> 4) of the slot (chunk ^ (row & 15) swizzle as before:
//     conflict-free, FOUR per-lane address registers instead of eight); the B fragments are [ks][ti] in 128 AGPRs;
//   * a lane holds, per unit, 8 values of TWO images (16 ti + (l & 15)): names 16 tj + 4 (l >> 4) + e.  So a lane keeps two lists,
//     each over a QUARTER of the vocabulary, and the four lanes of an image (l, l ^ 16, l ^ 32, l ^ 48) share their admission
//     threshold through v_permlane16_swap / v_permlane32_swap;
//   * lists hold TM entries, the best four of each leave the kernel (16 candidates per image, the lane layout of
//     sim_refine4_kernel) together with ONE bound per image: the largest approximate value any name outside the 16 can have
//     (the lists' last entries and the shared threshold).  The refine pass certifies against that number.
// Epilogue of unit u - 1, dealt over the 64 MFMAs of unit u (h = 4 ks + m):
//   h  4..19  one value into the (largest, second) key pair of image tile h & 1
//   h 20, 21  widen the winners; softmax reference maxima
//   h 22..    one list entry per slot (tile 0, then tile 1) and, h 22..37, one softmax term per slot
//   h 40, 44  the rare second-key paths;  h 48 (every other unit): thresholds exchanged between the four lanes of an image
__device__ __forceinline__ float rc_swap16(float v, int lane) {         // the value held by lane l ^ 16
    const unsigned u = __float_as_uint(v);
    const auto p = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float((lane & 16) ? p[0] : p[1]);
}
template <bool SOFTMAX, int TM, int KS>
__global__ void __launch_bounds__(512) sim_topk_rc_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt, long long n,
                                                          long long v, float scale, float* __restrict__ cand_val,
                                                          int* __restrict__ cand_idx, float* __restrict__ stats,
                                                          float* __restrict__ bound, const unsigned* __restrict__ wmax2_bits) {
    constexpr int D = 512, UB = 32768;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int jl = lane & 15, g = lane >> 4;
    const unsigned sbase = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

    half8 bf[16][2];                                           // [k32 step][image tile]
    float f2[2] = {0.f, 0.f};
    long long img[2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) img[ti] = (long long)blockIdx.x * 256 + wave * 32 + 16 * ti + jl;
    {
        const half_t* frow0 = F + (img[0] < n ? img[0] : n - 1) * D + 8 * g;
        const half_t* frow1 = F + (img[1] < n ? img[1] : n - 1) * D + 8 * g;
#pragma unroll
        for (int b = 0; b < 4; ++b) {                          // eight fragments at a time (see sim_topk_rb8_kernel)
#pragma unroll
            for (int ks = 4 * b; ks < 4 * b + 4; ++ks) {
                bf[ks][0] = *(const half8*)(frow0 + 32 * ks);
                bf[ks][1] = *(const half8*)(frow1 + 32 * ks);
            }
#pragma unroll
            for (int ks = 4 * b; ks < 4 * b + 4; ++ks)
#pragma unroll
                for (int ti = 0; ti < 2; ++ti)
#pragma unroll
                    for (int q = 0; q < 8; ++q) f2[ti] = fmaf((float)bf[ks][ti][q], (float)bf[ks][ti][q], f2[ti]);
#pragma unroll
            for (int ks = 4 * b; ks < 4 * b + 4; ++ks) {
                asm volatile("" : "+a"(bf[ks][0]) : : "memory");
                asm volatile("" : "+a"(bf[ks][1]) : : "memory");
            }
        }
    }
    // 4 E of the wave's largest image (a scalar register; per lane it was spilled, and its reload in the loop drained the ring)
    float e4;
    {
        float fm = fmaxf(f2[0] + rc_swap16(f2[0], lane), f2[1] + rc_swap16(f2[1], lane));
        fm += rb_swap32(fm, lane);                             // >= both images' squared norms (cheap upper bound: one exchange less)
        fm = wave_max_f32(fm);
        const float e = RB8_EMARGIN * 1.5f * ((float)D * 5.9604645e-8f + 2.4e-7f + 2.0e-6f) * sqrtf(fm) * sqrtf(__uint_as_float(*wmax2_bits)) * 1.001f + 1e-30f;
        int e4i;                                               // asm: the builtin is folded into the arithmetic above and the value re-derived in a VGPR
        asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(e4i) : "v"(__float_as_int(e)));
        e4 = __int_as_float(e4i);
    }
    // State per image tile: the list, the shared threshold and the softmax pair; everything else (key pair, widened winner) is
    // scratch of the tile being worked on - the two tiles of a unit are served one after the other so that it is (117 VGPRs with
    // both tiles' scratch alive at once, and the softmax variant spilled B fragments).
    double L[2][TM];                                           // per image tile: the lane's TM best (key | name index), descending
    float tsh[2] = {-INFINITY, -INFINITY};                     // (largest entry KS of the image's four lanes) - 4 E
    float nm[2] = {INFINITY, INFINITY}, smz[2] = {0.f, 0.f};   // softmax: nm = -(reference maximum) * c2, sum relative to it
    float m1, m2;
    double tk;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int j = 0; j < TM; ++j) L[ti][j] = -INFINITY;
    const float c2 = scale * 1.4426950408889634f;

    const int nunits = (int)((v + 31) / 32);
    const unsigned bsw = (unsigned)((lane ^ ((4 * wave) & 12)) << 4);
    const half_t* fbase = Wt;
    unsigned fm0 = 0;
    int frows = 32;
    auto fill_unit = [&](int unit) {
        fbase = Wt + (size_t)unit * 32 * D;
        fm0 = sbase + (unit & 3) * UB + 4 * wave * 1024;
        const long long left = v - (long long)unit * 32;
        frows = left < 32 ? (int)left : 32;
    };
    auto fill = [&](int p) {
        int srow = 4 * wave + p;
        srow = srow < frows ? srow : frows - 1;
        const unsigned off = (bsw ^ (unsigned)(p << 4)) + (unsigned)srow * 1024u;
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2"
                     ::"s"(fm0 + p * 1024), "v"(off), "s"(fbase) : "memory");
    };
    // A fragment (tj, ks = 4 a + b): fa[b] + a * 256 + tj * 16384
    unsigned fa[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) fa[b] = sbase + (unsigned)(jl * 1024 + (((4 * b + g) ^ jl) << 4));

#define RC_RD(DST, B, IMM) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(DST) : "v"(fa[B]), "n"(IMM))
#define RC_WAIT(N, FR) asm volatile("s_waitcnt lgkmcnt(" #N ")" : "+v"(FR))
#define RC_MFMA(ACC, A, B) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(ACC) : "v"(A), "a"(B))
#define RC_MFMA0(ACC, A, B) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(ACC) : "v"(A), "a"(B))

    auto key = [](float a, int p) { return __uint_as_float((__float_as_uint(a) & 0xfffffff8u) | (unsigned)p); };
    auto name_of = [&](int unit, int p) { return unit * 32 + 16 * (p >> 2) + 4 * g + (p & 3); };
    // value p = 4 tj + e of image tile ti sits in acc[tj][ti][e]
    auto p_top2 = [&](float a, int p) {
        const float kk = key(a, p);
        if (p == 0) {
            m1 = kk;
            m2 = -INFINITY;
        } else {
            const float n1 = rb_max(m1, kk);
            m2 = rb_med3(m1, m2, kk);
            m1 = n1;
        }
    };
    auto widen = [&](float kk, int unit) {
        const int p = (int)(__float_as_uint(kk) & 7u);
        return __hiloint2double(__double2hiint((double)kk), name_of(unit, p));
    };
    auto p_ins = [&](int ti, int j) {
        const double hi = rb_max64(L[ti][j], tk);
        if (j + 1 < TM) tk = rb_min64(L[ti][j], tk);
        L[ti][j] = hi;
    };
    auto p_ins_all = [&](int ti) {
#pragma unroll
        for (int j = 0; j < TM; ++j) p_ins(ti, j);
    };
    auto te_of = [&](int ti) { return rb_max((float)L[ti][TM - 1], tsh[ti]); };    // what a value of tile ti has to beat
    auto p_share = [&](int ti) {                               // the four lanes of an image: the largest of their entries KS
        float t = (float)L[ti][KS];
        t = rb_max(t, rc_swap16(t, lane));
        t = rb_max(t, rb_swap32(t, lane));
        tsh[ti] = t - e4;
    };
    f32x4 acc[2][2][2];                                        // [parity][name tile][image tile]
    half8 fr[4];                                               // fragment s = 2 ks + tj lives in fr[s & 3] (three in flight)
    auto p_rest = [&](auto parity, auto tic, int unit) {       // rare: the lane's second key beats what it has to beat as well
        constexpr int Q = decltype(parity)::value, ti = decltype(tic)::value;
        float te = te_of(ti);
        if (!__any(m2 > te)) return;
        tk = m2 > te ? widen(m2, unit) : (double)-INFINITY;
        p_ins_all(ti);
        te = te_of(ti);
        int cnt = 0;
#pragma unroll
        for (int p = 0; p < 8; ++p) cnt += key(acc[Q][p >> 2][ti][p & 3], p) > te ? 1 : 0;
        if (!__any(cnt > 2)) return;
        float bnd = m2;
        for (;;) {
            float c = -INFINITY;
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const float kk = key(acc[Q][p >> 2][ti][p & 3], p);
                c = (kk < bnd && kk > c) ? kk : c;
            }
            if (!__any(c > te)) break;
            if (c > te) {
                tk = widen(c, unit);
                p_ins_all(ti);
            }
            te = te_of(ti);
            bnd = c;
        }
    };
    auto p_sm_begin = [&](int ti) {                            // new reference maximum, old sum rescaled to it
        const float t = -m1 * c2;
        const float nn = fminf(nm[ti], t);
        smz[ti] = smz[ti] * __builtin_amdgcn_exp2f(nn - nm[ti]);                 // first unit: 0 * exp2(-inf) = 0
        nm[ti] = nn;
    };
    auto p_sm_add = [&](float a, int ti) { smz[ti] += __builtin_amdgcn_exp2f(fmaf(a, c2, nm[ti])); };

    using yes = std::true_type;
    using no = std::false_type;
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    auto body = [&](auto has_prev, auto parity, int u) {
        constexpr int P = decltype(parity)::value;
        constexpr bool EPI = decltype(has_prev)::value;
        using PREV = std::integral_constant<int, 1 - P>;
        if (u + 2 < nunits) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const bool more = u + 1 < nunits;
        const bool fills = u + 3 < nunits;
        if (fills) fill_unit(u + 3);
        static_for<0, 32>([&](auto sc_) {
            // fragment step s = 2 ks + tj: two MFMAs (image tiles 0, 1).  Reads run three fragments ahead; the wait of step s
            // retires the fragment of step s + 1 (a whole step before its first use)
            constexpr int s = decltype(sc_)::value, ks = s >> 1, tj = s & 1;
            if (s == 29) {
                const unsigned delta = ((u + 1) & 3) ? (unsigned)UB : (unsigned)(-3 * UB);      // wave-uniform
#pragma unroll
                for (int b = 0; b < 4; ++b) fa[b] += delta;
            }
            constexpr int sn = (s + 3) & 31, kn = sn >> 1;      // fragment being fetched (of unit u + 1 when s >= 29)
            if (s < 29 || more) RC_RD(fr[(s + 3) & 3], kn & 3, (kn >> 2) * 256 + (sn & 1) * 16384);
            if (s < 29 || more) RC_WAIT(2, fr[(s + 1) & 3]);
            else if (s == 29) RC_WAIT(1, fr[(s + 1) & 3]);
            else if (s == 30) RC_WAIT(0, fr[(s + 1) & 3]);
            static_for<0, 2>([&](auto tc) {
                constexpr int ti = decltype(tc)::value, h = 2 * s + ti;
                if (ks == 0) RC_MFMA0(acc[P][tj][ti], fr[s & 3], bf[ks][ti]);
                else RC_MFMA(acc[P][tj][ti], fr[s & 3], bf[ks][ti]);
                if ((h & 15) == 15 && fills) fill(h >> 4);
                if constexpr (EPI) {
                    // tile t2 = h / 20 (h < 40): its slots are h0 = h - 20 t2 - 4: 0..7 key pair, 8 widen, 9.. list entries and,
                    // 9..16, softmax terms, 18 the second-key path
                    constexpr int t2 = h >= 24 ? 1 : 0, h0 = h - 20 * t2 - 4;
                    if constexpr (h >= 4 && h < 44) {
                        if constexpr (h0 >= 0 && h0 < 8) {
                            p_top2(acc[1 - P][h0 >> 2][t2][h0 & 3], h0);
                        } else if constexpr (h0 == 8) {
                            tk = widen(m1, u - 1);
                            if (SOFTMAX) p_sm_begin(t2);
                        }
                        if constexpr (h0 >= 9 && h0 < 9 + TM) p_ins(t2, h0 - 9);
                        if constexpr (h0 >= 9 && h0 < 17) {
                            if (SOFTMAX) p_sm_add(acc[1 - P][(h0 - 9) >> 2][t2][(h0 - 9) & 3], t2);
                        }
                        if constexpr (h0 == 18) {
                            if constexpr (t2 == 0) p_rest(PREV{}, P0{}, u - 1);
                            else p_rest(PREV{}, P1{}, u - 1);
                        }
                    }
                    // (two slots: in one, hipcc packs the two subtractions into a v_pk_add_f32 whose (e4, e4) operand it then spills)
                    if constexpr (h == 48 && P == 0) p_share(0);
                    if constexpr (h == 50 && P == 0) p_share(1);
                }
                __builtin_amdgcn_sched_barrier(0);
            });
        });
    };
#pragma unroll 1
    for (int pre = 0; pre < 3; ++pre)
        if (pre < nunits) {
            fill_unit(pre);
#pragma unroll
            for (int p = 0; p < 4; ++p) fill(p);
        }
    if (nunits > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (nunits > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    RC_RD(fr[0], 0, 0);
    RC_RD(fr[1], 0, 16384);
    RC_RD(fr[2], 1, 0);
    RC_WAIT(2, fr[0]);

    body(no{}, P0{}, 0);
    int u = 1;
    for (; u + 1 < nunits; u += 2) {
        body(yes{}, P1{}, u);
        body(yes{}, P0{}, u + 1);
    }
    const bool odd_tail = u < nunits;
    if (odd_tail) body(yes{}, P1{}, u);
    // epilogue of the last unit (the only one with padded names), not hidden behind anything; in place on its accumulator set
    auto tail = [&](auto parity) {
        constexpr int P = decltype(parity)::value;
        asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc[P][0][0]), "+v"(acc[P][0][1]), "+v"(acc[P][1][0]), "+v"(acc[P][1][1]));
        const int lu = nunits - 1;
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) {
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if ((long long)name_of(lu, p) >= v) acc[P][p >> 2][ti][p & 3] = RB_NEG;
#pragma unroll
            for (int p = 0; p < 8; ++p) p_top2(acc[P][p >> 2][ti][p & 3], p);
            tk = widen(m1, lu);
            p_ins_all(ti);
            if (ti == 0) p_rest(parity, P0{}, lu);
            else p_rest(parity, P1{}, lu);
            if (SOFTMAX) {
                p_sm_begin(ti);
#pragma unroll
                for (int p = 0; p < 8; ++p)
                    if ((long long)name_of(lu, p) < v) smz[ti] += __builtin_amdgcn_exp2f(fmaf(acc[P][p >> 2][ti][p & 3], c2, nm[ti]));
            }
        }
    };
    if (odd_tail) tail(P1{});
    else tail(P0{});
    // the best four of each list leave the kernel: candidate slot 4 g + j of the image; everything else is below `bound`
#pragma unroll
    for (int ti = 0; ti < 2; ++ti) {
        p_share(ti);                                            // the final threshold: every lane of the image holds the same one
        float bq = rb_max(tsh[ti], (float)L[ti][TM - 1]);       // dropped by the threshold, or pushed out of / never into the list
        bq = rb_max(bq, rc_swap16(bq, lane));
        bq = rb_max(bq, rb_swap32(bq, lane));
        if (img[ti] < n) {
            float* cv = cand_val + (img[ti] * 4 + g) * 4;
            int* ci = cand_idx + (img[ti] * 4 + g) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool have = j < TM;
                const double e = have ? L[ti][j < TM ? j : 0] : (double)-INFINITY;
                const int idx = __double2loint(e);
                const bool ok = have && e > -INFINITY && (long long)idx < v;
                cv[j] = ok ? (float)e * scale : -INFINITY;
                ci[j] = ok ? idx : -1;
            }
            if (g == 0) bound[img[ti]] = bq > -INFINITY ? bq * scale : -INFINITY;
            if (SOFTMAX) {
                stats[(img[ti] * 4 + g) * 2] = -nm[ti] * 0.6931471805599453f;   // reference maximum * scale = -nm / log2(e)
                stats[(img[ti] * 4 + g) * 2 + 1] = smz[ti];
            }
        }
    }
#undef RC_RD
#undef RC_WAIT
#undef RC_MFMA
#undef RC_MFMA0
}

// max ||w_v||^2 over the vocabulary (error-bound scale), one wave per row
__global__ void __launch_bounds__(256) wmax_kernel(const half_t* __restrict__ Wt, long long v, int d, unsigned* out_bits) {
    // 16 lanes per row (8 below d = 128), each with d / 128 16-B pieces (whole 256-B segments per load instruction and row), eight
    // rows per wave in flight and a four-step butterfly: one wave per row with a 64-lane butterfly was latency-bound (14 us at V = 21,000)
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lpr = d >= 128 ? 16 : 8, rpw = 64 / lpr, sub = lane / lpr, jl = lane % lpr;
    float best = 0.f;
    for (long long row0 = ((long long)blockIdx.x * 4 + wave) * 2 * rpw; row0 < v; row0 += (long long)gridDim.x * 4 * 2 * rpw) {
        float sacc[2] = {0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long long row = row0 + t * rpw + sub;
            if (row < v)
                for (int j = jl * 8; j < d; j += lpr * 8) {
                    const half8 w8 = *(const half8*)(Wt + row * d + j);
#pragma unroll
                    for (int q = 0; q < 8; ++q) sacc[t] = fmaf((float)w8[q], (float)w8[q], sacc[t]);
                }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float sv = sacc[t];
            for (int o = lpr >> 1; o > 0; o >>= 1) sv += __shfl_xor(sv, o, 64);
            best = fmaxf(best, sv);
        }
    }
    best = wave_max_f32(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * 1.0001f));
}

struct SimHdr {
    unsigned wmax2_bits;
    int fb_cnt;
    int pad[14];
};

// exact float64 dot of one image row with one vocabulary row, all 64 lanes
__device__ __forceinline__ double dot64(const half_t* f, const half_t* w, int d, int lane) {
    double s = 0.0;
    for (int j = lane * 8; j < d; j += 512) {
        const half8 a = *(const half8*)(f + j);
        const half8 b = *(const half8*)(w + j);
#pragma unroll
        for (int q = 0; q < 8; ++q) s = fma((double)(float)a[q], (double)(float)b[q], s);
    }
    return wave_sum_f64(s);
}

// pass 2: one wave per image (TOPM = entries per half list: 8, or 4 for k <= 3)
template <bool SOFTMAX, int TM>
__global__ void __launch_bounds__(256) sim_refine_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt,
                                                         long long n, int d, long long v, float scale, int k,
                                                         const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                         const float* __restrict__ stats, SimHdr* hdr, int* fb_list,
                                                         long long* idx_out, float* val_out, int ks) {
    const int lane = threadIdx.x & 63;
    const long long img = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (img >= n) return;
    const half_t* f = F + img * d;
    // lanes 0..15 own one candidate each
    int myi = -1;
    float mya = -INFINITY;
    if (lane < 2 * TM) {
        myi = cand_idx[img * 2 * TM + lane];
        mya = cand_val[img * 2 * TM + lane];
    }
    double mye = -INFINITY;
    unsigned long long needm = __ballot(myi >= 0);                  // candidates whose exact value is computed and ranked
    double f2 = 0.0;
    for (int j = lane; j < d; j += 64) {
        const double x = (double)(float)f[j];
        f2 = fma(x, x, f2);
    }
    f2 = wave_sum_f64(f2);
    const float wmax = sqrtf(__uint_as_float(hdr->wmax2_bits));
    // |approx - exact| <= E: fp32 accumulation of exact fp16 products + the key bits of the row-block kernel (< 2^-20 relative)
    const float E = 1.5f * fabsf(scale) * ((float)d * 5.9604645e-8f + 2.4e-7f + 2.0e-6f) * (float)sqrt(f2) * wmax + 1e-30f;
    if (d <= 512) {
        // Only candidates that can still reach rank k are recomputed: with A_k the k-th largest APPROXIMATE value, a candidate
        // below A_k - 2E has an exact value below A_k - E <= the exact values of k others.  That is typically k+1 of the 2 TM
        // rows, and the row gather (1 KB per candidate from L2 / Infinity Cache) is what this kernel's time is made of.
        int ra = 0;
        for (int c = 0; c < 2 * TM; ++c) {
            const float oa = __shfl(mya, c, 64);
            const int oi = __shfl(myi, c, 64);
            if (oi >= 0 && (oa > mya || (oa == mya && c < lane))) ++ra;
        }
        float kap = -INFINITY;
        {
            const unsigned long long m = __ballot(ra == k - 1 && myi >= 0);
            if (m) kap = __shfl(mya, __ffsll((long long)m) - 1, 64);
        }
        needm = __ballot(myi >= 0 && mya >= kap - 2.f * E);
        // all needed candidate rows are requested before the first is consumed (a loop with one load per iteration paid one
        // L2 latency per candidate); lane l owns columns 8l .. 8l+7 of the image row and of every candidate row
        half8 fv, wv[2 * TM];
        const bool act = lane * 8 < d;
#pragma unroll
        for (int q = 0; q < 8; ++q) fv[q] = (half_t)0.f;
        if (act) fv = *(const half8*)(f + lane * 8);
#pragma unroll
        for (int c = 0; c < 2 * TM; ++c) {
            const int ci = __shfl(myi, c, 64);
            wv[c] = fv;
            if (act && (needm >> c & 1)) wv[c] = *(const half8*)(Wt + (long long)ci * d + lane * 8);
        }
#pragma unroll
        for (int c = 0; c < 2 * TM; ++c) {
            if (!(needm >> c & 1)) continue;                        // wave-uniform
            double sacc = 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q) sacc = fma((double)(float)fv[q], (double)(float)wv[c][q], sacc);
            const double e = (double)scale * wave_sum_f64(act ? sacc : 0.0);
            if (lane == c) mye = e;
        }
    } else {
        for (int c = 0; c < 2 * TM; ++c) {
            const int ci = __shfl(myi, c, 64);
            if (ci < 0) continue;                                   // wave-uniform
            const double e = (double)scale * dot64(f, Wt + (long long)ci * d, d, lane);
            if (lane == c) mye = e;
        }
    }
    // rank of each recomputed candidate among them: (value desc, index asc)
    const bool need_l = needm >> lane & 1;
    int rank = 0;
    for (int c = 0; c < 2 * TM; ++c) {
        const double oe = __shfl(mye, c, 64);
        const int oi = __shfl(myi, c, 64);
        if ((needm >> c & 1) && (oe > mye || (oe == mye && oi < myi))) ++rank;
    }
    // certification: a non-candidate of half h has approx <= list_h[TM-1]
    const float a0 = __shfl(mya, TM - 1, 64), a1 = __shfl(mya, 2 * TM - 1, 64);
    const int i0 = __shfl(myi, TM - 1, 64), i1 = __shfl(myi, 2 * TM - 1, 64);
    // if a list is not full, that half has no non-candidates at all
    float astar = -INFINITY;
    if (i0 >= 0) astar = fmaxf(astar, a0);
    if (i1 >= 0) astar = fmaxf(astar, a1);
    // sim_topk_rb8_kernel also drops what lies 4.2 E below the other half list's entry ks (ks < 0: the other kernels do not)
    if (ks >= 0) astar = fmaxf(astar, fmaxf(__shfl(mya, ks, 64), __shfl(mya, TM + ks, 64)) - 3.9f * E);
    // exact value of the k-th ranked candidate
    double kth = -INFINITY;
    {
        const unsigned long long m = __ballot(rank == k - 1 && need_l);
        if (m) kth = __shfl(mye, __ffsll((long long)m) - 1, 64);
    }
    const bool certified = (astar == -INFINITY) || (kth > (double)astar + (double)E);
    if (!certified) {
        if (lane == 0) {
            const int pos = atomicAdd(&hdr->fb_cnt, 1);
            fb_list[pos] = (int)img;
        }
        return;
    }
    if (need_l && rank < k) {
        idx_out[img * k + rank] = myi;
        float o = (float)mye;
        if (SOFTMAX) {
            const float m0 = stats[img * 4], z0 = stats[img * 4 + 1], m1 = stats[img * 4 + 2], z1 = stats[img * 4 + 3];
            const float mm = fmaxf(m0, m1);
            const float z = z0 * __expf(m0 - mm) + z1 * __expf(m1 - mm);
            o = __expf((float)mye - mm) / z;
        }
        val_out[img * k + rank] = o;
    }
}

// pass 2 at d == 512 (round 3): FOUR images per wave, 16 lanes each - lane j of a group owns candidate j (2 TM <= 16), the group's
// lanes split an image / vocabulary row into 4 x 16-B pieces per lane (whole 256-B segments per load instruction and group), the
// float64 dot products reduce over 16 lanes (four butterfly steps instead of six) and every ranking step serves four images.  Same
// decisions as sim_refine_kernel: which candidates are recomputed (approximate value within 2 E of the k-th largest), (value desc,
// index asc) order, the certificate against the lists' last entries and the shared threshold of sim_topk_rb8_kernel (ks).
__device__ __forceinline__ double grp16_sum_f64(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <bool SOFTMAX, int TM>
__global__ void __launch_bounds__(256) sim_refine4_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt,
                                                          long long n, long long v, float scale, int k,
                                                          const float* __restrict__ cand_val, const int* __restrict__ cand_idx,
                                                          const float* __restrict__ stats, SimHdr* hdr, int* fb_list,
                                                          long long* idx_out, float* val_out, int ks,
                                                          const float* __restrict__ bound, int nstat) {
    constexpr int D = 512, NC = 2 * TM;
    const int lane = threadIdx.x & 63, j = lane & 15, gb = lane & 48;
    const long long img0 = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    const bool live = img0 < n;
    const long long img = live ? img0 : n - 1;
    int myi = -1;
    float mya = -INFINITY;
    if (j < NC) {
        myi = cand_idx[img * NC + j];
        mya = cand_val[img * NC + j];
    }
    half8 fv[4];
    const half_t* f = F + img * D + 8 * j;
#pragma unroll
    for (int q = 0; q < 4; ++q) fv[q] = *(const half8*)(f + 128 * q);
    double f2 = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double x = (double)(float)fv[q][e];
            f2 = fma(x, x, f2);
        }
    f2 = grp16_sum_f64(f2);
    const float wmax = sqrtf(__uint_as_float(hdr->wmax2_bits));
    const float E = 1.5f * fabsf(scale) * ((float)D * 5.9604645e-8f + 2.4e-7f + 2.0e-6f) * (float)sqrt(f2) * wmax + 1e-30f;
    // the k-th largest approximate value of the image
    int ra = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float oa = __shfl(mya, gb | c, 64);
        const int oi = __shfl(myi, gb | c, 64);
        if (oi >= 0 && (oa > mya || (oa == mya && c < j))) ++ra;
    }
    float kap;
    {
        const unsigned gm = (unsigned)(__ballot(ra == k - 1 && myi >= 0) >> gb) & 0xffffu;
        const float t = __shfl(mya, gm ? (gb | (__ffs((int)gm) - 1)) : lane, 64);
        kap = gm ? t : -INFINITY;
    }
    const unsigned need = (unsigned)(__ballot(myi >= 0 && mya >= kap - 2.f * E) >> gb) & 0xffffu;   // uniform inside a group
    // exact values of the needed candidates, four rows per pass in flight
    double mye = -INFINITY;
    unsigned rem = need;
    while (__any(rem != 0)) {
        int cc[4];
        half8 wv[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            cc[t] = rem ? __ffs((int)rem) - 1 : -1;
            rem = rem ? (rem & (rem - 1)) : 0;
            const int ci = __shfl(myi, gb | (cc[t] >= 0 ? cc[t] : 0), 64);
#pragma unroll
            for (int q = 0; q < 4; ++q) wv[t][q] = fv[q];
            if (cc[t] >= 0) {
                const half_t* w = Wt + (long long)ci * D + 8 * j;
#pragma unroll
                for (int q = 0; q < 4; ++q) wv[t][q] = *(const half8*)(w + 128 * q);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (!__any(cc[t] >= 0)) break;                         // wave-uniform
            double sacc = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 8; ++e) sacc = fma((double)(float)fv[q][e], (double)(float)wv[t][q][e], sacc);
            const double ev = (double)scale * grp16_sum_f64(sacc);
            if (cc[t] == j) mye = ev;
        }
    }
    // rank of each recomputed candidate among them: (value desc, index asc)
    const bool need_l = need >> j & 1;
    int rank = 0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double oe = __shfl(mye, gb | c, 64);
        const int oi = __shfl(myi, gb | c, 64);
        if ((need >> c & 1) && (oe > mye || (oe == mye && oi < myi))) ++rank;
    }
    // certification: a non-candidate of half h has approx <= list_h[TM-1]; a list that is not full has no non-candidates
    const float a0 = __shfl(mya, gb | (TM - 1), 64), a1 = __shfl(mya, gb | (NC - 1), 64);
    const int i0 = __shfl(myi, gb | (TM - 1), 64), i1 = __shfl(myi, gb | (NC - 1), 64);
    float astar = -INFINITY;
    if (i0 >= 0) astar = fmaxf(astar, a0);
    if (i1 >= 0) astar = fmaxf(astar, a1);
    if (ks >= 0) astar = fmaxf(astar, fmaxf(__shfl(mya, gb | ks, 64), __shfl(mya, gb | (TM + ks), 64)) - 3.9f * E);
    if (bound) astar = bound[img];                              // sim_topk_rc_kernel: what a name outside the 16 candidates can reach
    double kth;
    {
        const unsigned gm = (unsigned)(__ballot(rank == k - 1 && need_l) >> gb) & 0xffffu;
        const double t = __shfl(mye, gm ? (gb | (__ffs((int)gm) - 1)) : lane, 64);
        kth = gm ? t : -INFINITY;
    }
    const bool certified = (astar == -INFINITY) || (kth > (double)astar + (double)E);
    if (!live) return;
    if (!certified) {
        if (j == 0) {
            const int pos = atomicAdd(&hdr->fb_cnt, 1);
            fb_list[pos] = (int)img;
        }
        return;
    }
    if (need_l && rank < k) {
        idx_out[img * k + rank] = myi;
        float o = (float)mye;
        if (SOFTMAX) {
            const float* st = stats + img * 2 * nstat;            // nstat (max, sum) pairs: two half lists or four quarter lists
            float mm = st[0];
            for (int q = 1; q < nstat; ++q) mm = fmaxf(mm, st[2 * q]);
            float z = 0.f;
            for (int q = 0; q < nstat; ++q) z += st[2 * q + 1] * __expf(st[2 * q] - mm);
            o = __expf((float)mye - mm) / z;
        }
        val_out[img * k + rank] = o;
    }
}

// pass 3 (rare): exact full-row top-k in float64 for uncertified rows; one block (256 threads) per row
template <bool SOFTMAX>
__global__ void __launch_bounds__(256) sim_exact_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt, int d,
                                                        long long v, float scale, int k, const SimHdr* hdr,
                                                        const int* fb_list, long long* idx_out, float* val_out, int fb0) {
    __shared__ float fs[1024];
    __shared__ double cval[256 * TOPM];
    __shared__ int cidx[256 * TOPM];
    __shared__ double red_m[256];
    __shared__ double red_z[256];
    const int cnt = hdr->fb_cnt;
    for (int fb = fb0 + blockIdx.x; fb < cnt; fb += gridDim.x) {
        const long long img = fb_list[fb];
        __syncthreads();
        for (int j = threadIdx.x; j < d; j += 256) fs[j] = (float)F[img * d + j];
        __syncthreads();
        double lv[TOPM];
        int li[TOPM];
#pragma unroll
        for (int j = 0; j < TOPM; ++j) { lv[j] = -INFINITY; li[j] = -1; }
        double m = -INFINITY, z = 0.0;
        for (long long vi = threadIdx.x; vi < v; vi += 256) {
            const half_t* w = Wt + vi * d;
            double s = 0.0;
            for (int j = 0; j < d; j += 8) {
                const half8 b = *(const half8*)(w + j);
#pragma unroll
                for (int q = 0; q < 8; ++q) s = fma((double)fs[j + q], (double)(float)b[q], s);
            }
            s *= (double)scale;
            if (SOFTMAX) {
                const double mn = s > m ? s : m;
                z = z * exp(m - mn) + exp(s - mn);
                m = mn;
            }
            if (s > lv[TOPM - 1]) {        // ascending vi per thread: strict > keeps the lower index on ties
#pragma unroll
                for (int j = TOPM - 1; j >= 1; --j) {
                    const bool up = s > lv[j - 1];
                    const bool here = s > lv[j];
                    lv[j] = up ? lv[j - 1] : (here ? s : lv[j]);
                    li[j] = up ? li[j - 1] : (here ? (int)vi : li[j]);
                }
                if (s > lv[0]) { lv[0] = s; li[0] = (int)vi; }
            }
        }
#pragma unroll
        for (int j = 0; j < TOPM; ++j) {
            cval[threadIdx.x * TOPM + j] = lv[j];
            cidx[threadIdx.x * TOPM + j] = li[j];
        }
        red_m[threadIdx.x] = m;
        red_z[threadIdx.x] = z;
        __syncthreads();
        if (threadIdx.x == 0) {
            double mm = -INFINITY, zz = 0.0;
            if (SOFTMAX) {
                for (int t = 0; t < 256; ++t) mm = red_m[t] > mm ? red_m[t] : mm;
                for (int t = 0; t < 256; ++t)
                    if (red_z[t] > 0.0) zz += red_z[t] * exp(red_m[t] - mm);
            }
            for (int out = 0; out < k; ++out) {
                int bt = -1;
                for (int t = 0; t < 256 * TOPM; ++t) {
                    if (cidx[t] < 0) continue;
                    if (bt < 0 || cval[t] > cval[bt] || (cval[t] == cval[bt] && cidx[t] < cidx[bt])) bt = t;
                }
                if (bt < 0) break;
                idx_out[img * k + out] = cidx[bt];
                val_out[img * k + out] = SOFTMAX ? (float)(exp(cval[bt] - mm) / zz) : (float)cval[bt];
                cidx[bt] = -1;
            }
        }
    }
}

// Uncertified rows, spread over the whole chip (a handful of rows is the normal case; the one-block-per-row kernel above keeps a
// single CU busy for 1.8 ms per row at V = 21,000, and round 2's one-wave-per-name version of this kernel paid a 1-KB gather and a
// 64-lane float64 butterfly per (row, name): 75 us for two rows, 1.3 ms for twenty).  Block c takes names [128 c, 128 c + 128) of
// EVERY such row: the chunk of W^T is staged ONCE in LDS (rows padded to 1040 B: conflict-free 16-B reads at one name per lane), two
// rows at a time meet it - thread t: name t & 127 of row slot t >> 7 (wave-uniform: the row's fp16 copy in LDS is a broadcast read),
// a 512-term float64 dot product per thread, no cross-lane reduction - and the chunk's TOPM best per row are found by RANK: every
// thread counts the values of its row slot that order before its own ((value desc, name asc); 128 broadcast LDS reads) and the
// threads of rank < TOPM write part[row][chunk].  sim_exact_merge_kernel (one block per row) then selects the row's top k from the
// chunks' lists and, for softmax, combines the (max, sum) pairs in chunk order.  Rows past the cap keep the one-block-per-row kernel.
constexpr int EXC = 128, EX_LDW = 1040;
constexpr int EX_LDS = EXC * EX_LDW + 2 * 1024 + 2 * EXC * 8 + 2 * 4 * 16;
struct ExPart {
    double val[TOPM];
    double m, z;
    int idx[TOPM];
};
static inline int ex_nchunks(long long v) { return (int)((v + EXC - 1) / EXC); }
static inline int ex_rows_cap(long long v) {                     // rows the chunk kernels serve: part[] stays <= 64 MB
    long long r = (64ll << 20) / (long long)sizeof(ExPart) / ex_nchunks(v);
    return (int)(r < 4 ? 4 : (r > 256 ? 256 : r));
}
__device__ __forceinline__ void ex_insert(double (&lv)[TOPM], int (&li)[TOPM], double s, int vi) {
    // candidates arrive in ascending name order or are merged with an explicit index test: (s, -vi) lexicographic
    if (s > lv[TOPM - 1] || (s == lv[TOPM - 1] && li[TOPM - 1] >= 0 && vi < li[TOPM - 1])) {
#pragma unroll
        for (int j = TOPM - 1; j >= 1; --j) {
            const bool up = s > lv[j - 1] || (s == lv[j - 1] && li[j - 1] >= 0 && vi < li[j - 1]);
            const bool here = s > lv[j] || (s == lv[j] && li[j] >= 0 && vi < li[j]);
            lv[j] = up ? lv[j - 1] : (here ? s : lv[j]);
            li[j] = up ? li[j - 1] : (here ? vi : li[j]);
        }
        if (s > lv[0] || (s == lv[0] && li[0] >= 0 && vi < li[0])) { lv[0] = s; li[0] = vi; }
    }
}
template <bool SOFTMAX>
__global__ void __launch_bounds__(256) sim_exact_chunk_kernel(const half_t* __restrict__ F, const half_t* __restrict__ Wt, int d,
                                                              long long v, float scale, const SimHdr* hdr,
                                                              const int* __restrict__ fb_list, ExPart* __restrict__ part,
                                                              int rows_cap, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cnt = hdr->fb_cnt < rows_cap ? hdr->fb_cnt : rows_cap;
    if (cnt <= 0) return;
    char* wl = smem;                                              // [EXC][EX_LDW] bytes
    char* fl = smem + EXC * EX_LDW;                               // [2][1024] bytes
    double* vals = (double*)(fl + 2 * 1024);                      // [2][EXC]
    double* red = vals + 2 * EXC;                                 // [2 slots][2 waves][m, z]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = blockIdx.x;
    const long long v0 = (long long)chunk * EXC;
    const int nv = v - v0 < EXC ? (int)(v - v0) : EXC;
    const int pr = d >> 3;                                        // 16-B pieces per row
    for (int p = tid; p < nv * pr; p += 256) {
        const int row = p / pr, c = p - row * pr;
        *(half8*)(wl + row * EX_LDW + c * 16) = *(const half8*)(Wt + (v0 + row) * d + c * 8);
    }
    const int slot = tid >> 7, name = tid & 127;
    for (int fb0 = 0; fb0 < cnt; fb0 += 2) {
        __syncthreads();                                          // W staged / the previous pair is done with fl, vals, red
        for (int p = tid; p < 2 * pr; p += 256) {
            const int rr = p / pr, c = p - rr * pr;
            if (fb0 + rr < cnt) *(half8*)(fl + rr * 1024 + c * 16) = *(const half8*)(F + (long long)fb_list[fb0 + rr] * d + c * 8);
        }
        __syncthreads();
        const int fb = fb0 + slot;                                // wave-uniform
        const bool active = fb < cnt && name < nv;
        double sv = -INFINITY;
        if (active) {
            double acc = 0.0;
            for (int j = 0; j < pr; ++j) {
                const half8 a = *(const half8*)(fl + slot * 1024 + j * 16);
                const half8 w8 = *(const half8*)(wl + name * EX_LDW + j * 16);
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = fma((double)(float)a[q], (double)(float)w8[q], acc);
            }
            sv = acc * (double)scale;
        }
        vals[slot * EXC + name] = sv;
        ExPart* o = part + (size_t)(fb < cnt ? fb : 0) * nchunks + chunk;
        if (fb < cnt && name < TOPM) { o->val[name] = -INFINITY; o->idx[name] = -1; }       // ranks nobody takes (NaN, short chunk)
        double m = -INFINITY, z = 0.0;
        if (SOFTMAX && fb < cnt) {                               // (max, sum) of the chunk: wave butterfly, then the slot's two waves
            m = sv;                                               // NaN never becomes the maximum; it does poison the sum, as exp() would
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double om = __shfl_xor(m, off, 64);
                m = om > m ? om : m;
            }
            if (lane == 0) red[(slot * 2 + (wave & 1)) * 2] = m;
        }
        __syncthreads();
        if (fb < cnt) {
            if (SOFTMAX) {
                const double m0 = red[(slot * 2) * 2], m1 = red[(slot * 2 + 1) * 2];
                m = m1 > m0 ? m1 : m0;
                z = active ? exp(sv - m) : 0.0;
                if (m == -INFINITY) z = 0.0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
                if (lane == 0) red[(slot * 2 + (wave & 1)) * 2 + 1] = z;
            }
            int rank = 1 << 20;
            if (active && sv == sv) {                             // NaN never enters
                rank = 0;
                for (int o2 = 0; o2 < nv; ++o2) {
                    const double ov = vals[slot * EXC + o2];
                    rank += (ov > sv || (ov == sv && o2 < name)) ? 1 : 0;
                }
            }
            if (rank < TOPM) { o->val[rank] = sv; o->idx[rank] = (int)(v0 + name); }
        }
        if (SOFTMAX) {
            __syncthreads();
            if (fb < cnt && name == 0) {
                o->m = m;
                o->z = red[(slot * 2) * 2 + 1] + red[(slot * 2 + 1) * 2 + 1];
            }
        }
    }
}
template <bool SOFTMAX>
__global__ void __launch_bounds__(256) sim_exact_merge_kernel(const SimHdr* hdr, const int* __restrict__ fb_list, const ExPart* __restrict__ part,
                                                              int k, long long* idx_out, float* val_out, int rows_cap, int nchunks) {
    __shared__ double rv[4];
    __shared__ int ri[4], rt[4];
    __shared__ double sm[256], sz[256];
    const int cnt = hdr->fb_cnt < rows_cap ? hdr->fb_cnt : rows_cap;
    const int fb = blockIdx.x;
    if (fb >= cnt) return;
    const long long img = fb_list[fb];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double cv[TOPM];
    int ci[TOPM];
#pragma unroll
    for (int j = 0; j < TOPM; ++j) { cv[j] = -INFINITY; ci[j] = -1; }
    double tm = -INFINITY, tz = 0.0;
    for (int c = t; c < nchunks; c += 256) {                    // chunks in ascending order per thread
        const ExPart* pp = part + (size_t)fb * nchunks + c;
#pragma unroll
        for (int j = 0; j < TOPM; ++j)
            if (pp->idx[j] >= 0) ex_insert(cv, ci, pp->val[j], pp->idx[j]);
        if (SOFTMAX) {
            const double pm = pp->m, pz = pp->z;
            const double mn = pm > tm ? pm : tm;
            if (mn > -INFINITY) tz = (tm > -INFINITY ? tz * exp(tm - mn) : 0.0) + (pm > -INFINITY ? pz * exp(pm - mn) : 0.0);
            if (pz != pz) tz = pz;                               // a NaN logit poisons the sum
            tm = mn;
        }
    }
    double mm = 0.0, zz = 1.0;
    if (SOFTMAX) {
        // fixed butterfly order (a serial loop over the 256 partials on one thread took 40 us)
        double a2 = tm;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double om = __shfl_xor(a2, o, 64);
            a2 = om > a2 ? om : a2;
        }
        if (lane == 0) sm[wave] = a2;
        __syncthreads();
        a2 = fmax(fmax(sm[0], sm[1]), fmax(sm[2], sm[3]));
        double b2 = (tz > 0.0 || tz != tz) ? tz * exp(tm - a2) : 0.0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) b2 += __shfl_xor(b2, o, 64);
        if (lane == 0) sz[wave] = b2;
        __syncthreads();
        mm = a2;
        zz = (sz[0] + sz[1]) + (sz[2] + sz[3]);
    }
    int head = 0;                                        // the thread's list is sorted: its best remaining candidate is cv[head]
    for (int out = 0; out < k; ++out) {
        double bv = -INFINITY;
        int bi = -1;
#pragma unroll
        for (int j = 0; j < TOPM; ++j)
            if (j == head) { bv = cv[j]; bi = ci[j]; }
        if (head >= TOPM) bi = -1;
        int bt = t;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
            const bool take = oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi));
            if (take) { bv = ov; bi = oi; bt = ot; }
        }
        __syncthreads();
        if (lane == 0) { rv[wave] = bv; ri[wave] = bi; rt[wave] = bt; }
        __syncthreads();
        bv = rv[0]; bi = ri[0]; bt = rt[0];
        for (int w = 1; w < 4; ++w)
            if (ri[w] >= 0 && (bi < 0 || rv[w] > bv || (rv[w] == bv && ri[w] < bi))) { bv = rv[w]; bi = ri[w]; bt = rt[w]; }
        if (bi < 0) break;                               // uniform: fewer than k ordered candidates (NaN rows)
        if (t == 0) {
            idx_out[img * k + out] = bi;
            val_out[img * k + out] = SOFTMAX ? (float)(exp(bv - mm) / zz) : (float)bv;
        }
        if (t == bt) ++head;
    }
}
template <bool SOFTMAX>
static int sim_exact_launch(const half_t* f, const half_t* wt, int d, long long v, float scale, int k, const SimHdr* hdr, const int* fb,
                            ExPart* part, long long* idx_out, float* val_out, hipStream_t st) {
    // the chunk kernels stage rows of at most 512 d (EX_LDW); wider rows (d = 768) all take the one-block-per-row kernel
    const int nch = ex_nchunks(v), cap = d <= 512 ? ex_rows_cap(v) : 0;
    if (cap > 0) {
        { const int rc_ = scd_set_max_lds((const void*)sim_exact_chunk_kernel<SOFTMAX>, EX_LDS); if (rc_) return rc_; }
        sim_exact_chunk_kernel<SOFTMAX><<<nch, 256, EX_LDS, st>>>(f, wt, d, v, scale, hdr, fb, part, cap, nch);
        sim_exact_merge_kernel<SOFTMAX><<<cap, 256, 0, st>>>(hdr, fb, part, k, idx_out, val_out, cap, nch);
    }
    sim_exact_kernel<SOFTMAX><<<256, 256, 0, st>>>(f, wt, d, v, scale, k, hdr, fb, idx_out, val_out, cap);
    return SCD_OK;
}

// side arrays of the split last round (two vocabulary parts of up to 128 row blocks): values, indices, softmax pairs
static const size_t SIM_SPLIT_ROWS = 2 * 128 * 256;
static const size_t SIM_SPLIT_BYTES = 2 * ((SIM_SPLIT_ROWS * 2 * TOPM * 4 + 255) / 256 * 256) + (SIM_SPLIT_ROWS * 2 * 2 * 4 + 255) / 256 * 256;
extern "C" size_t scd_sim_topk_ws_bytes(int64_t n, int d, int64_t v, int k) {
    (void)d; (void)v; (void)k;
    return 64 + scd_align((size_t)n * 2 * TOPM * 4) * 2 + scd_align((size_t)n * 32) + scd_align((size_t)n * 4) * 2 + 256 +
           scd_align(sizeof(ExPart) * (size_t)ex_rows_cap(v) * ex_nchunks(v)) + SIM_SPLIT_BYTES;
}

// one launch instead of three fills: the header ({max ||w||^2, fallback counter}), and the output slots no pass fills (a row whose logits
// are NaN has no ordered candidates) as index -1 / value NaN (all-ones bits), never garbage
__global__ void __launch_bounds__(256) sim_init_kernel(SimHdr* hdr, const unsigned* __restrict__ wmax2_src, unsigned long long* __restrict__ idx_out,
                                                       unsigned* __restrict__ val_out, long long nk) {
    const long long i0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    if (i0 == 0) {
        hdr->wmax2_bits = wmax2_src ? *wmax2_src : 0u;
        hdr->fb_cnt = 0;
    }
    for (long long i = i0; i < nk; i += step) {
        idx_out[i] = ~0ull;
        val_out[i] = ~0u;
    }
}

extern "C" int scd_sim_vocab_norm(scd_handle h, const void* Wt, int64_t v, int d, void* wmax2_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_sim_vocab_norm");
    SCD_REQUIRE(Wt && wmax2_out && v > 0 && d > 0 && d % 8 == 0, "scd_sim_vocab_norm: bad arguments");
    hipStream_t st = (hipStream_t)stream_;
    SCD_HIP(hipMemsetAsync(wmax2_out, 0, 4, st));
    const long long wb = scd_cdiv(v, 32);
    wmax_kernel<<<(unsigned)(wb < 256 ? 256 : (wb > 2048 ? 2048 : wb)), 256, 0, st>>>((const half_t*)Wt, v, d, (unsigned*)wmax2_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// which kernels the last scd_sim_topk* call of this process launched (include/scd_hip.h SCD_SIM_PATH_*): lets a test of the environment
// switches prove that the switched path ran
static int g_sim_last_path = 0;
extern "C" int scd_sim_last_path(void) { return g_sim_last_path; }

static int sim_topk_impl(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int k,
                         int mode, int64_t* idx_out, float* val_out, int32_t* fallback_rows_out, void* ws,
                         size_t ws_bytes, const void* wmax2, void* stream_) {
    SCD_REQUIRE(h && F && Wt && idx_out && val_out && ws, "scd_sim_topk: null argument");
    SCD_REQUIRE(n > 0 && v > 0 && n < (1ll << 31) && v < (1ll << 31), "scd_sim_topk: bad shape n=%lld v=%lld", (long long)n, (long long)v);
    SCD_REQUIRE(d > 0 && (d <= 512 || d == 768) && d % 64 == 0, "scd_sim_topk: d=%d must be a multiple of 64 up to 512, or 768", d);
    SCD_REQUIRE(k >= 1 && k <= TOPM && k <= v, "scd_sim_topk: k=%d must be in [1,%d] and <= v", k, TOPM);
    SCD_REQUIRE(mode == SCD_SIM_RAW || mode == SCD_SIM_SOFTMAX, "scd_sim_topk: bad mode %d", mode);
    SCD_REQUIRE(scale > 0.f, "scd_sim_topk: scale must be positive");
    SCD_REQUIRE(ws_bytes >= scd_sim_topk_ws_bytes(n, d, v, k), "scd_sim_topk: workspace too small");
    { const int rc_ = scd_check_device(h, "scd_sim_topk"); if (rc_) return rc_; }
    hipStream_t st = (hipStream_t)stream_;
    char* w = (char*)ws;
    SimHdr* hdr = (SimHdr*)w;
    const size_t csz = scd_align((size_t)n * 2 * TOPM * 4);
    float* cval = (float*)(w + 64);
    int* cidx = (int*)(w + 64 + csz);
    float* stats = (float*)(w + 64 + 2 * csz);
    int* fb = (int*)(w + 64 + 2 * csz + scd_align((size_t)n * 32));
    float* bnd = (float*)(w + 64 + 2 * csz + scd_align((size_t)n * 32) + scd_align((size_t)n * 4));
    ExPart* expart = (ExPart*)(w + 64 + 2 * csz + scd_align((size_t)n * 32) + scd_align((size_t)n * 4) * 2 + 256);
    const half_t* f = (const half_t*)F;
    const half_t* wt = (const half_t*)Wt;
    {   // header + unfilled output slots in one launch (were three fills); max ||w||^2 from the caller (scd_sim_vocab_norm: the vocabulary is
        // constant over a run, its norm was recomputed by every call: 12 us of a 2.7-ms call) or computed here
        const long long nk = (long long)n * k;
        const long long ib = scd_cdiv(nk, 256 * 8);
        sim_init_kernel<<<(unsigned)(ib < 1 ? 1 : (ib > 1024 ? 1024 : ib)), 256, 0, st>>>(hdr, (const unsigned*)wmax2, (unsigned long long*)idx_out,
                                                                                         (unsigned*)val_out, nk);
    }
    // one sweep of the rows (32 per block and iteration) up to 2,048 blocks: at V = 21,000 the 256-block launch walked the vocabulary in
    // three dependent iterations per wave (12 us for 21.5 MB)
    if (!wmax2) { const long long wb = scd_cdiv(v, 32); wmax_kernel<<<(unsigned)(wb < 256 ? 256 : (wb > 2048 ? 2048 : wb)), 256, 0, st>>>(wt, v, d, &hdr->wmax2_bits); }
    const unsigned g1 = (unsigned)scd_cdiv(n, 256), g2 = (unsigned)scd_cdiv(n, 4);
    { const int rc_ = scd_set_max_lds((const void*)sim_topk_kernel<true, 8>, 65536 + 32768); if (rc_) return rc_; }
    { const int rc_ = scd_set_max_lds((const void*)sim_topk_kernel<false, 8>, 65536 + 32768); if (rc_) return rc_; }
    // SCD_SIM_RB: 8 (default) = the eight-wave 32x32x16 kernel with eight entries per half list for k >= 2; 16 = 16x16x32 tiles for
    // k <= 3 (2-3 % faster on unstructured features, but its 16 candidates per image are the best four of four QUARTER lists: on
    // features whose top logits crowd inside the error bound - the bench's synthetic images: 100 planted names within ~0.5 - a hundred
    // rows per call fail their certificate and the exact pass costs more than the tiles save)
    static const int use_rb_env = getenv("SCD_SIM_RB") ? atoi(getenv("SCD_SIM_RB")) : 8;
    const int use_rb = use_rb_env == 16 ? 16 : 8;
    const bool sm = mode == SCD_SIM_SOFTMAX;
    if (use_rb && d == 512 && v < (1ll << 28)) {
        // row-block kernels (the CLIP width): units of 32 names x K = 512, epilogue hidden behind the next unit's MFMAs
        static const int refine4 = getenv("SCD_SIM_REFINE4") ? atoi(getenv("SCD_SIM_REFINE4")) : 1;
#define RB_TAIL(SM, TMV, KSV)                                                                                                   \
        if (refine4) sim_refine4_kernel<SM, TMV><<<(unsigned)scd_cdiv(n, 16), 256, 0, st>>>(f, wt, n, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, KSV, nullptr, 2); \
        else sim_refine_kernel<SM, TMV><<<g2, 256, 0, st>>>(f, wt, n, d, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, KSV); \
        { const int rc_ = sim_exact_launch<SM>(f, wt, d, v, scale, k, hdr, fb, expart, (long long*)idx_out, val_out, st); if (rc_) return rc_; }
#define RC_GO(SM, TMV, KSV)                                                                                                     \
    {                                                                                                                           \
        { const int rc_ = scd_set_max_lds((const void*)sim_topk_rc_kernel<SM, TMV, KSV>, 131072); if (rc_) return rc_; }            \
        sim_topk_rc_kernel<SM, TMV, KSV><<<g1, 512, 131072, st>>>(f, wt, n, v, scale, cval, cidx, stats, bnd, &hdr->wmax2_bits); \
        sim_refine4_kernel<SM, 8><<<(unsigned)scd_cdiv(n, 16), 256, 0, st>>>(f, wt, n, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, -1, bnd, 4); \
        { const int rc_ = sim_exact_launch<SM>(f, wt, d, v, scale, k, hdr, fb, expart, (long long*)idx_out, val_out, st); if (rc_) return rc_; } \
    }
        // the partial last round of row blocks (g1 mod 256 of them), when it fills at most half of the chip and the vocabulary is long
        // enough to halve: two blocks per row block, one per vocabulary half, merged before the refine pass
        static const int split_env = getenv("SCD_SIM_SPLIT") ? atoi(getenv("SCD_SIM_SPLIT")) : 1;
        const unsigned rem = g1 % 256u;
        const long long nun = (v + 31) / 32;
        const bool split = split_env && rem > 0 && rem <= 128 && nun >= 32;
        const long long vsplit = (nun / 2) * 32;
        char* sp = (char*)expart + scd_align(sizeof(ExPart) * (size_t)ex_rows_cap(v) * ex_nchunks(v));
        float* sp_val = (float*)sp;
        int* sp_idx = (int*)(sp + scd_align(SIM_SPLIT_ROWS * 2 * TOPM * 4));
        float* sp_st = (float*)(sp + 2 * scd_align(SIM_SPLIT_ROWS * 2 * TOPM * 4));
#define RB8_GO(SM, TMV, KSV)                                                                                                    \
    {                                                                                                                           \
        { const int rc_ = scd_set_max_lds((const void*)sim_topk_rb8_kernel<SM, TMV, KSV>, 131072); if (rc_) return rc_; }           \
        if (!split) sim_topk_rb8_kernel<SM, TMV, KSV><<<g1, 512, 131072, st>>>(f, wt, n, v, scale, cval, cidx, stats, &hdr->wmax2_bits); \
        else {                                                                                                                  \
            const long long row0 = (long long)(g1 - rem) * 256, prow = (long long)rem * 256;                                   \
            if (g1 > rem) sim_topk_rb8_kernel<SM, TMV, KSV><<<g1 - rem, 512, 131072, st>>>(f, wt, n, v, scale, cval, cidx, stats, &hdr->wmax2_bits); \
            sim_topk_rb8_kernel<SM, TMV, KSV><<<2 * rem, 512, 131072, st>>>(f, wt, n, v, scale, sp_val, sp_idx, sp_st, &hdr->wmax2_bits, \
                                                                            (int)(g1 - rem), 2, vsplit, row0, prow);           \
            sim_split_merge_kernel<<<(unsigned)scd_cdiv((n - row0) * 2, 256), 256, 0, st>>>(sp_val, sp_idx, sp_st, row0, n, prow, TMV, SM ? 1 : 0, \
                                                                                            cval, cidx, stats);                \
        }                                                                                                                       \
        RB_TAIL(SM, TMV, KSV)                                                                                                   \
    }
        g_sim_last_path = (use_rb == 16 && k <= 3) ? (SCD_SIM_PATH_RC16 | SCD_SIM_PATH_REFINE4)
                                                   : (SCD_SIM_PATH_RB8 | (split ? SCD_SIM_PATH_SPLIT : 0) | (refine4 ? SCD_SIM_PATH_REFINE4 : 0));
        if (use_rb == 16 && k <= 3) {
            // 16x16x32 tiles, four quarter lists per image: TM = k + 2 entries each, the best four leave the kernel
            if (k == 1) { if (sm) RC_GO(true, 3, 0) else RC_GO(false, 3, 0) }
            else { if (sm) RC_GO(true, 5, 2) else RC_GO(false, 5, 2) }
        } else {
            // entries per half list: TM >= k + 2 for k <= 6 (a row then fails its certificate only when one half holds the image's TM + 1
            // best and two gaps among them are inside the error bound).  For k = 7, 8 TM = 8 < k + 2: a row whose k + 1 best names share
            // a half list cannot be certified whatever the gaps (the list's last entry is the k-th value or next to it) and takes the
            // exact pass (docs/design/sim_topk.md, "what the tests pin").  KS + 1 >= k: the entry of the other half's list the shared
            // threshold uses
            if (k == 1) { if (sm) RB8_GO(true, 4, 0) else RB8_GO(false, 4, 0) }
            else if (k <= 3) { if (sm) RB8_GO(true, 8, 2) else RB8_GO(false, 8, 2) }
            else if (k <= 5) { if (sm) RB8_GO(true, 8, 4) else RB8_GO(false, 8, 4) }
            else { if (sm) RB8_GO(true, 8, 7) else RB8_GO(false, 8, 7) }
        }
#undef RB8_GO
#undef RC_GO
#undef RB_TAIL
        if (fallback_rows_out) SCD_HIP(hipMemcpyAsync(fallback_rows_out, &hdr->fb_cnt, 4, hipMemcpyDeviceToDevice, st));
        SCD_LAUNCH_CHECK();
        return SCD_OK;
    }
    if (d == 768) {
        // the ViT-L/14 width: the four-wave tile kernel with twelve 64-deep sub-steps per tile (128 images x 128 names)
        const unsigned g4 = (unsigned)scd_cdiv(n, 128);
        g_sim_last_path = SCD_SIM_PATH_TILE768;
        { const int rc_ = scd_set_max_lds((const void*)sim_topk_kernel<true, 4, 12>, 65536 + 16384); if (rc_) return rc_; }
        { const int rc_ = scd_set_max_lds((const void*)sim_topk_kernel<false, 4, 12>, 65536 + 16384); if (rc_) return rc_; }
        if (sm) {
            sim_topk_kernel<true, 4, 12><<<g4, 256, 65536 + 16384, st>>>(f, wt, n, d, v, scale, cval, cidx, stats, 0);
            sim_refine_kernel<true, TOPM><<<g2, 256, 0, st>>>(f, wt, n, d, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, -1);
            { const int rc_ = sim_exact_launch<true>(f, wt, d, v, scale, k, hdr, fb, expart, (long long*)idx_out, val_out, st); if (rc_) return rc_; }
        } else {
            sim_topk_kernel<false, 4, 12><<<g4, 256, 65536 + 16384, st>>>(f, wt, n, d, v, scale, cval, cidx, stats, 0);
            sim_refine_kernel<false, TOPM><<<g2, 256, 0, st>>>(f, wt, n, d, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, -1);
            { const int rc_ = sim_exact_launch<false>(f, wt, d, v, scale, k, hdr, fb, expart, (long long*)idx_out, val_out, st); if (rc_) return rc_; }
        }
        if (fallback_rows_out) SCD_HIP(hipMemcpyAsync(fallback_rows_out, &hdr->fb_cnt, 4, hipMemcpyDeviceToDevice, st));
        SCD_LAUNCH_CHECK();
        return SCD_OK;
    }
    // d < 512: the eight-wave tile kernel (256 images x 128 names sub-tiles)
    g_sim_last_path = SCD_SIM_PATH_TILE;
    if (sm) {
        sim_topk_kernel<true, 8><<<g1, 512, 65536 + 32768, st>>>(f, wt, n, d, v, scale, cval, cidx, stats, 0);
        sim_refine_kernel<true, TOPM><<<g2, 256, 0, st>>>(f, wt, n, d, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, -1);
        { const int rc_ = sim_exact_launch<true>(f, wt, d, v, scale, k, hdr, fb, expart, (long long*)idx_out, val_out, st); if (rc_) return rc_; }
    } else {
        sim_topk_kernel<false, 8><<<g1, 512, 65536 + 32768, st>>>(f, wt, n, d, v, scale, cval, cidx, stats, 0);
        sim_refine_kernel<false, TOPM><<<g2, 256, 0, st>>>(f, wt, n, d, v, scale, k, cval, cidx, stats, hdr, fb, (long long*)idx_out, val_out, -1);
        { const int rc_ = sim_exact_launch<false>(f, wt, d, v, scale, k, hdr, fb, expart, (long long*)idx_out, val_out, st); if (rc_) return rc_; }
    }
    if (fallback_rows_out) SCD_HIP(hipMemcpyAsync(fallback_rows_out, &hdr->fb_cnt, 4, hipMemcpyDeviceToDevice, st));
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) transpose_f16_kernel(const half_t* __restrict__ in, long long r, long long c,
                                                            half_t* __restrict__ out) {
    __shared__ half_t tile[64][66];
    const long long c0 = (long long)blockIdx.x * 64, r0 = (long long)blockIdx.y * 64;
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int y = i >> 6, x = i & 63;
        tile[y][x] = (r0 + y < r && c0 + x < c) ? in[(r0 + y) * c + c0 + x] : (half_t)0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int y = i >> 6, x = i & 63;       // out row = c0+y, col = r0+x
        if (c0 + y < c && r0 + x < r) out[(c0 + y) * r + r0 + x] = tile[x][y];
    }
}
extern "C" int scd_transpose_f16(scd_handle h, const void* in, int64_t r, int64_t c, void* out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_transpose_f16");
    SCD_REQUIRE(h && in && out && r > 0 && c > 0, "scd_transpose_f16: bad arguments");
    transpose_f16_kernel<<<dim3((unsigned)scd_cdiv(c, 64), (unsigned)scd_cdiv(r, 64)), 256, 0, (hipStream_t)stream_>>>(
        (const half_t*)in, r, c, (half_t*)out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// out = fp16((a + b) / 2), elementwise: the "textual enhancement" feature of BASELINE configs[4] - the reference leaves
// `logits = 100. * (clip_batch_feat @ zeroshot_weights + closed_text_feat @ zeroshot_weights) / 2` commented at
// main_unsup.py:518,523,604,609; by linearity that is 100 * ((f + t) / 2) @ W, so the re-ranking is scd_sim_topk on the mean.
__global__ void __launch_bounds__(256) mean2_f16_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, long long n8,
                                                        half_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const half8 x = *(const half8*)(a + i * 8), y = *(const half8*)(b + i * 8);
    half8 o;
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = (half_t)(((float)x[q] + (float)y[q]) * 0.5f);
    *(half8*)(out + i * 8) = o;
}
extern "C" int scd_mean2_f16(scd_handle h, const void* a, const void* b, int64_t n_elems, void* out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_mean2_f16");
    SCD_REQUIRE(h && a && b && out && n_elems > 0 && n_elems % 8 == 0, "scd_mean2_f16: bad arguments (n_elems must be a multiple of 8)");
    mean2_f16_kernel<<<(unsigned)scd_cdiv(n_elems / 8, 256), 256, 0, (hipStream_t)stream_>>>((const half_t*)a, (const half_t*)b,
                                                                                           n_elems / 8, (half_t*)out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

__global__ void __launch_bounds__(256) gather_rows_kernel(const half_t* __restrict__ Wt, const long long* __restrict__ idx,
                                                          long long m, int d, half_t* __restrict__ out) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const long long src = idx[row];
    for (int j = threadIdx.x & 63; j < d; j += 64) out[row * d + j] = Wt[src * d + j];
}
extern "C" int scd_gather_rows_f16(scd_handle h, const void* Wt, const int64_t* idx, int64_t m, int d, void* out,
                                   void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_gather_rows_f16");
    SCD_REQUIRE(h && Wt && idx && out && m > 0 && d > 0, "scd_gather_rows_f16: bad arguments");
    gather_rows_kernel<<<(unsigned)scd_cdiv(m, 4), 256, 0, (hipStream_t)stream_>>>((const half_t*)Wt, (const long long*)idx, m,
                                                                                 d, (half_t*)out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// the row selections of main_unsup.py:318-321,561 (`all_feats[~mask_lab]`, `all_feats[mask_lab]`, `name_idx_top5[~mask_lab]`) in one launch:
// for the m rows idx[i] of F (fp16 [n, d]): out16[i] = the row (the vote loop's features), out32[i] = its float32 image (the K-Means
// input) and nidx_out[i] = name_idx[idx[i]] (int64 [n, k]); any output may be NULL.  One wave per selected row.
__global__ void __launch_bounds__(256) select_rows_kernel(const half_t* __restrict__ F, const long long* __restrict__ name_idx,
                                                          const long long* __restrict__ idx, long long m, int d, int k,
                                                          half_t* __restrict__ out16, float* __restrict__ out32, long long* __restrict__ nidx_out) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= m) return;
    const int lane = threadIdx.x & 63;
    const long long src = idx[row];
    if ((d & 7) == 0) {
        for (int j = lane * 8; j < d; j += 512) {
            const half8 v = *(const half8*)(F + src * d + j);
            if (out16) *(half8*)(out16 + row * d + j) = v;
            if (out32) {
                float4 a = {(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, b = {(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
                *(float4*)(out32 + row * d + j) = a;
                *(float4*)(out32 + row * d + j + 4) = b;
            }
        }
    } else {
        for (int j = lane; j < d; j += 64) {
            const half_t v = F[src * d + j];
            if (out16) out16[row * d + j] = v;
            if (out32) out32[row * d + j] = (float)v;
        }
    }
    if (nidx_out && lane < k) nidx_out[row * k + lane] = name_idx[src * k + lane];
}
extern "C" int scd_select_rows(scd_handle h, const void* F, const int64_t* name_idx, const int64_t* idx, int64_t m, int d, int k,
                               void* out16, float* out32, int64_t* nidx_out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_select_rows");
    SCD_REQUIRE(h && F && idx && m > 0 && d > 0 && (out16 || out32 || nidx_out) && (!nidx_out || (name_idx && k > 0 && k <= 64)),
                "scd_select_rows: bad arguments");
    select_rows_kernel<<<(unsigned)scd_cdiv(m, 4), 256, 0, (hipStream_t)stream_>>>((const half_t*)F, (const long long*)name_idx,
                                                                                 (const long long*)idx, m, d, k, (half_t*)out16, out32,
                                                                                 (long long*)nidx_out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// F.normalize(x, dim=-1): x / max(||x||, 1e-12); one wave per row, float32 math on the stored values
template <typename T>
__global__ void __launch_bounds__(256) l2norm_kernel(const T* __restrict__ x, long long n, int d, T* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) {
        const float v = (float)x[row * d + j];
        s = fmaf(v, v, s);
    }
    s = wave_sum_f32(s);
    const float inv = 1.0f / fmaxf(sqrtf(s), 1e-12f);
    for (int j = lane; j < d; j += 64) out[row * d + j] = (T)((float)x[row * d + j] * inv);
}
extern "C" int scd_l2norm_rows(scd_handle h, const void* x, int dtype, int64_t n, int d, void* out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_l2norm_rows");
    SCD_REQUIRE(h && x && out && n > 0 && d > 0, "scd_l2norm_rows: bad arguments");
    const unsigned g = (unsigned)scd_cdiv(n, 4);
    if (dtype == SCD_F32) l2norm_kernel<float><<<g, 256, 0, (hipStream_t)stream_>>>((const float*)x, n, d, (float*)out);
    else if (dtype == SCD_F16) l2norm_kernel<half_t><<<g, 256, 0, (hipStream_t)stream_>>>((const half_t*)x, n, d, (half_t*)out);
    else SCD_REQUIRE(false, "scd_l2norm_rows: bad dtype %d", dtype);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------
// zeroshot_classifier pooling (local_utils/clip_lang_util.py:103-107): per name, L2-normalise its T prompt
// embeddings, average, L2-normalise, and store as COLUMN `name` of out[d, n_names] (torch.stack(dim=1)).
// One block (4 waves) per name; float32 accumulation; d <= 1024.
__global__ void __launch_bounds__(256) prompt_pool_kernel(const half_t* __restrict__ emb, int n_names, int t_per, int d,
                                                          long long col0, long long ld_out, half_t* __restrict__ out) {
    __shared__ float part[4][1024];
    __shared__ float red[4];
    const int name = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int t = wave; t < t_per; t += 4) {
        const half_t* row = emb + ((size_t)name * t_per + t) * d;
        float v[16];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = i * 64 + lane;
            v[i] = j < d ? (float)row[j] : 0.f;
            s = fmaf(v[i], v[i], s);
        }
        const float inv = 1.0f / sqrtf(wave_sum_f32(s));
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = fmaf(v[i], inv, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) part[wave][i * 64 + lane] = acc[i];
    __syncthreads();
    float s = 0.f;
    float m[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = q * 256 + threadIdx.x;
        m[q] = (part[0][j] + part[1][j] + part[2][j] + part[3][j]) / (float)t_per;
        if (j >= d) m[q] = 0.f;
        s = fmaf(m[q], m[q], s);
    }
    s = wave_sum_f32(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float inv = 1.0f / sqrtf(red[0] + red[1] + red[2] + red[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = q * 256 + threadIdx.x;
        if (j < d) out[(size_t)j * ld_out + col0 + name] = (half_t)(m[q] * inv);
    }
}
extern "C" int scd_prompt_pool(scd_handle h, const void* emb, int n_names, int t_per, int d, int64_t col0, int64_t ld_out,
                               void* out, void* stream_) {
    SCD_DEVICE_ENTRY(h, "scd_prompt_pool");
    SCD_REQUIRE(h && emb && out && n_names > 0 && t_per > 0 && d > 0 && d <= 1024, "scd_prompt_pool: bad arguments");
    prompt_pool_kernel<<<n_names, 256, 0, (hipStream_t)stream_>>>((const half_t*)emb, n_names, t_per, d, col0, ld_out, (half_t*)out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}

// SURVEY.md 8b names the re-classification `argmax(scale * F @ Wt^T, -1)` (main_unsup.py:601-614, main_ptsup.py:668-676) as an entry
// point of its own: it is scd_sim_topk with k = 1 on the raw logits (same kernels, same tie rule: the lowest index wins).
extern "C" int scd_sim_topk(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int k,
                            int mode, int64_t* idx_out, float* val_out, int32_t* fallback_rows_out, void* ws,
                            size_t ws_bytes, void* stream) {
    return sim_topk_impl(h, F, Wt, n, d, v, scale, k, mode, idx_out, val_out, fallback_rows_out, ws, ws_bytes, nullptr, stream);
}
extern "C" int scd_sim_topk_prenorm(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int k,
                                    int mode, int64_t* idx_out, float* val_out, int32_t* fallback_rows_out, void* ws,
                                    size_t ws_bytes, const void* wmax2, void* stream) {
    SCD_REQUIRE(wmax2, "scd_sim_topk_prenorm: null vocabulary norm (scd_sim_vocab_norm)");
    return sim_topk_impl(h, F, Wt, n, d, v, scale, k, mode, idx_out, val_out, fallback_rows_out, ws, ws_bytes, wmax2, stream);
}
extern "C" int scd_sim_argmax(scd_handle h, const void* F, const void* Wt, int64_t n, int d, int64_t v, float scale, int64_t* idx_out,
                              float* val_out, void* ws, size_t ws_bytes, void* stream) {
    return scd_sim_topk(h, F, Wt, n, d, v, scale, 1, SCD_SIM_RAW, idx_out, val_out, nullptr, ws, ws_bytes, stream);
}

