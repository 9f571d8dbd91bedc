// Image preprocessing for gfx950: the reference's CLIP `preprocess` (main_unsup.py:237,271; clip `_transform`) on the device, bit for bit.
//
// For each decoded uint8 RGB image (torchvision's pil_loader: Image.open(f).convert('RGB')):
//   Resize(size, BICUBIC)  torchvision 0.11 F_pil.resize -> PIL Image.resize -> Resample.c ImagingResample (8 bpc, separable)
//   CenterCrop(crop)       top/left = int(round((edge - crop) / 2.0)), ties to even
//   ToTensor + Normalize   ((x / 255) - mean) / std in float32, then .half() (the towers' input precision)
// Every resized pixel depends only on its own taps, so only the crop's outputs are computed: per axis the planner emits Pillow's int32
// taps (precompute_coeffs + normalize_coeffs_8bpc) for the `crop` outputs inside the crop window.  The horizontal pass runs over the
// source rows the cropped vertical outputs read and rounds to uint8 as Pillow's intermediate image does; the vertical pass then reads
// that band.  Normalisation is a [3][256] fp16 table the caller builds with the torch recipe, so it is exact by construction.
//
// The planner is host code in double precision; this file is compiled with -ffp-contract=off (scd_amd/build.py) so that no multiply-add
// is fused and the coefficients are Pillow's.
#include "common.h"
#include <math.h>
#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#define IMG_PRECISION_BITS 22
#define IMG_MAX_EDGE (1 << 16)

// ------------------------------------------------------------------------------------------------ host planner (Resample.c)
static double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// One axis: Pillow's taps of outputs off .. off + n - 1 of an in_size -> out_size resize, appended as [first n][ntaps n][koff n][taps ...]
// (koff relative to the start of the block).  in_size == out_size: one unit tap per output, what Pillow's skipped pass amounts to.
static void plan_axis(int in_size, int out_size, int off, int n, std::vector<int32_t>& v) {
    const size_t base = v.size();
    v.resize(base + 3 * (size_t)n);
    if (in_size == out_size) {
        for (int i = 0; i < n; ++i) {
            v[base + i] = off + i;
            v[base + n + i] = 1;
            v[base + 2 * n + i] = (int32_t)(v.size() - base);
            v.push_back(1 << IMG_PRECISION_BITS);
        }
        return;
    }
    const double scale = (double)(float)in_size / out_size;        // (double)(in1 - in0) / outSize, float box ends
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> w;
    for (int i = 0; i < n; ++i) {
        const int xx = off + i;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        w.assign(xmax > 0 ? xmax : 0, 0.0);
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = bicubic_filter((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        v[base + i] = xmin;
        v[base + n + i] = xmax > 0 ? xmax : 0;
        v[base + 2 * n + i] = (int32_t)(v.size() - base);
        for (int x = 0; x < xmax; ++x) {
            const double k = ww != 0.0 ? w[x] / ww : w[x];
            v.push_back(k < 0 ? (int32_t)(-0.5 + k * (1 << IMG_PRECISION_BITS)) : (int32_t)(0.5 + k * (1 << IMG_PRECISION_BITS)));
        }
    }
}

struct ImgGeom {
    int rw, rh, left, top, row0, rows;
};

static int img_geometry(int w, int h, int size, int crop, ImgGeom* g) {
    SCD_REQUIRE(w >= 1 && h >= 1 && w <= IMG_MAX_EDGE && h <= IMG_MAX_EDGE, "scd_image: image size %d x %d outside 1 .. %d", w, h, IMG_MAX_EDGE);
    SCD_REQUIRE(size >= 1 && size <= IMG_MAX_EDGE && crop >= 1 && crop <= size, "scd_image: resize %d / crop %d (1 <= crop <= size <= %d)",
                size, crop, IMG_MAX_EDGE);
    // torchvision 0.11 F_pil.resize, int size: short edge -> size, long edge -> int(size * long / short); short == size: unchanged
    const int shrt = w <= h ? w : h, lng = w <= h ? h : w;
    int rs = shrt, rl = lng;
    if (shrt != size) {
        rs = size;
        const double l = (double)((int64_t)size * lng) / (double)shrt;
        SCD_REQUIRE(l < (double)(1 << 30), "scd_image: %d x %d resizes to a long edge of %.0f", w, h, l);
        rl = (int)l;
    }
    g->rw = w <= h ? rs : rl;
    g->rh = w <= h ? rl : rs;
    SCD_REQUIRE(g->rw >= crop && g->rh >= crop, "scd_image: %d x %d resizes to %d x %d, smaller than the %d crop", w, h, g->rw, g->rh, crop);
    // CenterCrop: int(round((edge - crop) / 2.0)), Python's round = ties to even = nearbyint in the default rounding mode
    g->top = (int)nearbyint((g->rh - crop) / 2.0);
    g->left = (int)nearbyint((g->rw - crop) / 2.0);
    return SCD_OK;
}

struct ImgPlan {
    ImgGeom g;
    std::vector<int32_t> x, y;      // plan_axis blocks of the horizontal / vertical pass
};

// ImageNet is dominated by a few sizes: plans are kept per (w, h, size, crop) for the life of the process
static std::mutex g_plan_mu;
static std::map<std::array<int, 4>, std::shared_ptr<const ImgPlan>> g_plans;

static int get_plan(int w, int h, int size, int crop, std::shared_ptr<const ImgPlan>* out) {
    const std::array<int, 4> key = {w, h, size, crop};
    {
        std::lock_guard<std::mutex> lock(g_plan_mu);
        auto it = g_plans.find(key);
        if (it != g_plans.end()) {
            *out = it->second;
            return SCD_OK;
        }
    }
    auto p = std::make_shared<ImgPlan>();
    const int rc = img_geometry(w, h, size, crop, &p->g);
    if (rc) return rc;
    plan_axis(w, p->g.rw, p->g.left, crop, p->x);
    plan_axis(h, p->g.rh, p->g.top, crop, p->y);
    const int32_t* fy = p->y.data();
    p->g.row0 = fy[0];
    p->g.rows = fy[crop - 1] + fy[crop + crop - 1] - fy[0];       // Pillow's ybox_last - ybox_first over the crop's rows
    std::lock_guard<std::mutex> lock(g_plan_mu);
    if (g_plans.size() >= 4096) g_plans.clear();
    auto it = g_plans.emplace(key, p).first;
    *out = it->second;
    return SCD_OK;
}

extern "C" int scd_image_geometry(int w, int h, int size, int crop, int32_t* out6) {
    SCD_REQUIRE(out6, "scd_image_geometry: null out");
    std::shared_ptr<const ImgPlan> p;
    const int rc = get_plan(w, h, size, crop, &p);
    if (rc) return rc;
    const int32_t g[6] = {p->g.rw, p->g.rh, p->g.left, p->g.top, p->g.row0, p->g.rows};
    for (int i = 0; i < 6; ++i) out6[i] = g[i];
    return SCD_OK;
}

extern "C" int scd_image_plan_axis(int in_size, int out_size, int off, int n, int32_t* first, int32_t* ntaps, int32_t* taps,
                                   int64_t taps_cap, int64_t* n_taps_out) {
    SCD_REQUIRE(in_size >= 1 && out_size >= 1 && in_size <= IMG_MAX_EDGE && out_size <= (1 << 30), "scd_image_plan_axis: sizes %d -> %d",
                in_size, out_size);
    SCD_REQUIRE(off >= 0 && n >= 1 && (int64_t)off + n <= out_size, "scd_image_plan_axis: outputs %d .. %d of %d", off, off + n, out_size);
    std::vector<int32_t> v;
    plan_axis(in_size, out_size, off, n, v);
    const int64_t nt = (int64_t)v.size() - 3 * (int64_t)n;
    if (n_taps_out) *n_taps_out = nt;
    if (!taps) return SCD_OK;
    SCD_REQUIRE(first && ntaps && taps_cap >= nt, "scd_image_plan_axis: %lld taps, capacity %lld", (long long)nt, (long long)taps_cap);
    for (int i = 0; i < n; ++i) {
        first[i] = v[i];
        ntaps[i] = v[n + i];
    }
    for (int64_t t = 0; t < nt; ++t) taps[t] = v[3 * (size_t)n + t];
    return SCD_OK;
}

extern "C" int scd_image_batch_plan(const int32_t* wh, int batch, int size, int crop, scd_image_desc* descs, int32_t* plan,
                                    int64_t plan_cap, int64_t* plan_len, int64_t* pixel_bytes, int64_t* ws_bytes) {
    SCD_REQUIRE(wh && batch >= 1, "scd_image_batch_plan: empty batch");
    std::unordered_map<uint64_t, std::pair<int32_t, int32_t>> at;     // (w, h) -> offsets of its two blocks in `plan`
    int64_t np = 0, src = 0, tmp = 0;
    for (int b = 0; b < batch; ++b) {
        const int w = wh[2 * b], h = wh[2 * b + 1];
        std::shared_ptr<const ImgPlan> p;
        const int rc = get_plan(w, h, size, crop, &p);
        if (rc) return rc;
        const uint64_t key = ((uint64_t)(uint32_t)w << 32) | (uint32_t)h;
        auto it = at.find(key);
        if (it == at.end()) {
            SCD_REQUIRE(np + (int64_t)p->x.size() + (int64_t)p->y.size() < INT32_MAX, "scd_image_batch_plan: plan too large");
            it = at.emplace(key, std::make_pair((int32_t)np, (int32_t)(np + (int64_t)p->x.size()))).first;
            if (plan) {
                SCD_REQUIRE(np + (int64_t)(p->x.size() + p->y.size()) <= plan_cap, "scd_image_batch_plan: plan capacity %lld too small",
                            (long long)plan_cap);
                std::copy(p->x.begin(), p->x.end(), plan + np);
                std::copy(p->y.begin(), p->y.end(), plan + np + p->x.size());
            }
            np += (int64_t)(p->x.size() + p->y.size());
        }
        if (descs) {
            scd_image_desc& d = descs[b];
            d.src_off = src;
            d.tmp_off = tmp;
            d.w = w;
            d.h = h;
            d.plan_x = it->second.first;
            d.plan_y = it->second.second;
            d.row0 = p->g.row0;
            d.rows = p->g.rows;
        }
        src += (int64_t)w * h * 3;
        tmp += (int64_t)p->g.rows * crop * 3;
    }
    if (plan_len) *plan_len = np;
    if (pixel_bytes) *pixel_bytes = src;
    if (ws_bytes) *ws_bytes = tmp;
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ kernels
__device__ __forceinline__ int clip8(int acc) {
    acc >>= IMG_PRECISION_BITS;
    return acc < 0 ? 0 : (acc > 255 ? 255 : acc);
}

// Is output i of the axis block at `p` (crop outputs) inside the plan and reading inputs [lo, lo + len) only?  first is shifted by -shift.
__device__ __forceinline__ bool taps_ok(const int32_t* __restrict__ plan, long long plan_len, int p, int crop, int i, int shift, int len) {
    if (p < 0 || (long long)p + 3ll * crop > plan_len) return false;
    const int f = plan[p + i] - shift, n = plan[p + crop + i], k = plan[p + 2 * crop + i];
    return f >= 0 && n >= 0 && (long long)f + n <= len && k >= 0 && (long long)p + k + n <= plan_len;
}

// The descriptor's own ranges: source pixels inside pixel_bytes, band inside tmp_bytes, band rows inside the image.
__device__ __forceinline__ bool desc_ok(const scd_image_desc& d, long long pixel_bytes, long long tmp_bytes, int crop) {
    return d.w >= 1 && d.h >= 1 && d.src_off >= 0 && d.src_off + 3ll * d.w * d.h <= pixel_bytes && d.tmp_off >= 0 && d.rows >= 0 &&
           d.tmp_off + 3ll * d.rows * crop <= tmp_bytes && d.row0 >= 0 && (long long)d.row0 + d.rows <= d.h;
}

// Horizontal pass: band row r (source row row0 + r), crop column x -> tmp[r][x][c], uint8.  grid (row blocks, batch), one column per lane.
__global__ void __launch_bounds__(256) image_hpass_kernel(const uint8_t* __restrict__ pixels, long long pixel_bytes,
                                                          const scd_image_desc* __restrict__ descs, const int32_t* __restrict__ plan,
                                                          long long plan_len, int crop, uint8_t* __restrict__ tmp, long long tmp_bytes) {
    const scd_image_desc d = descs[blockIdx.y];
    const int x = threadIdx.x;
    if (x >= crop) return;
    if (!desc_ok(d, pixel_bytes, tmp_bytes, crop) || !taps_ok(plan, plan_len, d.plan_x, crop, x, 0, d.w)) return;    // vpass: NaN
    const int first = plan[d.plan_x + x], n = plan[d.plan_x + crop + x];
    const int32_t* __restrict__ k = plan + d.plan_x + plan[d.plan_x + 2 * crop + x];
    for (int r = blockIdx.x; r < d.rows; r += gridDim.x) {
        const uint8_t* __restrict__ s = pixels + d.src_off + ((long long)(d.row0 + r) * d.w + first) * 3;
        int a0 = 1 << (IMG_PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int t = 0; t < n; ++t) {
            const int kt = k[t];
            a0 += (int)s[3 * t + 0] * kt;
            a1 += (int)s[3 * t + 1] * kt;
            a2 += (int)s[3 * t + 2] * kt;
        }
        uint8_t* o = tmp + d.tmp_off + ((long long)r * crop + x) * 3;
        o[0] = (uint8_t)clip8(a0);
        o[1] = (uint8_t)clip8(a1);
        o[2] = (uint8_t)clip8(a2);
    }
}

// Vertical pass + normalisation: crop row y, column x -> out[b][c][y][x] = lut[c][clip8(sum)].  grid (row blocks, batch).
// It repeats the horizontal pass's checks of column x, so a band column that pass left unwritten is never read: those pixels are NaN.
__global__ void __launch_bounds__(256) image_vpass_kernel(const scd_image_desc* __restrict__ descs, const int32_t* __restrict__ plan,
                                                          long long plan_len, long long pixel_bytes, int crop, const uint8_t* __restrict__ tmp,
                                                          long long tmp_bytes, const half_t* __restrict__ lut, half_t* __restrict__ out) {
    const int b = blockIdx.y;
    const scd_image_desc d = descs[b];
    const int x = threadIdx.x;
    if (x >= crop) return;
    const bool ok = desc_ok(d, pixel_bytes, tmp_bytes, crop) && taps_ok(plan, plan_len, d.plan_x, crop, x, 0, d.w);
    half_t* ob = out + (long long)b * 3 * crop * crop;
    for (int y = blockIdx.x; y < crop; y += gridDim.x) {
        half_t v0, v1, v2;
        if (ok && taps_ok(plan, plan_len, d.plan_y, crop, y, d.row0, d.rows)) {
            const int first = plan[d.plan_y + y] - d.row0, n = plan[d.plan_y + crop + y];
            const int32_t* __restrict__ k = plan + d.plan_y + plan[d.plan_y + 2 * crop + y];
            const uint8_t* __restrict__ s = tmp + d.tmp_off + ((long long)first * crop + x) * 3;
            int a0 = 1 << (IMG_PRECISION_BITS - 1), a1 = a0, a2 = a0;
            for (int t = 0; t < n; ++t) {
                const int kt = k[t];
                const uint8_t* p = s + (long long)t * crop * 3;
                a0 += (int)p[0] * kt;
                a1 += (int)p[1] * kt;
                a2 += (int)p[2] * kt;
            }
            v0 = lut[clip8(a0)];
            v1 = lut[256 + clip8(a1)];
            v2 = lut[512 + clip8(a2)];
        } else {
            v0 = v1 = v2 = (half_t)__builtin_nanf("");     // a descriptor the planner did not make: visible, never read out of range
        }
        const long long o = (long long)y * crop + x;
        ob[o] = v0;
        ob[(long long)crop * crop + o] = v1;
        ob[2ll * crop * crop + o] = v2;
    }
}

extern "C" int scd_image_preprocess(scd_handle h, const uint8_t* pixels, int64_t pixel_bytes, const scd_image_desc* descs, const int32_t* plan,
                                    int64_t plan_len, int batch, int crop, const void* lut, void* out, void* ws, size_t ws_bytes, void* stream) {
    SCD_DEVICE_ENTRY(h, "scd_image_preprocess");
    SCD_REQUIRE(batch >= 0 && batch <= 65535, "scd_image_preprocess: batch %d outside 0 .. 65535", batch);
    SCD_REQUIRE(crop >= 1 && crop <= 256, "scd_image_preprocess: crop %d outside 1 .. 256 (one lane per output column)", crop);
    if (batch == 0) return SCD_OK;
    SCD_REQUIRE(pixels && descs && plan && lut && out && ws, "scd_image_preprocess: null pointer");
    hipStream_t st = (hipStream_t)stream;
    // 64 blocks of band rows per image: an ImageNet image's ~230-380 rows in 4-6 rounds, a 16k-row one in 256
    image_hpass_kernel<<<dim3(64, batch), 256, 0, st>>>(pixels, pixel_bytes, descs, plan, plan_len, crop, (uint8_t*)ws, (long long)ws_bytes);
    SCD_LAUNCH_CHECK();
    image_vpass_kernel<<<dim3((crop + 3) / 4, batch), 256, 0, st>>>(descs, plan, plan_len, pixel_bytes, crop, (const uint8_t*)ws, (long long)ws_bytes,
                                                                     (const half_t*)lut, (half_t*)out);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
