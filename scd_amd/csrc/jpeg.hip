// Baseline JPEG decoding on gfx950, bit-equal to Pillow's Image.open(f).convert('RGB') (libjpeg-turbo's default path): only the
// compressed bytes cross to the device, and the decoded uint8 RGB lands in the pixel section scd_image_preprocess reads
// (docs/design/ingest.md, "Device JPEG decode").
//
//   host    scd_jpeg_parse        markers, tables, scope check with a reason code, the scan's byte range and its RSTn markers
//           scd_jpeg_batch_plan   per-image descriptors, the batch's distinct Huffman / quantisation tables, section sizes
//           scd_jpeg_decode_host  one file on the CPU through the same functions as the kernels (jpeg.h)
//   device  scd_jpeg_decode       jpeg_entropy_idct_kernel: one wave per image - lane 0 walks the bit stream of up to 8 blocks into LDS,
//                                 then 8 lanes per block run the column and the row pass and store the samples into component planes;
//                                 jpeg_colour_kernel: fancy upsampling + YCbCr -> RGB, one lane per pixel
// Everything the entropy decoder cannot follow, and the range guard, end in a per-image status; the caller decodes such an image
// with Pillow.  No loop depends on the data alone: symbols per block <= 64, blocks from the header, every byte read checked against
// the file's length, every store against the image's own extent.
//
// The host half compiles without the HIP compiler too (tests/sanitize_jpeg.cpp builds it with the host sanitizers).
#include "common.h"
#include "jpeg.h"
#include <string.h>
#include <exception>
#include <map>
#include <string>
#include <vector>

#define JPEG_MAX_EDGE 65536

static const uint8_t k_zigzag[64] = JPEG_ZIGZAG_INIT;

// ------------------------------------------------------------------------------------------------ host: tables
// DHT payload (16 counts, then the symbols) -> derived table.  False for a table libjpeg refuses (jpeg_make_d_derived_tbl): more than
// 256 symbols, a code that does not fit its length (the all-ones code included), a DC category above 15, symbols past `avail`.
static bool build_huff(const uint8_t* p, int64_t avail, bool is_dc, JpegHuff* t) {
    if (avail < 16) return false;
    int total = 0;
    for (int l = 0; l < 16; ++l) total += p[l];
    if (total > 256 || 16 + total > avail) return false;
    memset(t, 0, sizeof(*t));
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = p[l - 1];
        t->maxcode[l] = -1;
        if (n) {
            if (code + n >= (1 << l)) return false;          // before anything is written: the fill below is indexed by the code
            t->valoff[l] = k - code;
            if (l <= 8)
                for (int i = 0; i < n; ++i)
                    for (int f = 0; f < (1 << (8 - l)); ++f) t->look[((code + i) << (8 - l)) + f] = (uint16_t)((l << 8) | p[16 + k + i]);
            k += n;
            code += n;
            t->maxcode[l] = code - 1;
        }
        code <<= 1;
    }
    for (int i = 0; i < total; ++i) {
        if (is_dc && p[16 + i] > 15) return false;
        t->huffval[i] = p[16 + i];
    }
    return true;
}

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// ------------------------------------------------------------------------------------------------ host: parser
static void jpeg_parse(const uint8_t* d, int64_t n, scd_jpeg_info* out, int32_t* rst, int64_t rst_cap) {
    scd_jpeg_info I;
    memset(&I, 0, sizeof(I));
    I.file_len = (int32_t)n;
#define REJECT(r)              \
    do {                       \
        I.reason = (r);        \
        *out = I;              \
        return;                \
    } while (0)
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) REJECT(SCD_JPEG_NOT_JPEG);
    int64_t qpos[4] = {0, 0, 0, 0}, hpos[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    int qprec[4] = {0, 0, 0, 0};
    bool jfif = false, adobe = false, sof = false;
    int adobe_transform = -1;
    int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, cq[3] = {0, 0, 0};
    int64_t p = 2;
    for (;;) {
        if (p + 2 > n) REJECT(SCD_JPEG_TRUNCATED);
        if (d[p] != 0xFF) REJECT(SCD_JPEG_BAD_MARKER);
        while (p + 1 < n && d[p + 1] == 0xFF) ++p;            // fill bytes before a marker
        if (p + 2 > n) REJECT(SCD_JPEG_TRUNCATED);
        const int m = d[p + 1];
        p += 2;
        // Pillow's own marker walk knows 0xC0 .. 0xFE only; a stray RSTn, SOI or EOI before the scan is left to it as well
        if (m < 0xC0 || m == 0xFF || (m >= 0xD0 && m <= 0xD9)) REJECT(SCD_JPEG_BAD_MARKER);
        if (m == 0xDE || m == 0xDF || (m >= 0xF0 && m <= 0xFD)) REJECT(SCD_JPEG_BAD_MARKER);     // libjpeg: unsupported marker type
        if (p + 2 > n) REJECT(SCD_JPEG_TRUNCATED);
        const int len = be16(d + p);
        if (len < 2 || p + len > n) REJECT(SCD_JPEG_TRUNCATED);
        const uint8_t* s = d + p + 2;
        const int sl = len - 2;
        if (m == 0xC0 || m == 0xC1) {
            if (sof) REJECT(SCD_JPEG_BAD_MARKER);
            if (sl < 6) REJECT(SCD_JPEG_TRUNCATED);
            sof = true;
            if (s[0] != 8) REJECT(SCD_JPEG_PRECISION);
            I.h = be16(s + 1);
            I.w = be16(s + 3);
            I.ncomp = s[5];
            if (I.h == 0 || I.w == 0) REJECT(SCD_JPEG_DNL);
            if (I.ncomp != 1 && I.ncomp != 3) REJECT(SCD_JPEG_COMPONENTS);
            if (sl != 6 + 3 * I.ncomp) REJECT(SCD_JPEG_BAD_MARKER);      // libjpeg: bad length
            for (int c = 0; c < I.ncomp; ++c) {
                cid[c] = s[6 + 3 * c];
                ch[c] = s[7 + 3 * c] >> 4;
                cv[c] = s[7 + 3 * c] & 15;
                cq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) REJECT(SCD_JPEG_SAMPLING);
                if (cq[c] > 3) REJECT(SCD_JPEG_BAD_TABLE);
            }
            if (I.ncomp == 1) {
                I.hs = I.vs = 1;             // a one-component scan is one block per MCU whatever the factors say
            } else {
                I.hs = ch[0];
                I.vs = cv[0];
                const bool luma_ok = (I.hs == 1 && I.vs == 1) || (I.hs == 2 && I.vs == 1) || (I.hs == 2 && I.vs == 2);
                if (!luma_ok || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) REJECT(SCD_JPEG_SAMPLING);
                if (cid[0] == cid[1] || cid[0] == cid[2] || cid[1] == cid[2]) REJECT(SCD_JPEG_BAD_MARKER);
            }
        } else if (m == 0xC2) {
            REJECT(SCD_JPEG_PROGRESSIVE);
        } else if (m >= 0xC9 && m <= 0xCF && m != 0xCC) {
            REJECT(SCD_JPEG_ARITHMETIC);
        } else if (m == 0xCC) {
            REJECT(SCD_JPEG_ARITHMETIC);
        } else if (m == 0xC3 || (m >= 0xC5 && m <= 0xC8)) {
            REJECT(SCD_JPEG_SOF);
        } else if (m == 0xC4) {
            int o = 0;
            while (o < sl) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) REJECT(SCD_JPEG_BAD_TABLE);
                JpegHuff t;
                if (!build_huff(s + o + 1, sl - o - 1, tc == 0, &t)) REJECT(SCD_JPEG_BAD_TABLE);
                int total = 0;
                for (int l = 0; l < 16; ++l) total += s[o + 1 + l];
                hpos[tc][th] = p + 2 + o + 1;
                o += 17 + total;
            }
        } else if (m == 0xDB) {
            int o = 0;
            while (o < sl) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                if (pq > 1 || tq > 3) REJECT(SCD_JPEG_BAD_TABLE);
                const int bytes = pq ? 128 : 64;
                if (o + 1 + bytes > sl) REJECT(SCD_JPEG_BAD_TABLE);
                qpos[tq] = p + 2 + o + 1;
                qprec[tq] = pq;
                o += 1 + bytes;
            }
        } else if (m == 0xDD) {
            if (sl != 2) REJECT(SCD_JPEG_BAD_MARKER);
            I.restart_interval = be16(s);
        } else if (m == 0xDC) {
            REJECT(SCD_JPEG_DNL);
        } else if (m == 0xE0) {
            if (sl >= 14 && s[0] == 'J' && s[1] == 'F' && s[2] == 'I' && s[3] == 'F' && s[4] == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && s[0] == 'A' && s[1] == 'd' && s[2] == 'o' && s[3] == 'b' && s[4] == 'e') {
                adobe = true;
                adobe_transform = s[11];
            }
        } else if (m == 0xDA) {
            if (!sof) REJECT(SCD_JPEG_BAD_MARKER);
            if (sl < 1 || sl != 1 + 2 * s[0] + 3) REJECT(SCD_JPEG_BAD_MARKER);     // libjpeg: bad length
            if (s[0] != I.ncomp) REJECT(SCD_JPEG_MULTISCAN);
            for (int c = 0; c < I.ncomp; ++c) {
                if (s[1 + 2 * c] != cid[c]) REJECT(SCD_JPEG_MULTISCAN);
                const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
                if (td > 3 || ta > 3) REJECT(SCD_JPEG_BAD_TABLE);
                if (!hpos[0][td] || !hpos[1][ta] || !qpos[cq[c]]) REJECT(SCD_JPEG_MISSING_TABLE);
                I.dc_off[c] = (int32_t)hpos[0][td];
                I.ac_off[c] = (int32_t)hpos[1][ta];
                I.qt_off[c] = (int32_t)qpos[cq[c]];
                I.qt_prec[c] = qprec[cq[c]];
            }
            const uint8_t* e = s + 1 + 2 * I.ncomp;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) REJECT(SCD_JPEG_MULTISCAN);
            if (I.ncomp == 3) {
                // libjpeg's default_decompress_parms: YCbCr only where it says so with certainty
                const bool ycc = jfif || (adobe && adobe_transform == 1) || (!adobe && cid[0] == 1 && cid[1] == 2 && cid[2] == 3);
                if (!ycc) REJECT(SCD_JPEG_COLOURSPACE);
                if (I.hs == 2 && (I.w + 1) / 2 <= 2) REJECT(SCD_JPEG_CHROMA_WIDTH);
            }
            p += len;
            break;
        }
        p += len;
    }
    // the scan's bytes: up to the first marker that is neither a stuffed zero nor RSTn
    I.scan_off = (int32_t)p;
    int64_t q = p, nr = 0;
    int term = -1;
    while (q < n) {
        const uint8_t* f = (const uint8_t*)memchr(d + q, 0xFF, (size_t)(n - q));
        if (!f) {
            q = n;
            break;
        }
        q = f - d;
        if (q + 1 >= n) {
            q = n;
            break;
        }
        const int m = d[q + 1];
        if (m == 0x00) {
            q += 2;
        } else if (m >= 0xD0 && m <= 0xD7) {
            if (rst && nr < rst_cap) rst[nr] = (int32_t)q;
            ++nr;
            q += 2;
        } else if (m == 0xFF) {
            q += 1;
        } else {
            term = m;
            break;
        }
    }
    I.scan_end = (int32_t)q;
    I.n_restarts = (int32_t)nr;
    I.has_eoi = term == 0xD9;
    if (term == 0xDC) REJECT(SCD_JPEG_DNL);
    if (term >= 0 && term != 0xD9) REJECT(SCD_JPEG_MULTISCAN);
    *out = I;
#undef REJECT
}

extern "C" int scd_jpeg_parse(const uint8_t* data, int64_t len, scd_jpeg_info* info, int32_t* rst_offsets, int64_t rst_cap) {
    SCD_REQUIRE(data && info && len >= 0, "scd_jpeg_parse: null pointer or negative length");
    SCD_REQUIRE(len < INT32_MAX, "scd_jpeg_parse: a file of %lld bytes (limit 2^31 - 1)", (long long)len);
    SCD_REQUIRE(rst_cap >= 0 && (rst_offsets || rst_cap == 0), "scd_jpeg_parse: restart capacity %lld without a buffer", (long long)rst_cap);
    jpeg_parse(data, len, info, rst_offsets, rst_cap);
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ host: batch plan
// An info is only trusted as far as it is consistent with itself and the file's length: the tables are read through it.
static bool info_ok(const scd_jpeg_info& I) {
    if (I.reason != 0 || I.file_len < 4) return false;
    if (I.w < 1 || I.h < 1 || I.w > JPEG_MAX_EDGE || I.h > JPEG_MAX_EDGE || (I.ncomp != 1 && I.ncomp != 3)) return false;
    if (I.ncomp == 3 && !((I.hs == 1 && I.vs == 1) || (I.hs == 2 && I.vs == 1) || (I.hs == 2 && I.vs == 2))) return false;
    if (I.scan_off < 0 || I.scan_off > I.scan_end || I.scan_end > I.file_len || I.restart_interval < 0) return false;
    for (int c = 0; c < I.ncomp; ++c) {
        if (I.qt_prec[c] < 0 || I.qt_prec[c] > 1) return false;
        if (I.qt_off[c] < 0 || (int64_t)I.qt_off[c] + (I.qt_prec[c] ? 128 : 64) > I.file_len) return false;
        if (I.dc_off[c] < 0 || (int64_t)I.dc_off[c] + 16 > I.file_len || I.ac_off[c] < 0 || (int64_t)I.ac_off[c] + 16 > I.file_len) return false;
    }
    return true;
}

static void read_quant(const uint8_t* file, const scd_jpeg_info& I, int c, uint16_t* q) {
    const uint8_t* s = file + I.qt_off[c];
    for (int k = 0; k < 64; ++k) q[k] = I.qt_prec[c] ? (uint16_t)be16(s + 2 * k) : (uint16_t)s[k];
}

static int64_t plane_bytes(const scd_jpeg_info& I) {
    const JpegGeom g = jpeg_geometry(I.w, I.h, I.ncomp, I.hs, I.vs);
    return (int64_t)g.ypw * g.yph + 2 * (int64_t)g.cpw * g.cph;
}

extern "C" int scd_jpeg_batch_plan(const uint8_t* const* files, const scd_jpeg_info* infos, const int64_t* out_offs, int n,
                                   scd_jpeg_desc* descs, uint8_t* tables, int64_t tables_cap, int64_t* tables_bytes, int64_t* data_bytes,
                                   int64_t* ws_bytes) {
    SCD_REQUIRE(files && infos && n >= 1, "scd_jpeg_batch_plan: empty batch");
    SCD_REQUIRE(!descs || (out_offs && tables), "scd_jpeg_batch_plan: descriptors need out_offs and a table buffer");
    std::map<std::string, int32_t> at;        // table bytes -> offset in `tables`: most files of a batch share the standard tables
    int64_t nt = 0, nd = 0, nw = 0;
    auto place = [&](const void* bytes, size_t len, int32_t* off) -> int {
        std::string key((const char*)bytes, len);
        auto it = at.find(key);
        if (it == at.end()) {
            SCD_REQUIRE(nt + (int64_t)len < INT32_MAX, "scd_jpeg_batch_plan: tables too large");
            if (tables) {
                SCD_REQUIRE(nt + (int64_t)len <= tables_cap, "scd_jpeg_batch_plan: table capacity %lld too small", (long long)tables_cap);
                memcpy(tables + nt, bytes, len);
            }
            it = at.emplace(std::move(key), (int32_t)nt).first;
            nt = (int64_t)scd_align((size_t)(nt + (int64_t)len), 16);
        }
        *off = it->second;
        return SCD_OK;
    };
    for (int b = 0; b < n; ++b) {
        const scd_jpeg_info& I = infos[b];
        SCD_REQUIRE(files[b] && info_ok(I), "scd_jpeg_batch_plan: image %d is not device-decodable (reason %d) or its info is inconsistent", b,
                    I.reason);
        scd_jpeg_desc D;
        memset(&D, 0, sizeof(D));
        for (int c = 0; c < I.ncomp; ++c) {
            uint16_t q[64];
            read_quant(files[b], I, c, q);
            int rc = place(q, sizeof(q), &D.qt[c]);
            if (rc) return rc;
            JpegHuff t;
            SCD_REQUIRE(build_huff(files[b] + I.dc_off[c], (int64_t)I.file_len - I.dc_off[c], true, &t),
                        "scd_jpeg_batch_plan: image %d: bad DC Huffman table", b);
            rc = place(&t, sizeof(t), &D.dc[c]);
            if (rc) return rc;
            SCD_REQUIRE(build_huff(files[b] + I.ac_off[c], (int64_t)I.file_len - I.ac_off[c], false, &t),
                        "scd_jpeg_batch_plan: image %d: bad AC Huffman table", b);
            rc = place(&t, sizeof(t), &D.ac[c]);
            if (rc) return rc;
        }
        if (descs) {
            D.data_off = nd;
            D.out_off = out_offs[b];
            D.plane_off = nw;
            D.data_len = I.file_len;
            D.scan_off = I.scan_off;
            D.scan_end = I.scan_end;
            D.has_eoi = I.has_eoi;
            D.w = I.w;
            D.h = I.h;
            D.ncomp = I.ncomp;
            D.hs = I.hs;
            D.vs = I.vs;
            D.restart_interval = I.restart_interval;
            descs[b] = D;
        }
        nd += (int64_t)scd_align((size_t)I.file_len, 16);
        nw += (int64_t)scd_align((size_t)plane_bytes(I), 16);
    }
    if (tables_bytes) *tables_bytes = nt;
    if (data_bytes) *data_bytes = nd;
    if (ws_bytes) *ws_bytes = nw;
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ host: one file on the CPU
extern "C" int scd_jpeg_decode_host(const uint8_t* data, int64_t len, uint8_t* rgb, int64_t rgb_cap, int32_t* status_out) {
    SCD_REQUIRE(data && status_out && len >= 0 && len < INT32_MAX, "scd_jpeg_decode_host: null pointer or bad length");
    scd_jpeg_info I;
    jpeg_parse(data, len, &I, nullptr, 0);
    SCD_REQUIRE(I.reason == 0, "scd_jpeg_decode_host: not device-decodable (reason %d)", I.reason);
    SCD_REQUIRE(rgb && rgb_cap >= 3ll * I.w * I.h, "scd_jpeg_decode_host: %d x %d needs %lld bytes, capacity %lld", I.w, I.h, 3ll * I.w * I.h,
                (long long)rgb_cap);
    JpegHuff hd[3], ha[3];
    uint16_t q[3][64];
    for (int c = 0; c < I.ncomp; ++c) {
        read_quant(data, I, c, q[c]);
        SCD_REQUIRE(build_huff(data + I.dc_off[c], len - I.dc_off[c], true, &hd[c]) && build_huff(data + I.ac_off[c], len - I.ac_off[c], false, &ha[c]),
                    "scd_jpeg_decode_host: bad Huffman table");
    }
    const JpegGeom g = jpeg_geometry(I.w, I.h, I.ncomp, I.hs, I.vs);
    std::vector<uint8_t> planes;
    try {
        planes.resize((size_t)plane_bytes(I));
    } catch (const std::exception&) {       // a header may claim up to 65,535 x 65,535 whatever the file holds
        scd_set_error("scd_jpeg_decode_host: cannot allocate %lld bytes of component planes for %d x %d", (long long)plane_bytes(I), I.w, I.h);
        return SCD_EINVAL;
    }
    uint8_t* pl[3] = {planes.data(), planes.data() + (size_t)g.ypw * g.yph, planes.data() + (size_t)g.ypw * g.yph + (size_t)g.cpw * g.cph};
    const JpegMemSrc src = {data};
    JpegBits b = {0, 0, I.scan_off, I.scan_end, 0};
    int pred[3] = {0, 0, 0};
    const int64_t n_mcu = (int64_t)g.mcus_x * g.mcus_y;
    const int ri = I.restart_interval;
    for (int64_t m = 0; m < n_mcu && !b.err; ++m) {
        if (ri > 0 && m > 0 && m % ri == 0) {
            if (!jpeg_restart(src, b, (int)(m / ri - 1))) break;
            pred[0] = pred[1] = pred[2] = 0;
        }
        const int mx = (int)(m % g.mcus_x), my = (int)(m / g.mcus_x);
        for (int j = 0; j < g.nblk && !b.err; ++j) {
            int comp, pitch;
            long long off;
            jpeg_block_place(g, I.ncomp, I.hs, I.vs, mx, my, j, &comp, &off, &pitch);
            int coef[64], ws[64];
            memset(coef, 0, sizeof(coef));
            if (!jpeg_decode_block(src, b, &hd[comp], &ha[comp], q[comp], k_zigzag, &pred[comp], coef)) break;
            bool ok = true;
            for (int c = 0; c < 8; ++c) ok = jpeg_idct_col(coef, c, ws) && ok;
            if (!ok) {
                b.err = JPEG_ERANGE;
                break;
            }
            for (int r = 0; r < 8; ++r) ok = jpeg_idct_row(ws, r, pl[comp] + off + (long long)r * pitch) && ok;
            if (!ok) b.err = JPEG_ERANGE;
        }
    }
    if (!b.err && !I.has_eoi) b.err = JPEG_EEOF;
    *status_out = b.err;
    if (b.err) return SCD_OK;
    for (int y = 0; y < I.h; ++y)
        for (int x = 0; x < I.w; ++x) {
            uint8_t* o = rgb + ((int64_t)y * I.w + x) * 3;
            const int yy = pl[0][(int64_t)y * g.ypw + x];
            if (I.ncomp == 1) {
                o[0] = o[1] = o[2] = (uint8_t)yy;
            } else {
                jpeg_ycc_rgb(yy, jpeg_chroma(pl[1], g.cpw, I.hs, I.vs, I.w, I.h, x, y), jpeg_chroma(pl[2], g.cpw, I.hs, I.vs, I.w, I.h, x, y), o);
            }
        }
    return SCD_OK;
}

// ------------------------------------------------------------------------------------------------ kernels
#ifdef __HIPCC__
#define JPEG_WIN 2048            // bytes of the scan held in LDS ahead of the lane that walks it
#define JPEG_BLK_STRIDE 72       // ints between the blocks of a group in LDS (64 + 8: the 8 blocks' columns fall on distinct banks)

__constant__ uint8_t c_zigzag[64] = JPEG_ZIGZAG_INIT;

// Byte source of the kernel: the LDS window where it covers `pos`, the file in global memory otherwise (pos < the file's length
// either way: jpeg_fill checks it).
struct JpegWinSrc {
    const uint8_t* g;
    const uint8_t* win;
    int start;
    __host__ __device__ int byte(int pos) const {
        const unsigned o = (unsigned)(pos - start);
        return o < (unsigned)JPEG_WIN ? win[o] : g[pos];
    }
};

__device__ __forceinline__ bool table_ok(int off, int bytes, long long tables_bytes) {
    return off >= 0 && (off & 3) == 0 && (long long)off + bytes <= tables_bytes;
}

// What both kernels check before they touch anything the descriptor points at.
__device__ __forceinline__ bool jpeg_desc_ok(const scd_jpeg_desc& d, const JpegGeom& g, long long planes_bytes) {
    if (d.w < 1 || d.h < 1 || d.w > JPEG_MAX_EDGE || d.h > JPEG_MAX_EDGE || (d.ncomp != 1 && d.ncomp != 3)) return false;
    if (d.ncomp == 3 && !((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
    const long long pb = (long long)g.ypw * g.yph + 2ll * g.cpw * g.cph;
    return d.plane_off >= 0 && (d.plane_off & 15) == 0 && d.plane_off + pb <= planes_bytes;
}

// One wave per image.  Per group of up to 8 blocks (8 / blocks-per-MCU whole MCUs): zero the coefficients and top up the byte window
// (all lanes), decode (lane 0), column pass and row pass (8 lanes per block).
__global__ void __launch_bounds__(64) jpeg_entropy_idct_kernel(const uint8_t* __restrict__ data, long long data_bytes,
                                                               const scd_jpeg_desc* __restrict__ descs, const uint8_t* __restrict__ tables,
                                                               long long tables_bytes, uint8_t* __restrict__ planes, long long planes_bytes,
                                                               long long pixel_bytes, int32_t* __restrict__ status) {
    __shared__ JpegHuff s_h[6];                                   // DC of the components, then AC
    __shared__ uint16_t s_q[3][64];
    __shared__ uint8_t s_zz[64];
    __shared__ int s_coef[8 * JPEG_BLK_STRIDE], s_ws[8 * JPEG_BLK_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t s_win[JPEG_WIN];
    __shared__ int s_pred[3], s_pos, s_status;
    const int img = blockIdx.x, lane = threadIdx.x;
    const scd_jpeg_desc d = descs[img];
    const JpegGeom g = jpeg_geometry(d.w, d.h, d.ncomp, d.hs, d.vs);
    bool ok = jpeg_desc_ok(d, g, planes_bytes);
    ok = ok && d.data_off >= 0 && (d.data_off & 15) == 0 && d.data_len >= 0 && d.data_off + d.data_len <= data_bytes;
    ok = ok && d.scan_off >= 0 && d.scan_off <= d.scan_end && d.scan_end <= d.data_len && d.restart_interval >= 0;
    ok = ok && d.out_off >= 0 && d.out_off + 3ll * d.w * d.h <= pixel_bytes;
    int tq[3], td[3], ta[3];                                      // table offsets, by constant index only (registers)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        tq[c] = d.qt[c];
        td[c] = d.dc[c];
        ta[c] = d.ac[c];
        if (c < d.ncomp)
            ok = ok && table_ok(tq[c], JPEG_QUANT_BYTES, tables_bytes) && table_ok(td[c], JPEG_HUFF_BYTES, tables_bytes) &&
                 table_ok(ta[c], JPEG_HUFF_BYTES, tables_bytes);
    }
    if (!ok) {
        if (lane == 0) status[img] = JPEG_EDESC;
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (c >= d.ncomp) break;
        const uint32_t* sd = (const uint32_t*)(tables + td[c]);
        const uint32_t* sa = (const uint32_t*)(tables + ta[c]);
        for (int i = lane; i < JPEG_HUFF_BYTES / 4; i += 64) {
            ((uint32_t*)&s_h[c])[i] = sd[i];
            ((uint32_t*)&s_h[3 + c])[i] = sa[i];
        }
        if (lane < JPEG_QUANT_BYTES / 4) ((uint32_t*)s_q[c])[lane] = ((const uint32_t*)(tables + tq[c]))[lane];
    }
    s_zz[lane] = c_zigzag[lane];
    if (lane == 0) {
        s_pred[0] = s_pred[1] = s_pred[2] = 0;
        s_pos = d.scan_off;
        s_status = 0;
    }
    const uint8_t* file = data + d.data_off;
    uint8_t* pl = planes + d.plane_off;
    const long long ysz = (long long)g.ypw * g.yph, csz = (long long)g.cpw * g.cph, psz = ysz + 2 * csz;
    const int n_mcu = g.mcus_x * g.mcus_y;                        // <= 8192 x 8192
    const int group = 8 / g.nblk, ri = d.restart_interval, ny = g.nblk == 1 ? 1 : g.nblk - 2;
    JpegBits b = {0, 0, d.scan_off, d.scan_end, 0};              // lane 0's; the other lanes never use theirs
    int win_start = -JPEG_WIN;                                    // nothing loaded
    __syncthreads();
    for (int m0 = 0; m0 < n_mcu; m0 += group) {
        const int mcus = n_mcu - m0 < group ? n_mcu - m0 : group, nb = mcus * g.nblk;
        for (int i = lane; i < 8 * JPEG_BLK_STRIDE; i += 64) s_coef[i] = 0;
        const int pos = s_pos;
        if (pos - win_start > JPEG_WIN / 2) {
            win_start = pos & ~15;
            for (int c = lane; c < JPEG_WIN / 16; c += 64) {
                const long long a = d.data_off + win_start + 16ll * c;
                if (a + 16 <= data_bytes) {
                    *(uint4*)(s_win + 16 * c) = *(const uint4*)(data + a);
                } else {                                          // the section's last bytes
                    for (int k = 0; k < 16; ++k) s_win[16 * c + k] = a + k < data_bytes ? data[a + k] : (uint8_t)0;
                }
            }
        }
        __syncthreads();
        if (lane == 0) {
            const JpegWinSrc src = {file, s_win, win_start};
            for (int gi = 0; gi < mcus && !b.err; ++gi) {
                const int m = m0 + gi;
                if (ri > 0 && m > 0 && m % ri == 0) {
                    if (!jpeg_restart(src, b, m / ri - 1)) break;
                    s_pred[0] = s_pred[1] = s_pred[2] = 0;
                }
                for (int j = 0; j < g.nblk; ++j) {
                    const int c = j < ny ? 0 : 1 + (j - ny);
                    if (!jpeg_decode_block(src, b, &s_h[c], &s_h[3 + c], s_q[c], s_zz, &s_pred[c], s_coef + (gi * g.nblk + j) * JPEG_BLK_STRIDE)) break;
                }
            }
            s_pos = b.pos;
            if (b.err) s_status = b.err;
        }
        __syncthreads();
        if (s_status) break;
        const int blk = lane >> 3, sub = lane & 7;
        if (blk < nb && !jpeg_idct_col(s_coef + blk * JPEG_BLK_STRIDE, sub, s_ws + blk * JPEG_BLK_STRIDE)) s_status = JPEG_ERANGE;
        __syncthreads();
        if (s_status) break;
        if (blk < nb) {
            const int m = m0 + blk / g.nblk;
            int comp, pitch;
            long long off;
            jpeg_block_place(g, d.ncomp, d.hs, d.vs, m % g.mcus_x, m / g.mcus_x, blk % g.nblk, &comp, &off, &pitch);
            off += (comp == 0 ? 0 : (comp == 1 ? ysz : ysz + csz)) + (long long)sub * pitch;
            uint8_t o[8];
            if (!jpeg_idct_row(s_ws + blk * JPEG_BLK_STRIDE, sub, o)) s_status = JPEG_ERANGE;
            if (off >= 0 && off + 8 <= psz)        // the image's own planes (pitches and offsets are multiples of 8)
                *(uint2*)(pl + off) = make_uint2(o[0] | o[1] << 8 | o[2] << 16 | (uint32_t)o[3] << 24, o[4] | o[5] << 8 | o[6] << 16 | (uint32_t)o[7] << 24);
        }
    }
    __syncthreads();
    if (lane == 0) status[img] = s_status ? s_status : (d.has_eoi ? JPEG_OK : JPEG_EEOF);
}

// Fancy upsampling + colour: planes -> uint8 RGB HWC at the image's offset of the pixel section.  grid (row blocks, images).  An image
// whose status is not 0 is left alone.
__global__ void __launch_bounds__(256) jpeg_colour_kernel(const scd_jpeg_desc* __restrict__ descs, const uint8_t* __restrict__ planes,
                                                          long long planes_bytes, const int32_t* __restrict__ status, uint8_t* __restrict__ pixels,
                                                          long long pixel_bytes) {
    const int img = blockIdx.y;
    if (status[img] != 0) return;
    const scd_jpeg_desc d = descs[img];
    const JpegGeom g = jpeg_geometry(d.w, d.h, d.ncomp, d.hs, d.vs);
    // the entropy kernel has checked the same and set the status: nothing is read or written through a descriptor that fails here
    if (!jpeg_desc_ok(d, g, planes_bytes) || d.out_off < 0 || d.out_off + 3ll * d.w * d.h > pixel_bytes) return;
    const uint8_t* py = planes + d.plane_off;
    const uint8_t* pcb = py + (long long)g.ypw * g.yph;
    const uint8_t* pcr = pcb + (long long)g.cpw * g.cph;
    uint8_t* out = pixels + d.out_off;
    for (int y = blockIdx.x; y < d.h; y += gridDim.x)
        for (int x = threadIdx.x; x < d.w; x += 256) {
            uint8_t rgb[3];
            const int yy = py[(long long)y * g.ypw + x];
            if (d.ncomp == 1)
                rgb[0] = rgb[1] = rgb[2] = (uint8_t)yy;
            else
                jpeg_ycc_rgb(yy, jpeg_chroma(pcb, g.cpw, d.hs, d.vs, d.w, d.h, x, y), jpeg_chroma(pcr, g.cpw, d.hs, d.vs, d.w, d.h, x, y), rgb);
            uint8_t* o = out + ((long long)y * d.w + x) * 3;
            o[0] = rgb[0];
            o[1] = rgb[1];
            o[2] = rgb[2];
        }
}

extern "C" int scd_jpeg_decode(scd_handle h, const uint8_t* data, int64_t data_bytes, const scd_jpeg_desc* descs, const uint8_t* tables,
                               int64_t tables_bytes, int n, uint8_t* pixels, int64_t pixel_bytes, int32_t* status, void* ws, size_t ws_bytes,
                               void* stream) {
    SCD_DEVICE_ENTRY(h, "scd_jpeg_decode");
    SCD_REQUIRE(n >= 0 && n <= 65535, "scd_jpeg_decode: batch %d outside 0 .. 65535", n);
    if (n == 0) return SCD_OK;
    SCD_REQUIRE(data && descs && tables && pixels && status && ws, "scd_jpeg_decode: null pointer");
    SCD_REQUIRE(data_bytes >= 0 && tables_bytes >= 0 && pixel_bytes >= 0, "scd_jpeg_decode: negative section size");
    SCD_REQUIRE(((uintptr_t)data & 15) == 0 && ((uintptr_t)tables & 15) == 0 && ((uintptr_t)ws & 15) == 0 && ((uintptr_t)descs & 7) == 0,
                "scd_jpeg_decode: data, tables and ws must be 16-byte aligned, descs 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    jpeg_entropy_idct_kernel<<<n, 64, 0, st>>>(data, data_bytes, descs, tables, tables_bytes, (uint8_t*)ws, (long long)ws_bytes, pixel_bytes, status);
    SCD_LAUNCH_CHECK();
    jpeg_colour_kernel<<<dim3(64, n), 256, 0, st>>>(descs, (const uint8_t*)ws, (long long)ws_bytes, status, pixels, pixel_bytes);
    SCD_LAUNCH_CHECK();
    return SCD_OK;
}
#endif   // __HIPCC__
