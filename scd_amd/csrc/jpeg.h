// Baseline JPEG decoding, bit-equal to libjpeg-turbo's default path (Pillow's Image.open(f).convert('RGB')): the entropy decoder and
// the integer arithmetic behind it, as functions that compile for the host and for gfx950 from one text (docs/design/ingest.md).
// The kernels of jpeg.hip and scd_jpeg_decode_host call exactly these, so what the CPU tests and the host sanitizers see is what
// the device runs.
//
//   Huffman decode, DC prediction, dequantisation     jdhuff.c (decode_mcu_slow's rules; no look-ahead past a marker)
//   IDCT                                              jidctint.c jpeg_idct_islow, CONST_BITS 13, PASS1_BITS 2
//   chroma upsampling                                 jdsample.c h2v1_fancy_upsample / h2v2_fancy_upsample
//   colour                                            jdcolor.c ycc_rgb_convert (16-bit fixed point tables)
//
// All arithmetic is int32 with arithmetic right shifts.  The range guard (|dequantised coefficient| <= 4096, |column-pass output| <=
// 8192) keeps every partial sum below 1.5e9 and every value libjpeg-turbo's SIMD code keeps in a 16-bit lane inside it; its third
// bound (row-pass output in [-512, 511]) keeps the samples where the C code's range-limit table and the SIMD code's saturation
// agree.  So the C, SIMD and this restatement agree; an image that trips the guard is decoded by Pillow on the host instead.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JPEG_HD __host__ __device__ __forceinline__
#define JPEG_HD_MEMBER __host__ __device__ __forceinline__
#else
#define JPEG_HD static inline
#define JPEG_HD_MEMBER inline
#endif

// per-image status of the decoders (scd_hip.h: SCD_JPEG_E*)
#define JPEG_OK 0
#define JPEG_EHUFF 1       // a bit pattern that is no code of the table
#define JPEG_EINDEX 2      // a run that puts a coefficient past index 63
#define JPEG_EEOF 3        // the scan needs bytes past the end of the file, or the file has no EOI behind the scan
#define JPEG_EMARKER 4     // a marker other than the expected RSTn inside the scan, or 0xFF 0xFF fill
#define JPEG_ERANGE 5      // the range guard
#define JPEG_EDESC 6       // a descriptor that reaches outside its buffers (device only)

#define JPEG_MAX_COEF 4096
#define JPEG_MAX_WS 8192
#define JPEG_MAX_OUT 511

// A derived Huffman table (jdhuff.c jpeg_make_d_derived_tbl): look[top 8 bits] = (length << 8) | symbol for codes of up to 8 bits, 0
// otherwise; maxcode[l] = largest code of length l or -1; valoff[l] = index of the first symbol of length l minus its code.
struct JpegHuff {
    uint16_t look[256];
    int32_t maxcode[17];
    int32_t valoff[17];
    uint8_t huffval[256];
};
#define JPEG_HUFF_BYTES 904
#define JPEG_QUANT_BYTES 128      // uint16 [64] in zigzag (file) order
// zigzag index -> natural index (jpeg_natural_order): the one list behind the host's table and the kernel's __constant__ copy
#define JPEG_ZIGZAG_INIT                                                                                                              \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

struct JpegBits {
    uint32_t acc;      // the low `nbits` bits are unread
    int nbits;
    int pos, end;      // next byte of the scan, end of the scan's bytes (the marker that ends it, or the file's length)
    int err;
};

// Byte source of the host: the file itself.  (The kernel's source reads through an LDS window, jpeg.hip.)
struct JpegMemSrc {
    const uint8_t* p;
    JPEG_HD_MEMBER int byte(int pos) const { return p[pos]; }
};

// At least `need` (<= 16) unread bits.  Bytes are fetched only when needed, so a valid stream never reads past its last byte or into
// a marker.  hard = false: stop quietly where the scan's bytes end (the look-ahead of jpeg_huff_decode).
template <class Src>
JPEG_HD bool jpeg_fill(const Src& src, JpegBits& b, int need, bool hard) {
    for (int it = 0; it < 3 && b.nbits < need; ++it) {
        if (b.pos >= b.end) {
            if (hard) b.err = JPEG_EEOF;
            return false;
        }
        const int c = src.byte(b.pos);
        if (c == 0xFF) {
            if (b.pos + 1 >= b.end) {
                if (hard) b.err = JPEG_EEOF;
                return false;
            }
            if (src.byte(b.pos + 1) != 0) {
                if (hard) b.err = JPEG_EMARKER;
                return false;
            }
            b.pos += 2;
        } else {
            b.pos += 1;
        }
        b.acc = (b.acc << 8) | (uint32_t)c;
        b.nbits += 8;
    }
    return b.nbits >= need;
}

// One Huffman symbol, or -1 with b.err set.
template <class Src>
JPEG_HD int jpeg_huff_decode(const Src& src, JpegBits& b, const JpegHuff* t) {
    int len = 1;
    if (jpeg_fill(src, b, 8, false)) {
        const int look = t->look[(b.acc >> (b.nbits - 8)) & 255];
        if (look) {
            b.nbits -= look >> 8;
            return look & 255;
        }
        len = 9;
    }
    for (; len <= 16; ++len) {
        if (!jpeg_fill(src, b, len, true)) return -1;
        const int code = (int)((b.acc >> (b.nbits - len)) & ((1u << len) - 1u));
        if (code <= t->maxcode[len]) {
            b.nbits -= len;
            return t->huffval[(t->valoff[len] + code) & 255];
        }
    }
    b.err = JPEG_EHUFF;
    return -1;
}

// s (1 .. 15) further bits as a signed value (HUFF_EXTEND).  False with b.err set when the scan ends first.
template <class Src>
JPEG_HD bool jpeg_receive_extend(const Src& src, JpegBits& b, int s, int* out) {
    if (!jpeg_fill(src, b, s, true)) return false;
    const int r = (int)((b.acc >> (b.nbits - s)) & ((1u << s) - 1u));
    b.nbits -= s;
    *out = r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
    return true;
}

// One 8x8 block: coef[64] (zeroed by the caller, natural order) receives the dequantised coefficients.  q: the component's table in
// zigzag order; zz: zigzag index -> natural index; pred: the component's DC predictor.  At most 64 symbols.
template <class Src>
JPEG_HD bool jpeg_decode_block(const Src& src, JpegBits& b, const JpegHuff* dc, const JpegHuff* ac, const uint16_t* q, const uint8_t* zz,
                               int* pred, int* coef) {
    int s = jpeg_huff_decode(src, b, dc);
    if (s < 0) return false;
    s &= 15;
    int v = 0;
    if (s && !jpeg_receive_extend(src, b, s, &v)) return false;
    const int p = *pred + v;
    if (p < -32768 || p > 32767) {       // libjpeg keeps the coefficient in 16 bits
        b.err = JPEG_ERANGE;
        return false;
    }
    *pred = p;
    v = p * (int)q[0];
    if (v < -JPEG_MAX_COEF || v > JPEG_MAX_COEF) {
        b.err = JPEG_ERANGE;
        return false;
    }
    coef[0] = v;
    int k = 1;
    for (int it = 0; it < 63 && k < 64; ++it) {
        const int rs = jpeg_huff_decode(src, b, ac);
        if (rs < 0) return false;
        const int r = rs >> 4;
        s = rs & 15;
        if (s) {
            k += r;
            if (k > 63) {
                b.err = JPEG_EINDEX;
                return false;
            }
            if (!jpeg_receive_extend(src, b, s, &v)) return false;
            v *= (int)q[k];
            if (v < -JPEG_MAX_COEF || v > JPEG_MAX_COEF) {
                b.err = JPEG_ERANGE;
                return false;
            }
            coef[zz[k]] = v;
            k += 1;
        } else {
            if (r != 15) break;
            k += 16;
        }
    }
    return true;
}

// Restart number n (0, 1, ...) is due: the unread bits are padding, the next two bytes are 0xFF 0xD0 + (n & 7).
template <class Src>
JPEG_HD bool jpeg_restart(const Src& src, JpegBits& b, int n) {
    b.acc = 0;
    b.nbits = 0;
    if (b.pos + 2 > b.end) {
        b.err = JPEG_EEOF;
        return false;
    }
    if (src.byte(b.pos) != 0xFF || src.byte(b.pos + 1) != 0xD0 + (n & 7)) {
        b.err = JPEG_EMARKER;
        return false;
    }
    b.pos += 2;
    return true;
}

// ---------------------------------------------------------------------------------------------------- IDCT (jidctint.c)
// One pass over 8 values at stride `st` of `in`; shift 11 for the column pass, 18 for the row pass.
JPEG_HD void jpeg_idct_1d(const int* in, int st, int shift, int* o) {
    int z2 = in[2 * st], z3 = in[6 * st];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 - z3 * 15137;
    int tmp3 = z1 + z2 * 6270;
    z2 = in[0];
    z3 = in[4 * st];
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7 * st];
    tmp1 = in[5 * st];
    tmp2 = in[3 * st];
    tmp3 = in[1 * st];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int rnd = 1 << (shift - 1);
    o[0] = (tmp10 + tmp3 + rnd) >> shift;
    o[7] = (tmp10 - tmp3 + rnd) >> shift;
    o[1] = (tmp11 + tmp2 + rnd) >> shift;
    o[6] = (tmp11 - tmp2 + rnd) >> shift;
    o[2] = (tmp12 + tmp1 + rnd) >> shift;
    o[5] = (tmp12 - tmp1 + rnd) >> shift;
    o[3] = (tmp13 + tmp0 + rnd) >> shift;
    o[4] = (tmp13 - tmp0 + rnd) >> shift;
}

// Column c of a block: coef[64] -> ws[64] (column c of it).  False when the range guard trips.
JPEG_HD bool jpeg_idct_col(const int* coef, int c, int* ws) {
    int o[8];
    jpeg_idct_1d(coef + c, 8, 11, o);
    bool ok = true;
    for (int r = 0; r < 8; ++r) {
        ws[8 * r + c] = o[r];
        ok = ok && o[r] >= -JPEG_MAX_WS && o[r] <= JPEG_MAX_WS;
    }
    return ok;
}

// libjpeg's range-limit table on the 10 low bits: the wrap is part of the contract, not a clamp.
JPEG_HD int jpeg_range_limit(int x) {
    const int v = x & 1023;
    return v < 128 ? 128 + v : (v < 512 ? 255 : (v < 896 ? 0 : v - 896));
}

// Row r of a block: ws[64] -> 8 samples.  False when an output leaves [-512, 511]: there the table's wrap and the saturating packs
// of libjpeg-turbo's SIMD IDCT give different samples, so which one Pillow shows depends on the host it runs on.
JPEG_HD bool jpeg_idct_row(const int* ws, int r, uint8_t* out8) {
    int o[8];
    jpeg_idct_1d(ws + 8 * r, 1, 18, o);
    bool ok = true;
    for (int c = 0; c < 8; ++c) {
        out8[c] = (uint8_t)jpeg_range_limit(o[c]);
        ok = ok && o[c] >= -JPEG_MAX_OUT - 1 && o[c] <= JPEG_MAX_OUT;
    }
    return ok;
}

// ---------------------------------------------------------------------------------------------------- upsampling and colour
// Chroma sample of output pixel (x, y) from plane p (row pitch pw) of an image w x h whose luma sampling is hs x vs.
JPEG_HD int jpeg_chroma(const uint8_t* p, int pw, int hs, int vs, int w, int h, int x, int y) {
    if (hs == 1) return p[(long long)y * pw + x];
    const int dw = (w + 1) >> 1, i = x >> 1;
    if (vs == 1) {
        const uint8_t* row = p + (long long)y * pw;
        const int v = row[i];
        if (x & 1) return x == 2 * dw - 1 ? v : (3 * v + row[i + 1] + 2) >> 2;
        return x == 0 ? v : (3 * v + row[i - 1] + 1) >> 2;
    }
    const int ch = (h + 1) >> 1, cy = y >> 1;
    int ny = (y & 1) ? cy + 1 : cy - 1;       // the neighbour row, clamped to the real chroma rows
    ny = ny < 0 ? 0 : (ny > ch - 1 ? ch - 1 : ny);
    const uint8_t* r0 = p + (long long)cy * pw;
    const uint8_t* r1 = p + (long long)ny * pw;
    const int s = 3 * r0[i] + r1[i];
    if (x & 1) return x == 2 * dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * r0[i + 1] + r1[i + 1] + 7) >> 4;
    return x == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * r0[i - 1] + r1[i - 1] + 8) >> 4;
}

JPEG_HD uint8_t jpeg_clamp8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

JPEG_HD void jpeg_ycc_rgb(int y, int cb, int cr, uint8_t* rgb) {
    cb -= 128;
    cr -= 128;
    rgb[0] = jpeg_clamp8(y + ((91881 * cr + 32768) >> 16));
    rgb[1] = jpeg_clamp8(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    rgb[2] = jpeg_clamp8(y + ((116130 * cb + 32768) >> 16));
}

// ---------------------------------------------------------------------------------------------------- geometry
struct JpegGeom {
    int mcus_x, mcus_y;     // MCUs per row, MCU rows
    int nblk;               // blocks per MCU
    int ypw, yph;           // luma plane: pitch and rows (whole MCUs)
    int cpw, cph;           // chroma planes (0 for grayscale)
};

JPEG_HD JpegGeom jpeg_geometry(int w, int h, int ncomp, int hs, int vs) {
    JpegGeom g;
    if (ncomp == 1) hs = vs = 1;
    g.mcus_x = (w + 8 * hs - 1) / (8 * hs);
    g.mcus_y = (h + 8 * vs - 1) / (8 * vs);
    g.nblk = ncomp == 1 ? 1 : hs * vs + 2;
    g.ypw = g.mcus_x * 8 * hs;
    g.yph = g.mcus_y * 8 * vs;
    g.cpw = ncomp == 1 ? 0 : g.mcus_x * 8;
    g.cph = ncomp == 1 ? 0 : g.mcus_y * 8;
    return g;
}

// Block j of an MCU at (mx, my): its component (0 Y, 1 Cb, 2 Cr) and the offset of its top-left sample in that component's plane.
JPEG_HD void jpeg_block_place(const JpegGeom& g, int ncomp, int hs, int vs, int mx, int my, int j, int* comp, long long* off, int* pitch) {
    if (ncomp == 1) hs = vs = 1;
    const int ny = hs * vs;
    if (j < ny) {
        const int bx = j % hs, by = j / hs;
        *comp = 0;
        *pitch = g.ypw;
        *off = (long long)((my * vs + by) * 8) * g.ypw + (mx * hs + bx) * 8;
    } else {
        *comp = 1 + (j - ny);
        *pitch = g.cpw;
        *off = (long long)(my * 8) * g.cpw + mx * 8;
    }
}
