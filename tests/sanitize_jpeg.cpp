// Host-side driver for the JPEG parser, table builder and CPU decoder (scd_amd/csrc/jpeg.hip, jpeg.h) under AddressSanitizer +
// UndefinedBehaviorSanitizer: every fixture of tests/golden/jpeg_decode.npz and of tests/golden/jpeg_decode_foreign.npz, the corrupt ones
// included, must get the reason / status the fixture records, and 1,000 seeded single-byte corruptions (one in eight of them in a Huffman table's counts) and truncations of them
// must all return without a sanitizer report.  The functions it drives are the ones the kernels run, so the device sees these bytes
// only after this program has.
//
//   clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__
//       -I/opt/rocm/include -Iinclude -Iscd_amd/csrc scd_amd/csrc/jpeg.hip tests/sanitize_jpeg.cpp -o sanitize_jpeg
//   ./sanitize_jpeg tests/golden/jpeg_decode.npz tests/golden/jpeg_decode_foreign.npz
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "scd_hip.h"

static char g_err[512];
extern "C" const char* scd_last_error(void) { return g_err; }
void scd_set_error(const char* fmt, ...) {      // api.cpp's definition lives beside the HIP entry points
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- the members of an uncompressed .npz (a zip of stored .npy files, zip64 sizes in the extra field)
static uint64_t le(const uint8_t* p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

static bool npz_member(const std::vector<uint8_t>& z, const char* name, const uint8_t** data, size_t* bytes) {
    size_t p = 0;
    while (p + 30 <= z.size() && le(&z[p], 4) == 0x04034b50) {
        const int method = (int)le(&z[p + 8], 2);
        uint64_t csize = le(&z[p + 18], 4);
        const size_t nl = (size_t)le(&z[p + 26], 2), el = (size_t)le(&z[p + 28], 2);
        if (p + 30 + nl + el > z.size()) return false;
        const std::string nm((const char*)&z[p + 30], nl);
        for (size_t e = p + 30 + nl; e + 4 <= p + 30 + nl + el;) {
            const int id = (int)le(&z[e], 2);
            const size_t sz = (size_t)le(&z[e + 2], 2);
            if (id == 1 && sz >= 16) csize = le(&z[e + 12], 8);      // zip64: uncompressed, then compressed size
            e += 4 + sz;
        }
        const size_t body = p + 30 + nl + el;
        if (body + csize > z.size()) return false;
        if (nm == std::string(name) + ".npy") {
            if (method != 0 || csize < 10) return false;
            const uint8_t* a = &z[body];
            const size_t hl = a[6] == 1 ? 10 + (size_t)le(a + 8, 2) : 12 + (size_t)le(a + 8, 4);
            if (hl > csize) return false;
            *data = a + hl;
            *bytes = (size_t)csize - hl;
            return true;
        }
        p = body + (size_t)csize;
    }
    return false;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 24) % n);
}

static long g_calls = 0;

// Parse, plan and decode one byte string held in a heap block of exactly its length (an over-read is a sanitizer report).
// Returns the reason, and the decoder's status through *status (-1 when the parser rejected the file).
static int run_one(const uint8_t* bytes, size_t len, int* status) {
    uint8_t* d = (uint8_t*)malloc(len ? len : 1);
    if (len) memcpy(d, bytes, len);
    scd_jpeg_info info;
    int32_t rst[8];
    *status = -1;
    if (scd_jpeg_parse(d, (int64_t)len, &info, rst, 8) != SCD_OK) {
        free(d);
        return -1;
    }
    ++g_calls;
    if (info.reason == 0) {
        const uint8_t* files[1] = {d};
        const int64_t out_off[1] = {0};
        int64_t tb = 0, db = 0, wb = 0;
        if (scd_jpeg_batch_plan(files, &info, out_off, 1, nullptr, nullptr, 0, &tb, &db, &wb) == SCD_OK) {
            std::vector<uint8_t> tables((size_t)tb + 1);
            scd_jpeg_desc desc;
            scd_jpeg_batch_plan(files, &info, out_off, 1, &desc, tables.data(), tb, &tb, &db, &wb);
        }
        ++g_calls;
        // a corrupted frame header may claim up to 65,535 x 65,535: the callers keep such a file from the decoder (Pillow's pixel
        // limit, scd_amd/jpeg.py), and so does this driver, at 4 M pixels
        if ((int64_t)info.w * info.h <= (1 << 22)) {
            const size_t px = (size_t)info.w * info.h * 3;
            uint8_t* rgb = (uint8_t*)malloc(px);
            int32_t st = -1;
            if (scd_jpeg_decode_host(d, (int64_t)len, rgb, (int64_t)px, &st) == SCD_OK) *status = st;
            ++g_calls;
            free(rgb);
        }
    }
    free(d);
    return info.reason;
}

// The cases of one fixture file: every one must get the reason / status the file records.  Returns the failures, or -1 when the file
// cannot be read.  `fx` receives the file's bytes and case offsets, for the corruption rounds.
struct Fixtures {
    std::vector<uint8_t> z;
    const uint8_t* data = nullptr;
    std::vector<size_t> off;
};

static int run_file(const char* path, Fixtures* fx) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        printf("cannot open %s\n", path);
        return -1;
    }
    std::vector<uint8_t>& z = fx->z;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) z.insert(z.end(), buf, buf + n);
    fclose(f);
    const uint8_t *data, *lens, *meta;
    size_t nb, nl, nm;
    if (!npz_member(z, "data", &data, &nb) || !npz_member(z, "data_len", &lens, &nl) || !npz_member(z, "meta", &meta, &nm)) {
        printf("%s: not the uncompressed fixture file expected\n", path);
        return -1;
    }
    const size_t n = nl / 8;
    if (nm != n * 32) {
        printf("%s: meta has %zu bytes for %zu cases\n", path, nm, n);
        return -1;
    }
    fx->data = data;
    fx->off.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) fx->off[i + 1] = fx->off[i] + (size_t)le(lens + 8 * i, 8);
    if (fx->off[n] != nb) {
        printf("%s: data has %zu bytes, lengths sum to %zu\n", path, nb, fx->off[n]);
        return -1;
    }
    int failures = 0;
    for (size_t i = 0; i < n; ++i) {
        int st;
        const int reason = run_one(data + fx->off[i], fx->off[i + 1] - fx->off[i], &st);
        const int want_reason = (int)(int32_t)le(meta + 32 * i, 4), want_status = (int)(int32_t)le(meta + 32 * i + 4, 4);
        if (reason != want_reason || (reason == 0 && st != want_status)) {
            printf("%s case %zu: reason %d status %d, expected %d / %d\n", path, i, reason, st, want_reason, want_status);
            ++failures;
        }
    }
    return failures;
}

// Usage: sanitize_jpeg [fixture file ...].  Every case of every file is run; the corruptions are drawn from the first file's cases.
int main(int argc, char** argv) {
    const char* fallback[] = {argv[0], "tests/golden/jpeg_decode.npz"};
    if (argc < 2) {
        argv = (char**)fallback;
        argc = 2;
    }
    std::vector<Fixtures> files((size_t)argc - 1);
    int failures = 0;
    size_t fixtures = 0;
    for (int a = 1; a < argc; ++a) {
        const int r = run_file(argv[a], &files[(size_t)a - 1]);
        if (r < 0) return 2;
        failures += r;
        fixtures += files[(size_t)a - 1].off.size() - 1;
    }
    const uint8_t* data = files[0].data;
    const std::vector<size_t>& off = files[0].off;
    const size_t n = off.size() - 1;
    int accepted = 0, rejected = 0, status_nz = 0;
    for (int t = 0; t < 1000; ++t) {
        const size_t i = rnd((uint32_t)n);
        std::vector<uint8_t> v(data + off[i], data + off[i + 1]);
        size_t dht = 0;
        for (size_t k = 2; k + 21 < v.size() && !dht; ++k)
            if (v[k] == 0xFF && v[k + 1] == 0xC4) dht = k;
        if (t % 4 == 3) {
            v.resize(rnd((uint32_t)v.size() + 1));
        } else if (t % 8 == 1 && dht) {
            // a count byte of the first Huffman table: over- and under-subscribed tables, symbol lists past the segment
            v[dht + 5 + rnd(16)] = (uint8_t)rnd(256);
        } else {
            // three in four corruptions fall inside the scan, where the entropy decoder is the one that has to cope
            const size_t lo = t % 4 == 0 ? 0 : v.size() / 3;
            v[lo + rnd((uint32_t)(v.size() - lo))] = (uint8_t)rnd(256);
        }
        int st;
        const int reason = run_one(v.data(), v.size(), &st);
        if (reason != 0)
            ++rejected;
        else if (st != 0)
            ++status_nz;
        else
            ++accepted;
    }
    printf("%zu fixtures, 1000 corruptions (%d decoded, %d parser rejects, %d decoder rejects), %ld calls returned, %d failures\n", fixtures, accepted,
           rejected, status_nz, g_calls, failures);
    return failures ? 1 : 0;
}
