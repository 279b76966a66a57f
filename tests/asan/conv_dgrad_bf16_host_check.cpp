// Host-side sanitizer run of the bf16 direct convolution data gradient's C ABI
// (include/mcgmil_conv_dgrad_bf16.h). Built by tests/asan/build_conv_dgrad_bf16.sh (from
// tests/test_conv_dgrad_bf16_capi_sanitizers.py): mcgmil_conv_dgrad_bf16.hip and the sources it
// links against with -fsanitize=address,undefined on the host pass only (no GPU needed). Every
// call below returns before any launch: argument validation, error codes and messages, the limits
// of dx and dy, and the class arithmetic of mcgmil_conv_dgrad_classes_bf16 over a sweep of
// geometries, against a brute-force count and including sizes that would overflow 32 bits (and
// 64). Exits 0 when every expectation holds; the sanitizers abort on the first memory or UB error.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "mcgmil_conv_dgrad_bf16.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void* fake(uintptr_t p) { return reinterpret_cast<void*>(p); }   // never dereferenced on the host

static mcgmil_conv_dgrad_bf16_args base_args() {
    mcgmil_conv_dgrad_bf16_args g;
    memset(&g, 0, sizeof g);
    mcgmil_conv_args& a = g.fwd;
    a.batch = 4; a.height = 56; a.width = 56; a.in_channels = 64; a.out_channels = 128;
    a.kernel_h = a.kernel_w = 3; a.stride = 2; a.pad = 1;
    g.dy = fake(0x20000);
    g.w_t = fake(0x30000);
    g.dx = fake(0x40000);
    return g;
}

static void expect_error(int rc, int code, const char* fragment = nullptr) {
    EXPECT(rc == code);
    const char* msg = mcgmil_last_error();
    EXPECT(msg != nullptr && strlen(msg) > 0);
    if (fragment && msg) EXPECT(strstr(msg, fragment) != nullptr);
}

// The documented classes, counted by brute force over the input rows, columns and taps.
static void brute(const mcgmil_conv_args& a, int32_t taps[4], int64_t pixels[4]) {
    for (int c = 0; c < 4; ++c) taps[c] = 0, pixels[c] = 0;
    const int s = a.stride;
    for (int rh = 0; rh < s; ++rh)
        for (int rw = 0; rw < s; ++rw) {
            int th = 0, tw = 0, nh = 0, nw = 0;
            for (int kh = 0; kh < a.kernel_h; ++kh) th += kh % s == rh;
            for (int kw = 0; kw < a.kernel_w; ++kw) tw += kw % s == rw;
            for (int ih = 0; ih < a.height; ++ih) nh += (ih + a.pad) % s == rh;
            for (int iw = 0; iw < a.width; ++iw) nw += (iw + a.pad) % s == rw;
            taps[rh * s + rw] = th * tw;
            pixels[rh * s + rw] = (int64_t)a.batch * nh * nw;
        }
}

static void classes() {
    for (int batch : {1, 3, 64, 1507})
        for (int h : {1, 2, 7, 56, 113})
            for (int cin : {64, 128, 192, 512})
                for (int kh : {1, 2, 3, 7})
                    for (int kw : {1, 3, 6})
                        for (int stride : {1, 2})
                            for (int pad : {0, 1, 2, 5}) {
                                if (pad >= kh || pad >= kw) continue;
                                mcgmil_conv_dgrad_bf16_args g = base_args();
                                g.fwd.batch = batch; g.fwd.height = h; g.fwd.width = h + 1;
                                g.fwd.in_channels = cin; g.fwd.kernel_h = kh; g.fwd.kernel_w = kw;
                                g.fwd.stride = stride; g.fwd.pad = pad;
                                if (h + 2 * pad < kh || h + 1 + 2 * pad < kw) continue;
                                int32_t taps[4], want_taps[4];
                                int64_t pixels[4], tiles[4], want_pixels[4];
                                const int rc = mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles);
                                // a dx or dy of 2^31 bytes or more (1507 x 113 x 114 x 512 bf16): refused, not wrapped
                                const int64_t oh = (h + 2 * pad - kh) / stride + 1, ow = (h + 1 + 2 * pad - kw) / stride + 1;
                                const bool big = (int64_t)batch * h * (h + 1) * cin * 2 >= (1ll << 31) ||
                                                 (int64_t)batch * oh * ow * g.fwd.out_channels * 2 >= (1ll << 31);
                                EXPECT(rc == (big ? MCGMIL_E_UNSUPPORTED : MCGMIL_OK));
                                if (rc != MCGMIL_OK) continue;
                                brute(g.fwd, want_taps, want_pixels);
                                const int64_t tile = cin == 64 ? 256 : 128;
                                int64_t total = 0;
                                int32_t all_taps = 0;
                                for (int c = 0; c < 4; ++c) {
                                    EXPECT(taps[c] == want_taps[c]);
                                    EXPECT(pixels[c] == want_pixels[c]);
                                    EXPECT(tiles[c] == (pixels[c] + tile - 1) / tile);
                                    total += pixels[c];
                                    all_taps += taps[c];
                                }
                                EXPECT(total == (int64_t)batch * h * (h + 1));     // every input pixel once
                                EXPECT(all_taps == kh * kw);                        // every tap once
                            }
    EXPECT(mcgmil_conv_dgrad_bf16_args_size() == sizeof(mcgmil_conv_dgrad_bf16_args));
}

static void limits() {
    // sizes whose products leave 32 or 64 bits or the supported range: an error, never a wrapped size
    int32_t taps[4] = {7, 7, 7, 7};
    int64_t pixels[4], tiles[4];
    mcgmil_conv_dgrad_bf16_args g = base_args();
    g.fwd.batch = 0x7fffffff; g.fwd.height = 0x7fffffff; g.fwd.width = 0x7fffffff;      // pixels leave 64 bits
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 1 << 20; g.fwd.height = 128; g.fwd.width = 128;                        // 2^32 pixels per class
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 16; g.fwd.height = 1024; g.fwd.width = 1024;                           // dx of exactly 2^31 bytes
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED, "2^31 bytes");
    g.fwd.batch = 15;                                                                    // one image less: fine
    EXPECT(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles) == MCGMIL_OK);
    EXPECT(pixels[0] == 15ll << 18 && pixels[3] == 15ll << 18 && tiles[0] == 15ll << 10 && taps[0] == 4 && taps[3] == 1);
    taps[0] = taps[3] = 7;
    g = base_args();
    g.fwd.batch = 4; g.fwd.height = 1024; g.fwd.width = 1024; g.fwd.out_channels = 256;
    g.fwd.kernel_h = g.fwd.kernel_w = 1; g.fwd.stride = 1; g.fwd.pad = 0;                // dy of exactly 2^31 bytes
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED, "2^31 bytes");
    g.fwd.height = 1023;                                                                 // one row less: fine
    EXPECT(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles) == MCGMIL_OK);
    EXPECT(pixels[0] == 1023ll << 12 && pixels[1] == 0 && taps[0] == 1 && taps[1] == 0);
    taps[0] = taps[1] = taps[3] = 7;
    g = base_args();
    g.fwd.in_channels = 0x7fffffc0; g.fwd.out_channels = 0x7fffffc0; g.fwd.kernel_h = g.fwd.kernel_w = 7;
    g.fwd.pad = 3;                                                                       // dx and the weight leave 64 bits
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 1; g.fwd.height = 7; g.fwd.width = 7;
    g.fwd.in_channels = 1 << 16; g.fwd.out_channels = 1 << 16; g.fwd.kernel_h = g.fwd.kernel_w = 7;
    g.fwd.pad = 3;                                                                       // 2^32 * 49 weights
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED, "weight too large");
    g = base_args();
    g.fwd.height = 0x7fffffff; g.fwd.width = 1; g.fwd.pad = 0x7fffffff;                  // 2 * pad leaves 32 bits
    EXPECT(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles) != MCGMIL_OK);
    g = base_args();
    g.fwd.batch = 0x7fffffff; g.fwd.height = 1; g.fwd.width = 1; g.fwd.in_channels = 0x7fffffc0;
    g.fwd.out_channels = 64; g.fwd.kernel_h = g.fwd.kernel_w = 1; g.fwd.stride = 1; g.fwd.pad = 0;
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_UNSUPPORTED);
    EXPECT(taps[0] == 7 && taps[3] == 7);                                                // outputs untouched on error
}

static void errors() {
    int32_t taps[4];
    int64_t pixels[4], tiles[4];
    expect_error(mcgmil_conv_dgrad_classes_bf16(nullptr, taps, pixels, tiles), MCGMIL_E_INVALID, "NULL");
    expect_error(mcgmil_conv2d_dgrad_bf16(nullptr, nullptr), MCGMIL_E_INVALID, "NULL");
    mcgmil_conv_dgrad_bf16_args g = base_args();
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, nullptr, pixels, tiles), MCGMIL_E_INVALID);
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, nullptr, tiles), MCGMIL_E_INVALID);
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, nullptr), MCGMIL_E_INVALID);
    g.fwd.batch = 0; expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_INVALID); g = base_args();
    g.fwd.height = 0; expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_INVALID); g = base_args();
    g.fwd.in_channels = 48; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "in_channels"); g = base_args();
    g.fwd.in_channels = 16; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "in_channels"); g = base_args();
    g.fwd.in_channels = 0; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "in_channels"); g = base_args();
    g.fwd.out_channels = 32; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "out_channels"); g = base_args();
    g.fwd.out_channels = 96; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "out_channels"); g = base_args();
    g.fwd.kernel_h = 8; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "kernel size"); g = base_args();
    g.fwd.kernel_w = 0; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "kernel size"); g = base_args();
    g.fwd.stride = 3; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "stride"); g = base_args();
    g.fwd.stride = 0; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "stride"); g = base_args();
    g.fwd.pad = 3; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "pad"); g = base_args();
    g.fwd.pad = -1; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "pad"); g = base_args();
    g.fwd.height = 1; g.fwd.width = 1; g.fwd.pad = 0;
    expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "does not fit"); g = base_args();
    g.reserved = 1; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "reserved");
    expect_error(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles), MCGMIL_E_INVALID, "reserved");
    // the validation order: reserved, then channels, then stride, then pad, then the fit
    g.fwd.in_channels = 96; g.fwd.stride = 3; g.fwd.pad = 3;
    expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "reserved");
    g.reserved = 0; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "in_channels");
    g.fwd.in_channels = 64; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "stride");
    g.fwd.stride = 2; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_UNSUPPORTED, "pad"); g = base_args();
    // the forward call's x, w, y, stats, in_ab, workspace, flags and reserved are ignored, not validated
    g.fwd.flags = 0x7fff; g.fwd.reserved = 9; g.fwd.w = fake(0x3); g.fwd.y = fake(0x5); g.fwd.x = fake(0x7);
    g.fwd.in_ab = static_cast<const float*>(fake(0x9));
    EXPECT(mcgmil_conv_dgrad_classes_bf16(&g, taps, pixels, tiles) == MCGMIL_OK && taps[0] == 4); g = base_args();

    // mcgmil_conv2d_dgrad_bf16: every pointer / alignment check (a supported geometry never launches
    // with one of them wrong)
    g.dy = nullptr; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.w_t = nullptr; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dx = nullptr; expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dy = fake(0x20002); expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "aligned"); g = base_args();
    g.w_t = fake(0x30008); expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "aligned"); g = base_args();
    g.dx = fake(0x40004); expect_error(mcgmil_conv2d_dgrad_bf16(&g, nullptr), MCGMIL_E_INVALID, "aligned");
}

int main() {
    classes();
    limits();
    errors();
    printf("conv_dgrad_bf16_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
