// Host-side sanitizer run of the bf16x3 convolution weight gradient's C ABI
// (include/mcgmil_conv_grad_x3.h). Built by tests/asan/build_conv_grad_x3.sh (from
// tests/test_conv_grad_x3_capi_sanitizers.py): mcgmil_conv_grad_x3.hip and the sources it links against
// with -fsanitize=address,undefined on the host pass only (no GPU needed). Every call below
// returns before any launch: argument validation, error codes and messages, and the
// workspace-size arithmetic over a sweep of geometries, including sizes that would overflow 32
// bits (and 64). Exits 0 when every expectation holds; the sanitizers abort on the first memory
// or UB error.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "mcgmil_conv_grad_x3.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void* fake(uintptr_t p) { return reinterpret_cast<void*>(p); }   // never dereferenced on the host

static mcgmil_conv_grad_args base_args() {
    mcgmil_conv_grad_args g;
    memset(&g, 0, sizeof g);
    mcgmil_conv_args& a = g.fwd;
    a.batch = 4; a.height = 56; a.width = 56; a.in_channels = 64; a.out_channels = 64;
    a.kernel_h = a.kernel_w = 3; a.stride = 1; a.pad = 1;
    a.x = fake(0x10000);
    g.dy = static_cast<const float*>(fake(0x20000));
    g.dw = static_cast<float*>(fake(0x30000));
    return g;
}

static void expect_error(int rc, int code) {
    EXPECT(rc == code);
    const char* msg = mcgmil_last_error();
    EXPECT(msg != nullptr && strlen(msg) > 0);
}

// The documented workspace formula, restated: (1 + granules per chunk) * E fp32 words.
static unsigned long long expected_bytes(const mcgmil_conv_grad_args& g) {
    const mcgmil_conv_args& a = g.fwd;
    const long long oh = (a.height + 2LL * a.pad - a.kernel_h) / a.stride + 1;
    const long long ow = (a.width + 2LL * a.pad - a.kernel_w) / a.stride + 1;
    const long long P = a.batch * oh * ow;
    const long long E = (long long)a.out_channels * a.kernel_h * a.kernel_w * a.in_channels;
    const long long total = (P + MCGMIL_WGRAD_GRANULE_PIXELS - 1) / MCGMIL_WGRAD_GRANULE_PIXELS;
    long long gc = g.chunk_pixels ? g.chunk_pixels / MCGMIL_WGRAD_GRANULE_PIXELS
                                  : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / (E * 4);
    if (gc < 1) gc = 1;
    if (gc > total) gc = total;
    return (unsigned long long)(gc + 1) * E * 4;
}

static void sizes() {
    for (int batch : {1, 3, 64, 1507})
        for (int hw : {1, 7, 56, 112})
            for (int cin : {32, 64, 96, 512})
                for (int cout : {64, 192, 512, 2048})
                    for (int k : {1, 3, 7})
                        for (int stride : {1, 2})
                            for (long long cap : {0LL, 1LL, 2048LL, 10000LL, 1LL << 40}) {
                                mcgmil_conv_grad_args g = base_args();
                                g.fwd.batch = batch; g.fwd.height = hw; g.fwd.width = hw + 1;
                                g.fwd.in_channels = cin; g.fwd.out_channels = cout;
                                g.fwd.kernel_h = g.fwd.kernel_w = k; g.fwd.stride = stride; g.fwd.pad = k / 2;
                                g.chunk_pixels = cap;
                                size_t n = 0;
                                const int rc = mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n);
                                EXPECT(rc == MCGMIL_OK);
                                if (rc == MCGMIL_OK) {
                                    EXPECT(n == expected_bytes(g));
                                    EXPECT(n % 256 == 0);
                                }
                            }
    // the r50 layer-1 output of a config-5 bag: 4.8 GB of dy, offsets past 32 bits, still supported
    mcgmil_conv_grad_args g = base_args();
    g.fwd.batch = 1507; g.fwd.in_channels = 64; g.fwd.out_channels = 256; g.fwd.kernel_h = g.fwd.kernel_w = 1;
    g.fwd.pad = 0;
    size_t n = 0;
    EXPECT(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n) == MCGMIL_OK && n == expected_bytes(g));
    // a smaller cap needs a smaller workspace, never a larger one
    size_t small = 0;
    g.chunk_pixels = MCGMIL_WGRAD_GRANULE_PIXELS;
    EXPECT(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &small) == MCGMIL_OK && small < n);
    EXPECT(small == 2ull * 256 * 64 * 4);
}

static void overflow() {
    // sizes whose products leave 32 or 64 bits or the supported range: an error, never a wrapped size
    size_t n = 12345;
    mcgmil_conv_grad_args g = base_args();
    g.fwd.batch = 0x7fffffff; g.fwd.height = 0x7fffffff; g.fwd.width = 0x7fffffff;      // pixels leave 64 bits
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 1 << 20; g.fwd.height = 64; g.fwd.width = 64;                          // 2^32 pixels
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 1; g.fwd.height = 46341; g.fwd.width = 46341; g.fwd.kernel_h = g.fwd.kernel_w = 1;
    g.fwd.pad = 0;                                                                       // just past 2^31 pixels
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.in_channels = 0x7ffffff0; g.fwd.out_channels = 0x7fffffc0; g.fwd.kernel_h = g.fwd.kernel_w = 7;
    g.fwd.pad = 3;                                                                       // weight leaves 64 bits
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.in_channels = 1 << 16; g.fwd.out_channels = 1 << 16; g.fwd.kernel_h = g.fwd.kernel_w = 7;
    g.fwd.pad = 3;                                                                       // 2^32 * 49 weights
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.height = 0x7fffffff; g.fwd.width = 1; g.fwd.pad = 0x7fffffff;                  // 2 * pad leaves 32 bits
    EXPECT(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n) != MCGMIL_OK);
    g = base_args();
    g.chunk_pixels = INT64_MAX;                                                          // capped by the granule count
    size_t m = 0;
    EXPECT(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &m) == MCGMIL_OK && m == expected_bytes(g));
    EXPECT(n == 12345);
}

static void errors() {
    size_t n = 0;
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(nullptr, &n), MCGMIL_E_INVALID);
    expect_error(mcgmil_conv2d_wgrad_f32x3(nullptr, nullptr), MCGMIL_E_INVALID);
    mcgmil_conv_grad_args g = base_args();
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, nullptr), MCGMIL_E_INVALID);
    g.fwd.batch = 0; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.in_channels = 48; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.in_channels = 16; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.in_channels = 0; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.out_channels = 96; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.kernel_h = 8; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.kernel_w = 0; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.stride = 3; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.stride = 0; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.pad = 3; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.pad = -1; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.height = 1; g.fwd.width = 1; g.fwd.pad = 0;
    expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.in_ab = static_cast<const float*>(fake(0x50000));
    expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.chunk_pixels = -1; expect_error(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.reserved = 1; expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    // the forward call's w, y, stats, workspace, flags and reserved are ignored, not validated
    g.fwd.flags = 0x7fff; g.fwd.reserved = 9; g.fwd.w = fake(0x3); g.fwd.y = fake(0x5);
    EXPECT(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n) == MCGMIL_OK && n > 0); g = base_args();

    // mcgmil_conv2d_wgrad_f32x3: every pointer / alignment check, then the workspace ones
    g.fwd.x = nullptr; expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dy = nullptr; expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dw = nullptr; expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.fwd.x = fake(0x10004); expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.dy = static_cast<const float*>(fake(0x20008)); expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.dw = static_cast<float*>(fake(0x30004)); expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_WORKSPACE);             // no workspace
    EXPECT(mcgmil_conv_wgrad_workspace_size_f32x3(&g, &n) == MCGMIL_OK);
    g.workspace = fake(0x100000);
    g.workspace_bytes = n - 1;                                                           // one byte short
    expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_WORKSPACE);
    g.workspace = fake(0x100010);                                                        // misaligned
    g.workspace_bytes = n;
    expect_error(mcgmil_conv2d_wgrad_f32x3(&g, nullptr), MCGMIL_E_ALIGN);
}

int main() {
    sizes();
    overflow();
    errors();
    printf("conv_grad_x3_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
