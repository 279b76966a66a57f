// Host-side sanitizer run of the bf16 stem convolution's C ABI (include/mcgmil_stem_grad_bf16.h).
// Built by tests/asan/build_stem_grad_bf16.sh (from tests/test_stem_grad_bf16_capi_sanitizers.py):
// mcgmil_stem_grad_bf16.hip, mcgmil_stem.hip and the sources they link against with
// -fsanitize=address,undefined on the host pass only (no GPU needed). Every call below returns
// before any launch: argument validation, error codes and messages of the three entries, and the
// workspace-size arithmetic over a sweep of geometries, including sizes that would overflow 32
// bits (and 64). Exits 0 when every expectation holds; the sanitizers abort on the first memory
// or UB error.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "mcgmil_stem_grad_bf16.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void* fake(uintptr_t p) { return reinterpret_cast<void*>(p); }   // never dereferenced on the host

static mcgmil_stem_grad_bf16_args base_args() {
    mcgmil_stem_grad_bf16_args g;
    memset(&g, 0, sizeof g);
    mcgmil_stem_args& a = g.fwd;
    a.batch = 4; a.in_channels = 3; a.height = 224; a.width = 224; a.out_channels = 64;
    a.kernel = 7; a.stride = 2; a.pad = 3;
    a.x = fake(0x10000);
    g.dy = fake(0x20000);
    g.dw = static_cast<float*>(fake(0x30000));
    return g;
}

static void expect_error(int rc, int code) {
    EXPECT(rc == code);
    const char* msg = mcgmil_last_error();
    EXPECT(msg != nullptr && strlen(msg) > 0);
}

// The documented workspace formula, restated: (1 + granules per chunk) * E fp32 words,
// E = 64 * in_channels * kernel * 8.
static unsigned long long expected_bytes(const mcgmil_stem_grad_bf16_args& g) {
    const mcgmil_stem_args& a = g.fwd;
    const long long oh = (a.height + 2LL * a.pad - a.kernel) / 2 + 1;
    const long long ow = (a.width + 2LL * a.pad - a.kernel) / 2 + 1;
    const long long P = a.batch * oh * ow;
    const long long E = 64LL * a.in_channels * a.kernel * 8;
    const long long total = (P + MCGMIL_WGRAD_GRANULE_PIXELS - 1) / MCGMIL_WGRAD_GRANULE_PIXELS;
    long long gc = g.chunk_pixels ? g.chunk_pixels / MCGMIL_WGRAD_GRANULE_PIXELS
                                  : MCGMIL_WGRAD_DEFAULT_PARTIAL_BYTES / (E * 4);
    if (gc < 1) gc = 1;
    if (gc > total) gc = total;
    return (unsigned long long)(gc + 1) * E * 4;
}

static void sizes() {
    for (int batch : {1, 3, 64, 1507})
        for (int h : {2, 7, 96, 224})
            for (int w : {2, 8, 100, 244})
                for (int cin : {1, 2, 3, 4})
                    for (int k : {1, 3, 6, 7, 8})
                        for (int pad : {0, 2, 3, 4})
                            for (long long cap : {0LL, 1LL, 2048LL, 10000LL, 1LL << 40}) {
                                if (k + (pad & 1) > 8 || h + 2 * pad < k || w + 2 * pad < k) continue;
                                if ((w + 2 * pad - k) / 2 + 1 > 125) continue;       // outside the domain
                                mcgmil_stem_grad_bf16_args g = base_args();
                                g.fwd.batch = batch; g.fwd.height = h; g.fwd.width = w;
                                g.fwd.in_channels = cin; g.fwd.kernel = k; g.fwd.pad = pad;
                                g.chunk_pixels = cap;
                                size_t n = 0;
                                const int rc = mcgmil_stem_wgrad_workspace_size_bf16(&g, &n);
                                EXPECT(rc == MCGMIL_OK);
                                if (rc == MCGMIL_OK) {
                                    EXPECT(n == expected_bytes(g));
                                    EXPECT(n % 256 == 0);
                                }
                            }
    EXPECT(mcgmil_stem_grad_bf16_args_size() == sizeof(mcgmil_stem_grad_bf16_args));
    // the stem of a config-5 bag: 2.4 GB of dy, offsets past 32 bits, still supported
    mcgmil_stem_grad_bf16_args g = base_args();
    g.fwd.batch = 1507;
    size_t n = 0;
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) == MCGMIL_OK && n == expected_bytes(g));
    EXPECT(n == (1 + (128ull << 20) / (64 * 168 * 4)) * 64 * 168 * 4);
    // a smaller cap needs a smaller workspace, never a larger one
    size_t small = 0;
    g.chunk_pixels = MCGMIL_WGRAD_GRANULE_PIXELS;
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &small) == MCGMIL_OK && small < n);
    EXPECT(small == 2ull * 64 * 168 * 4);
    g.chunk_pixels = 3 * MCGMIL_WGRAD_GRANULE_PIXELS + 5;
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &small) == MCGMIL_OK && small == 4ull * 64 * 168 * 4);
}

static void overflow() {
    // sizes whose products leave 32 or 64 bits or the supported range: an error, never a wrapped size
    size_t n = 12345;
    mcgmil_stem_grad_bf16_args g = base_args();
    g.fwd.batch = 0x7fffffff; g.fwd.height = 0x7fffffff; g.fwd.width = 244;              // x leaves 64 bits
    expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 1 << 20; g.fwd.height = 64; g.fwd.width = 64;                          // 2^32 input elements
    expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.batch = 7134; g.fwd.in_channels = 3;                                           // x just past 2 GiB
    expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED);
    g.fwd.batch = 7133;                                                                  // ... and just below
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) == MCGMIL_OK && n == expected_bytes(g));
    n = 12345;
    g = base_args();
    g.fwd.height = 0x7fffffff; g.fwd.width = 2; g.fwd.pad = 0x7ffffffe;                  // 2 * pad leaves 32 bits
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) != MCGMIL_OK);
    g = base_args();
    g.fwd.kernel = 0x7fffffff; g.fwd.pad = 1;                                            // kernel + 1 leaves 32 bits
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) != MCGMIL_OK);
    EXPECT(n == 12345);
    g = base_args();
    g.chunk_pixels = INT64_MAX;                                                          // capped by the granule count
    size_t m = 0;
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &m) == MCGMIL_OK && m == expected_bytes(g));
}

static void errors() {
    size_t n = 0;
    expect_error(mcgmil_stem_wgrad_workspace_size_bf16(nullptr, &n), MCGMIL_E_INVALID);
    expect_error(mcgmil_stem_wgrad_bf16(nullptr, nullptr), MCGMIL_E_INVALID);
    mcgmil_stem_grad_bf16_args g = base_args();
    expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, nullptr), MCGMIL_E_INVALID);
    g.fwd.batch = 0; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.height = 0; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.in_channels = 5; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.in_channels = 0; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.out_channels = 128; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.kernel = 9; g.fwd.pad = 4; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.kernel = 8; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();   // odd pad
    g.fwd.kernel = 0; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.stride = 1; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.pad = -1; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.width = 223; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.width = 252; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();  // OW 126
    g.fwd.width = 250; EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) == MCGMIL_OK); g = base_args();                // OW 125
    g.fwd.height = 2; g.fwd.width = 2; g.fwd.pad = 0;
    expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.chunk_pixels = -1; expect_error(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.reserved = 1; expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    // everything of the forward call but its geometry and x is ignored, not validated
    g.fwd.flags = 0x7fff; g.fwd.reserved = 9; g.fwd.w = fake(0x3); g.fwd.y = fake(0x5); g.fwd.pool_kernel = -4;
    g.fwd.relu = 7; g.fwd.gamma = static_cast<const float*>(fake(0x7));
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) == MCGMIL_OK && n > 0); g = base_args();

    // mcgmil_stem_wgrad_bf16: every pointer / alignment check, then the workspace ones
    g.fwd.x = nullptr; expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dy = nullptr; expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dw = nullptr; expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.fwd.x = fake(0x10002); expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.dy = fake(0x20008); expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.dw = static_cast<float*>(fake(0x30004)); expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.fwd.x = fake(0x10004);                                                             // 4-byte aligned x is enough
    expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_WORKSPACE); g = base_args();   // no workspace
    EXPECT(mcgmil_stem_wgrad_workspace_size_bf16(&g, &n) == MCGMIL_OK);
    g.workspace = fake(0x100000);
    g.workspace_bytes = n - 1;                                                           // one byte short
    expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_WORKSPACE);
    g.workspace = fake(0x100010);                                                        // misaligned
    g.workspace_bytes = n;
    expect_error(mcgmil_stem_wgrad_bf16(&g, nullptr), MCGMIL_E_ALIGN);
}

static void forward_errors() {
    // mcgmil_stem_conv_bf16: mcgmil_stem_forward's domain without pooling and without a BatchNorm
    expect_error(mcgmil_stem_conv_bf16(nullptr, nullptr), MCGMIL_E_INVALID);
    mcgmil_stem_args a = base_args().fwd;
    a.w = fake(0x40000); a.y = fake(0x50000);
    const mcgmil_stem_args ok = a;
    a.in_channels = 5; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = ok;
    a.out_channels = 128; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = ok;
    a.stride = 1; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = ok;
    a.width = 223; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = ok;
    a.width = 252; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = ok;
    a.batch = 7134; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = ok;
    a.batch = 0; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.relu = 2; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.flags = 7; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.reserved = 1; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.pool_kernel = 3; a.pool_stride = 2; a.pool_pad = 1;
    expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.pool_kernel = -1; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    const float* p = static_cast<const float*>(fake(0x60000));
    a.gamma = p; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.beta = p; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.running_mean = p; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.running_var = p; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.batch_mean = static_cast<float*>(fake(0x60000)); expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.batch_invstd = static_cast<float*>(fake(0x60000)); expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.x = nullptr; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.w = nullptr; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.y = nullptr; expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_INVALID); a = ok;
    a.x = fake(0x10002); expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = ok;
    a.w = fake(0x40008); expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = ok;
    a.y = fake(0x50008); expect_error(mcgmil_stem_conv_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = ok;
}

int main() {
    sizes();
    overflow();
    errors();
    forward_errors();
    printf("stem_grad_bf16_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
