// Host-side sanitizer run of the backward pass's C ABI (include/mcgmil_grad.h). Built by
// tests/asan/build_grad.sh (from tests/test_grad_capi_sanitizers.py): mcgmil_grad.hip and the
// sources it links against with -fsanitize=address,undefined on the host pass only (no GPU
// needed). Every call below returns before any launch: argument validation, error codes and
// messages, and the workspace-size arithmetic over a sweep of shapes, including sizes that would
// overflow. Exits 0 when every expectation holds; the sanitizers abort on the first memory or UB
// error.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mcgmil_grad.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void* fake(uintptr_t p) { return reinterpret_cast<void*>(p); }   // never dereferenced on the host

static mcgmil_grad_args base_args() {
    mcgmil_grad_args g;
    memset(&g, 0, sizeof g);
    mcgmil_args& a = g.fwd;
    a.L = 512; a.D = 128; a.C = 2; a.G = 2; a.T = 2; a.num_bags = 1; a.total_rows = 1100;
    a.h_dtype = MCGMIL_F32;
    a.ldh = 512;
    a.H = fake(0x10000);
    a.bag_offsets = static_cast<const int32_t*>(fake(0x1000));
    a.Wv = a.Wu = a.bv = a.bu = a.wa = a.ba = a.wk = static_cast<const float*>(fake(0x20000));
    a.p_feat = a.p_att = 0.1f;
    g.A = g.Y = g.dY = static_cast<const float*>(fake(0x30000));
    g.dH = static_cast<float*>(fake(0x40000));
    g.ldh_grad = 512;
    return g;
}

static void expect_error(int rc, int code) {
    EXPECT(rc == code);
    const char* msg = mcgmil_last_error();
    EXPECT(msg != nullptr && strlen(msg) > 0);
}

static size_t block(size_t words) { return (words * 4 + 255) / 256 * 256; }

// The documented workspace formula, restated.
static size_t expected_bytes(const mcgmil_grad_args& g) {
    const mcgmil_args& a = g.fwd;
    const size_t K2 = 2 * (size_t)a.G * a.D, Kw = K2 + 16, NPA = (size_t)a.C * a.D + K2 + a.C, L = a.L;
    const size_t lds32 = (32 * L + 32 * (K2 + 4) + 12 * 32 + ((NPA + 3) & ~(size_t)3)) * 4 + 32 * 6 * 4 + 32 * (L / 8);
    const size_t BM = lds32 <= 160 * 1024 ? 32 : 16;
    const long long cap = g.chunk_pairs ? g.chunk_pairs : MCGMIL_GRAD_DEFAULT_CHUNK_PAIRS;
    const long long gran_total = (a.total_rows + MCGMIL_GRAD_GRANULE_ROWS - 1) / MCGMIL_GRAD_GRANULE_ROWS;
    long long gc = cap / ((long long)a.T * MCGMIL_GRAD_GRANULE_ROWS);
    if (gc < 1) gc = 1;
    if (gc > gran_total) gc = gran_total;
    const size_t Rc = (size_t)gc * MCGMIL_GRAD_GRANULE_ROWS;
    return block(L * K2) + block(Rc * 2) + block(Rc * a.T * Kw) + block(Rc / BM * NPA) + block((size_t)gc * Kw * L) +
           block(NPA) + block(Kw * L) + block((size_t)a.num_bags * a.T * a.C);
}

static void sizes() {
    for (int L : {32, 512, 1024})
        for (int D : {16, 64, 128})
            for (int C = 1; C <= 4; ++C)
                for (int G : {1, C})
                    for (int T : {1, 3, 100})
                        for (long long rows : {0LL, 1LL, 37LL, 1100LL, 24112LL, 1LL << 20})
                            for (long long cap : {0LL, 1LL, 1024LL, 1LL << 40}) {
                                mcgmil_grad_args g = base_args();
                                g.fwd.L = L; g.fwd.ldh = L; g.fwd.D = D; g.fwd.C = C; g.fwd.G = G; g.fwd.T = T;
                                g.fwd.total_rows = rows;
                                g.chunk_pairs = cap;
                                size_t n = 0;
                                const int rc = mcgmil_grad_workspace_size(&g, &n);
                                if (rc == MCGMIL_OK)
                                    EXPECT(n == expected_bytes(g));
                                else
                                    EXPECT(rc == MCGMIL_E_UNSUPPORTED);    // only "too large"
                                if (rows <= 24112 && cap <= 1024) EXPECT(rc == MCGMIL_OK);
                            }
    EXPECT(mcgmil_grad_args_size() == sizeof(mcgmil_grad_args));
}

static void overflow() {
    // sizes whose products leave 64 bits or the supported range: an error, never a wrapped size
    size_t n = 12345;
    mcgmil_grad_args g = base_args();
    g.fwd.T = 32768; g.fwd.total_rows = 0x7fffffffLL; g.chunk_pairs = INT64_MAX;
    expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.D = 1 << 30; g.fwd.G = 1; g.fwd.C = 1;
    EXPECT(mcgmil_grad_workspace_size(&g, &n) != MCGMIL_OK);
    g = base_args();
    g.fwd.D = 1 << 20; g.fwd.G = 4; g.fwd.C = 4;            // G * D beyond the supported range
    expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.L = 2048; g.fwd.ldh = 2048; g.fwd.D = 2048; g.fwd.G = 4; g.fwd.C = 4;   // row tile beyond the LDS
    expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED);
    g = base_args();
    g.fwd.total_rows = 0x7fffffffLL; g.fwd.T = 1; g.chunk_pairs = INT64_MAX;    // one chunk of 2^31 rows
    expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED);
    EXPECT(n == 12345);
}

static void errors() {
    size_t n = 0;
    expect_error(mcgmil_grad_workspace_size(nullptr, &n), MCGMIL_E_INVALID);
    expect_error(mcgmil_head_backward(nullptr, nullptr), MCGMIL_E_INVALID);
    mcgmil_grad_args g = base_args();
    expect_error(mcgmil_grad_workspace_size(&g, nullptr), MCGMIL_E_INVALID);
    g.fwd.T = 0; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.L = 100; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.C = 5; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.G = 3; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.p_att = -0.5f; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.bag_offsets = nullptr; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.fwd.h_dtype = MCGMIL_BF16; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_UNSUPPORTED);
    expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.fwd.keep_feat = static_cast<const uint8_t*>(fake(0x50000));
    g.fwd.keep_att = static_cast<const uint8_t*>(fake(0x60000));
    expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_UNSUPPORTED); g = base_args();
    g.chunk_pairs = -1; expect_error(mcgmil_grad_workspace_size(&g, &n), MCGMIL_E_INVALID); g = base_args();
    g.reserved = 1; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    // the forward call's flags / debug / reserved are ignored, not validated
    g.fwd.flags = 0x7fff; g.fwd.reserved = 9;
    EXPECT(mcgmil_grad_workspace_size(&g, &n) == MCGMIL_OK && n > 0); g = base_args();

    // mcgmil_head_backward: every pointer / stride / alignment check, then the workspace ones
    g.fwd.H = nullptr; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.fwd.wa = nullptr; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.fwd.Wv = nullptr; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.A = nullptr; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.Y = nullptr; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.dY = nullptr; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.fwd.ldh = 256; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.ldh_grad = 100; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_INVALID); g = base_args();
    g.fwd.H = fake(0x10004); expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.fwd.ldh = 514; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.fwd.wk = static_cast<const float*>(fake(0x20008)); expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.dH = static_cast<float*>(fake(0x40004)); expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    g.ldh_grad = 513; expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_ALIGN); g = base_args();
    expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_WORKSPACE);            // no workspace
    EXPECT(mcgmil_grad_workspace_size(&g, &n) == MCGMIL_OK);
    std::vector<unsigned char> ws(4096);
    g.workspace = ws.data();
    g.workspace_bytes = n - 1;                                                      // one byte short
    expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_WORKSPACE);
    g.workspace = fake(0x100010);                                                   // misaligned
    g.workspace_bytes = n;
    expect_error(mcgmil_head_backward(&g, nullptr), MCGMIL_E_ALIGN);
    // a smaller cap needs a smaller workspace, never a larger one
    size_t small = 0;
    g.chunk_pairs = 1024;
    EXPECT(mcgmil_grad_workspace_size(&g, &small) == MCGMIL_OK && small < n);
}

int main() {
    sizes();
    overflow();
    errors();
    printf("grad_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
