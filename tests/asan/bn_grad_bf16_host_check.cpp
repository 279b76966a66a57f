// Host-side sanitizer run of the bf16 fused BatchNorm backward's C ABI
// (include/mcgmil_bn_grad_bf16.h). Built by tests/asan/build_bn_grad_bf16.sh (from
// tests/test_bn_grad_bf16_capi_sanitizers.py): mcgmil_bn_grad_bf16.hip and the sources it links
// against with -fsanitize=address,undefined on the host pass only (no GPU needed). Every call
// below returns before any launch: argument validation, error codes and messages, and the
// workspace-size arithmetic over a sweep of shapes, including rows x C past 2^32 elements and
// past the supported range -- the fp32 entry points' domain, validation order and formula. Exits 0
// when every expectation holds; the sanitizers abort on the first memory or UB error.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "mcgmil_bn_grad_bf16.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static float* fake(uintptr_t p) { return reinterpret_cast<float*>(p); }   // never dereferenced on the host

static mcgmil_bn_grad_bf16_args base_args() {
    mcgmil_bn_grad_bf16_args a;
    memset(&a, 0, sizeof a);
    a.rows = 189; a.channels = 64; a.relu = 1;
    a.x = fake(0x10000); a.y = fake(0x20000); a.dy = fake(0x30000);
    a.gamma = fake(0x40000); a.mean = fake(0x41000); a.invstd = fake(0x42000);
    a.dx = fake(0x50000); a.dresidual = fake(0x60000); a.dgamma = fake(0x70000); a.dbeta = fake(0x71000);
    a.workspace = fake(0x100000);
    a.workspace_bytes = 1 << 20;
    return a;
}

static void expect_error(int rc, int code) {
    EXPECT(rc == code);
    const char* msg = mcgmil_last_error();
    EXPECT(msg != nullptr && strlen(msg) > 0);
}

// The documented workspace formula, restated: (4 C + 2 C parts) fp32 words, rounded up to 256 bytes.
static unsigned long long expected_bytes(long long rows, long long C) {
    const long long rpp = MCGMIL_BN_GRAD_PART_ELEMS / C;
    const long long parts = (rows + rpp - 1) / rpp;
    const unsigned long long raw = (unsigned long long)(4 * C + 2 * C * parts) * 4ull;
    return (raw + 255ull) & ~255ull;
}

static void sizes() {
    for (long long rows : {2LL, 3LL, 189LL, 512LL, 513LL, 5125LL, 1507LL * 56 * 56, 33LL * 512 * 512, 1LL << 33})
        for (int C : {8, 24, 64, 512, 1000, 2048}) {
            mcgmil_bn_grad_bf16_args a = base_args();
            a.rows = rows; a.channels = C;
            size_t n = 0;
            const int rc = mcgmil_bn_grad_workspace_size_bf16(&a, &n);
            EXPECT(rc == MCGMIL_OK);
            if (rc == MCGMIL_OK) {
                EXPECT(n == expected_bytes(rows, C));
                EXPECT(n % 256 == 0 && n >= (size_t)(6 * C * 4));
            }
        }
    EXPECT(mcgmil_bn_grad_bf16_args_size() == sizeof(mcgmil_bn_grad_bf16_args));
    // only rows, channels and reserved are read: no pointer is needed for the size
    mcgmil_bn_grad_bf16_args a;
    memset(&a, 0, sizeof a);
    a.rows = 1LL << 26; a.channels = 64;                    // 2^32 elements: offsets past 32 bits, supported
    size_t n = 0;
    EXPECT(mcgmil_bn_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == expected_bytes(1LL << 26, 64));
    EXPECT(n == (4ull * 64 + 2ull * 64 * (1ull << 17)) * 4ull);
    // one block per MCGMIL_BN_GRAD_PART_ELEMS / C rows, whatever the device
    // the same bytes as the fp32 entry point's: the partials and coefficients are fp32 here too
    mcgmil_bn_grad_args f;
    memset(&f, 0, sizeof f);
    f.rows = a.rows; f.channels = a.channels;
    size_t nf = 0;
    EXPECT(mcgmil_bn_grad_workspace_size(&f, &nf) == MCGMIL_OK && nf == n);
    EXPECT(sizeof(mcgmil_bn_grad_bf16_args) == sizeof(mcgmil_bn_grad_args));
    a.rows = 512; EXPECT(mcgmil_bn_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == (4 * 64 + 2 * 64 * 1) * 4);
    a.rows = 513; EXPECT(mcgmil_bn_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == (4 * 64 + 2 * 64 * 2) * 4);
}

static void overflow() {
    // shapes whose products leave the supported range or 64 bits: an error, never a wrapped size
    size_t n = 12345;
    mcgmil_bn_grad_bf16_args a = base_args();
    a.rows = INT64_MAX; a.channels = 2048;                                  // rows * C leaves 64 bits
    expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    a.rows = INT64_MAX / 8; a.channels = 8;                                 // fits 64 bits, past 2^46
    expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    a.rows = 1LL << 43; a.channels = 8;                                     // exactly 2^46 elements
    expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    EXPECT(n == 12345);
    a.rows = (1LL << 43) - 1; a.channels = 8;                               // the largest supported
    EXPECT(mcgmil_bn_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == expected_bytes((1LL << 43) - 1, 8));
    a.rows = INT64_MIN; a.channels = 64;
    expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID);
}

static void errors() {
    size_t n = 0;
    expect_error(mcgmil_bn_grad_workspace_size_bf16(nullptr, &n), MCGMIL_E_INVALID);
    expect_error(mcgmil_batchnorm_act_backward_bf16(nullptr, nullptr), MCGMIL_E_INVALID);
    mcgmil_bn_grad_bf16_args a = base_args();
    expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, nullptr), MCGMIL_E_INVALID);
    a.channels = 12; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED); a = base_args();
    a.channels = 0; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED); a = base_args();
    a.channels = -8; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED); a = base_args();
    a.channels = 2056; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED); a = base_args();
    a.channels = 2056; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_UNSUPPORTED); a = base_args();
    a.rows = 1; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID); a = base_args();
    a.rows = 1; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.rows = 0; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID); a = base_args();
    a.reserved = 1; expect_error(mcgmil_bn_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID); a = base_args();
    a.reserved = -1; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();

    // mcgmil_batchnorm_act_backward_bf16: every pointer check ...
    a.relu = 2; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.x = nullptr; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.dy = nullptr; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.mean = nullptr; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.invstd = nullptr; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.y = nullptr; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();   // relu needs y
    a.dx = a.dresidual = a.dgamma = a.dbeta = nullptr;                                                             // nothing to compute
    expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    a.relu = 0; a.y = nullptr;                                                                                      // dresidual needs relu
    expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_INVALID); a = base_args();
    // ... every alignment check ...
    a.x = fake(0x10004); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.y = fake(0x20008); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.dy = fake(0x3000c); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.dx = fake(0x50004); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.dresidual = fake(0x60008); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.mean = fake(0x41004); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.invstd = fake(0x42008); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.gamma = fake(0x40002); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.dgamma = fake(0x70001); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    a.dbeta = fake(0x71003); expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN); a = base_args();
    // ... then the workspace ones
    a.workspace = nullptr; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_WORKSPACE); a = base_args();
    EXPECT(mcgmil_bn_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == expected_bytes(189, 64));
    a.workspace_bytes = n - 1;                                                            // one byte short
    expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_WORKSPACE);
    a.workspace_bytes = 0; expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_WORKSPACE);
    a.workspace = fake(0x100010);                                                         // misaligned
    a.workspace_bytes = n;
    expect_error(mcgmil_batchnorm_act_backward_bf16(&a, nullptr), MCGMIL_E_ALIGN);
}

int main() {
    sizes();
    overflow();
    errors();
    printf("bn_grad_bf16_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
