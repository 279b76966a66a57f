// Host-side sanitizer run of the C ABI of the bf16 stem BatchNorm / ReLU / max-pool training op
// (include/mcgmil_pool_grad_bf16.h). Built by tests/asan/build_pool_grad_bf16.sh (from
// tests/test_pool_grad_bf16_capi_sanitizers.py): mcgmil_pool_grad_bf16.hip and the sources it links
// against with -fsanitize=address,undefined on the host pass only (no GPU needed). Every call
// below returns before any launch: argument validation, error codes and messages of the three
// entry points, and the workspace-size arithmetic over a sweep of shapes, including
// batch x H x W x C past 2^32 elements and past the supported range -- the fp32 entry points'
// domain, validation order and formula, with 2-byte elements in the overlap checks. Exits 0 when
// every expectation holds; the sanitizers abort on the first memory or UB error.
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "mcgmil_pool_grad_bf16.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static float* fake(uintptr_t p) { return reinterpret_cast<float*>(p); }   // never dereferenced on the host
static uint8_t* fake8(uintptr_t p) { return reinterpret_cast<uint8_t*>(p); }

// 3 x 9 x 7 x 64 under the stem's 3 / 2 / 1 pool: z is 24,192 bytes in bf16, dy 7,680, the codes 3,840
static mcgmil_bn_pool_grad_bf16_args base_args() {
    mcgmil_bn_pool_grad_bf16_args a;
    memset(&a, 0, sizeof a);
    a.batch = 3; a.height = 9; a.width = 7; a.channels = 64;
    a.pool_kernel = 3; a.pool_stride = 2; a.pool_pad = 1;
    a.pooled_height = 5; a.pooled_width = 4;
    a.z = fake(0x100000); a.argmax = fake8(0x200000); a.dy = fake(0x300000);
    a.gamma = fake(0x400000); a.mean = fake(0x410000); a.invstd = fake(0x420000);
    a.dz = fake(0x500000); a.dgamma = fake(0x700000); a.dbeta = fake(0x710000);
    a.workspace = fake(0x1000000);
    a.workspace_bytes = 1 << 20;
    return a;
}

static void expect_error(int rc, int code) {
    EXPECT(rc == code);
    const char* msg = mcgmil_last_error();
    EXPECT(msg != nullptr && strlen(msg) > 0);
}

static int pooled(int size, int k, int st, int pd) { return (int)(((long long)size + 2 * pd - k) / st + 1); }

// The documented workspace formula, restated: (4 C + 2 C parts) fp32 words, rounded up to 256 bytes.
static unsigned long long expected_bytes(long long rows, long long C) {
    const long long rpp = MCGMIL_BN_POOL_GRAD_PART_ELEMS / C;
    const long long parts = (rows + rpp - 1) / rpp;
    const unsigned long long raw = (unsigned long long)(4 * C + 2 * C * parts) * 4ull;
    return (raw + 255ull) & ~255ull;
}

static mcgmil_bn_pool_grad_bf16_args shaped(int N, int H, int W, int C, int k = 3, int st = 2, int pd = 1) {
    mcgmil_bn_pool_grad_bf16_args a;
    memset(&a, 0, sizeof a);                                // only the integer fields are read for the size
    a.batch = N; a.height = H; a.width = W; a.channels = C;
    a.pool_kernel = k; a.pool_stride = st; a.pool_pad = pd;
    a.pooled_height = pooled(H, k, st, pd); a.pooled_width = pooled(W, k, st, pd);
    return a;
}

static void sizes() {
    const int shapes[][3] = {{1, 2, 1}, {1, 2, 2}, {3, 9, 7}, {1, 23, 23}, {2, 16, 16}, {64, 112, 112},
                             {1507, 112, 112}, {1338, 112, 112}, {33, 512, 512}, {4096, 1024, 1024}};
    for (const auto& s : shapes)
        for (int C : {8, 24, 64, 512, 1000, 2048}) {
            const long long rows = (long long)s[0] * s[1] * s[2];
            mcgmil_bn_pool_grad_bf16_args a = shaped(s[0], s[1], s[2], C);
            size_t n = 0;
            const int rc = mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n);
            EXPECT(rc == MCGMIL_OK);
            if (rc == MCGMIL_OK) {
                EXPECT(n == expected_bytes(rows, C));
                EXPECT(n % 256 == 0 && n >= (size_t)(6 * C * 4));
            }
            // the same bytes as the fp32 entry point's: the partials and coefficients are fp32 here too
            mcgmil_bn_pool_grad_args f;
            memset(&f, 0, sizeof f);
            f.batch = a.batch; f.height = a.height; f.width = a.width; f.channels = a.channels;
            f.pool_kernel = a.pool_kernel; f.pool_stride = a.pool_stride; f.pool_pad = a.pool_pad;
            f.pooled_height = a.pooled_height; f.pooled_width = a.pooled_width;
            size_t nf = 0;
            EXPECT(mcgmil_bn_pool_grad_workspace_size(&f, &nf) == rc && nf == n);
        }
    EXPECT(mcgmil_bn_pool_grad_bf16_args_size() == sizeof(mcgmil_bn_pool_grad_bf16_args));
    EXPECT(sizeof(mcgmil_bn_pool_grad_bf16_args) == sizeof(mcgmil_bn_pool_grad_args));
    EXPECT(mcgmil_bn_pool_grad_args_size() == sizeof(mcgmil_bn_pool_grad_args));
    // 4096 x 1024 x 1024 x 64 = 2^38 elements: batch * H * W * C far past 2^32, supported
    mcgmil_bn_pool_grad_bf16_args a = shaped(4096, 1024, 1024, 64);
    size_t n = 0;
    EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK);
    EXPECT(n == (4ull * 64 + 2ull * 64 * (1ull << 23)) * 4ull);
    // 1338 x 64 x 112 x 112: just past 2^31 bytes of bf16
    a = shaped(1338, 112, 112, 64);
    EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == expected_bytes(1338LL * 112 * 112, 64));
    // one block per MCGMIL_BN_POOL_GRAD_PART_ELEMS / C pixels, whatever the device
    a = shaped(1, 256, 2, 64, 2, 2, 0);
    EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == (4 * 64 + 2 * 64 * 1) * 4);
    a = shaped(1, 513, 2, 64, 2, 2, 0);
    EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == (4 * 64 + 2 * 64 * 3) * 4);
    // every supported geometry, and the pooled dims it implies
    for (int k : {2, 3})
        for (int st = 1; st <= k; ++st)
            for (int pd = 0; 2 * pd <= k; ++pd) {
                a = shaped(2, 9, 7, 16, k, st, pd);
                EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == expected_bytes(2 * 9 * 7, 16));
                a.pooled_height += 1;
                expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID);
            }
}

static void overflow() {
    // shapes whose products leave the supported range: an error, never a wrapped size
    size_t n = 12345;
    mcgmil_bn_pool_grad_bf16_args a = shaped(INT32_MAX, INT32_MAX, 1, 2048);      // H * W < 2^31, rows * C past 2^46
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    a = shaped(INT32_MAX, 46341, 46341, 2048);                                    // H * W >= 2^31
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    a = shaped(INT32_MAX, INT32_MAX, INT32_MAX, 8);
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    a = shaped(1 << 13, 1 << 15, 1 << 15, 8);                                     // exactly 2^46 elements
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_UNSUPPORTED);
    EXPECT(n == 12345);
    a = shaped((1 << 13) - 1, 1 << 15, 1 << 15, 8);                               // just below
    EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK &&
           n == expected_bytes(((1LL << 13) - 1) << 30, 8));
    a = shaped(1, INT32_MAX, 1, 8);                                               // H + 2 pad passes 2^31: 64-bit
    EXPECT(a.pooled_height == (1 << 30) && mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK &&
           n == expected_bytes(INT32_MAX, 8));
    a = shaped(INT32_MIN, 9, 7, 64);
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID);
    a = shaped(3, -9, 7, 64);
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), MCGMIL_E_INVALID);
}

static void backward_errors() {
    size_t n = 0;
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(nullptr, &n), MCGMIL_E_INVALID);
    expect_error(mcgmil_batchnorm_pool_backward_bf16(nullptr, nullptr), MCGMIL_E_INVALID);
    mcgmil_bn_pool_grad_bf16_args a = base_args();
    expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, nullptr), MCGMIL_E_INVALID);
    EXPECT(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n) == MCGMIL_OK && n == expected_bytes(189, 64));
#define BAD(set, code)                                                             \
    do {                                                                           \
        a = base_args();                                                           \
        set;                                                                       \
        expect_error(mcgmil_batchnorm_pool_backward_bf16(&a, nullptr), code);      \
    } while (0)
#define BAD_SIZE(set, code)                                                        \
    do {                                                                           \
        BAD(set, code);                                                            \
        expect_error(mcgmil_bn_pool_grad_workspace_size_bf16(&a, &n), code);       \
    } while (0)
    // the plan: the integer fields, for the size and the backward alike
    BAD_SIZE(a.reserved = 1, MCGMIL_E_INVALID);
    BAD_SIZE(a.reserved32 = 1, MCGMIL_E_INVALID);
    BAD_SIZE(a.channels = 12, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.channels = 0, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.channels = -8, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.channels = 2056, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.batch = 0, MCGMIL_E_INVALID);
    BAD_SIZE(a.height = 0, MCGMIL_E_INVALID);
    BAD_SIZE((a.batch = 1, a.height = 1, a.width = 1, a.pooled_height = 1, a.pooled_width = 1), MCGMIL_E_INVALID);  // rows < 2
    BAD_SIZE(a.pool_kernel = 4, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.pool_kernel = 1, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.pool_pad = 2, MCGMIL_E_UNSUPPORTED);                                   // pad > k / 2
    BAD_SIZE(a.pool_pad = -1, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.pool_stride = 4, MCGMIL_E_UNSUPPORTED);                                // stride > k
    BAD_SIZE(a.pool_stride = 0, MCGMIL_E_UNSUPPORTED);
    BAD_SIZE(a.pooled_height = 4, MCGMIL_E_INVALID);                                  // not this pool's dy
    BAD_SIZE(a.pooled_width = 5, MCGMIL_E_INVALID);
    BAD_SIZE((a.height = 1, a.width = 1, a.pool_stride = 1, a.pool_pad = 0), MCGMIL_E_INVALID);   // window larger than the input
    // every pointer check ...
    BAD(a.z = nullptr, MCGMIL_E_INVALID);
    BAD(a.argmax = nullptr, MCGMIL_E_INVALID);
    BAD(a.dy = nullptr, MCGMIL_E_INVALID);
    BAD(a.mean = nullptr, MCGMIL_E_INVALID);
    BAD(a.invstd = nullptr, MCGMIL_E_INVALID);
    BAD((a.dz = nullptr, a.dgamma = a.dbeta = nullptr), MCGMIL_E_INVALID);           // nothing to compute
    // ... every alignment check ...
    BAD(a.z = fake(0x100002), MCGMIL_E_ALIGN);
    BAD(a.dy = fake(0x300008), MCGMIL_E_ALIGN);
    BAD(a.dz = fake(0x500004), MCGMIL_E_ALIGN);
    BAD(a.mean = fake(0x410004), MCGMIL_E_ALIGN);
    BAD(a.invstd = fake(0x420008), MCGMIL_E_ALIGN);
    BAD(a.argmax = fake8(0x200004), MCGMIL_E_ALIGN);
    BAD(a.gamma = fake(0x400002), MCGMIL_E_ALIGN);
    BAD(a.dgamma = fake(0x700001), MCGMIL_E_ALIGN);
    BAD(a.dbeta = fake(0x710003), MCGMIL_E_ALIGN);
    // ... the overlaps, with 2-byte elements: z and dz are 3 * 9 * 7 * 64 * 2 = 24,192 bytes, dy
    // 3 * 5 * 4 * 64 * 2 = 7,680 and the codes 3,840
    BAD(a.dz = const_cast<void*>(a.z), MCGMIL_E_INVALID);
    BAD(a.dz = fake(0x100000 + 24192 - 16), MCGMIL_E_INVALID);                        // the last 16 bytes of z
    BAD(a.dz = fake(0x100000 - 24192 + 16), MCGMIL_E_INVALID);                        // dz's last 16 bytes on z's first
    BAD(a.dz = fake(0x300000 + 7680 - 16), MCGMIL_E_INVALID);                         // the tail of dy
    BAD(a.dz = fake(0x200000 + 3840 - 16), MCGMIL_E_INVALID);                         // the tail of the codes
    BAD(a.dgamma = const_cast<float*>(a.mean), MCGMIL_E_INVALID);
    BAD(a.dbeta = const_cast<float*>(a.gamma), MCGMIL_E_INVALID);
    BAD(a.dbeta = a.dgamma, MCGMIL_E_INVALID);                                        // the outputs overlap each other
    BAD(a.dgamma = fake(0x500000 + 24192 - 16), MCGMIL_E_INVALID);                    // dgamma in dz's tail
    // what would overlap with 4-byte elements but does not with 2-byte ones passes these checks and
    // stops at the workspace: dz right behind z's 24,192 bytes, dz right behind dy's 7,680
    BAD((a.dz = fake(0x100000 + 24192), a.workspace = nullptr), MCGMIL_E_WORKSPACE);
    BAD((a.dz = fake(0x300000 + 7680), a.workspace = nullptr), MCGMIL_E_WORKSPACE);
    BAD((a.z = fake(0x500000 + 24192), a.workspace = nullptr), MCGMIL_E_WORKSPACE);
    // ... then the workspace ones
    BAD(a.workspace = nullptr, MCGMIL_E_WORKSPACE);
    BAD(a.workspace_bytes = expected_bytes(189, 64) - 1, MCGMIL_E_WORKSPACE);            // one byte short
    BAD(a.workspace_bytes = 0, MCGMIL_E_WORKSPACE);
    BAD((a.workspace = fake(0x1000010), a.workspace_bytes = expected_bytes(189, 64)), MCGMIL_E_ALIGN);
    // the order: alignment before the overlaps, the overlaps before the workspace
    BAD((a.z = fake(0x100002), a.dz = fake(0x100002)), MCGMIL_E_ALIGN);
    BAD((a.dz = const_cast<void*>(a.z), a.workspace = nullptr), MCGMIL_E_INVALID);
#undef BAD_SIZE
#undef BAD
}

static mcgmil_bn_args forward_args() {
    mcgmil_bn_args a;
    memset(&a, 0, sizeof a);
    a.rows = 189; a.channels = 64; a.dtype = MCGMIL_BF16;
    a.batch = 3; a.height = 9; a.width = 7;
    a.pool_kernel = 3; a.pool_stride = 2; a.pool_pad = 1;
    a.x = fake(0x100000); a.y = fake(0x300000);
    a.gamma = fake(0x400000); a.beta = fake(0x401000);
    a.eps = 1e-5; a.relu = 1;
    a.batch_mean = fake(0x410000); a.batch_invstd = fake(0x420000);
    a.workspace = fake(0x1000000);
    a.workspace_bytes = 0;          // too small on purpose: a complete call would launch
    return a;
}

static void forward_errors() {
    uint8_t* const codes = fake8(0x200000);
    expect_error(mcgmil_batchnorm_pool_train_bf16(nullptr, codes, nullptr), MCGMIL_E_INVALID);
    mcgmil_bn_args a = forward_args();
#define BADF(set, cd, code)                                                        \
    do {                                                                           \
        a = forward_args();                                                        \
        set;                                                                       \
        expect_error(mcgmil_batchnorm_pool_train_bf16(&a, cd, nullptr), code);     \
    } while (0)
    BADF(a.dtype = MCGMIL_F32, codes, MCGMIL_E_UNSUPPORTED);                          // the fp32 entry point's
    BADF(a.dtype = 7, codes, MCGMIL_E_UNSUPPORTED);
    BADF(a.channels = 12, codes, MCGMIL_E_UNSUPPORTED);
    BADF(a.channels = 2056, codes, MCGMIL_E_UNSUPPORTED);
    BADF(a.pool_kernel = 4, codes, MCGMIL_E_UNSUPPORTED);
    BADF(a.pool_kernel = 0, codes, MCGMIL_E_UNSUPPORTED);                             // no pool: mcgmil_batchnorm_act's job
    BADF(a.pool_pad = 2, codes, MCGMIL_E_UNSUPPORTED);
    BADF(a.pool_stride = 4, codes, MCGMIL_E_UNSUPPORTED);
    BADF((a.rows = 1, a.batch = 1, a.height = 1, a.width = 1), codes, MCGMIL_E_INVALID);
    BADF(a.rows = 190, codes, MCGMIL_E_INVALID);                                      // batch * height * width != rows
    BADF(a.batch = 0, codes, MCGMIL_E_INVALID);
    BADF((a.rows = (1LL << 43), a.batch = 1 << 13, a.height = 1 << 15, a.width = 1 << 15, a.channels = 8), codes,
         MCGMIL_E_UNSUPPORTED);                                                       // 2^46 elements
    BADF((a.running_mean = fake(0x430000), a.running_var = fake(0x431000)), codes, MCGMIL_E_INVALID);
    BADF((a.partials = fake(0x440000), a.num_partials = 1), codes, MCGMIL_E_INVALID);
    BADF(a.residual = fake(0x600000), codes, MCGMIL_E_UNSUPPORTED);
    BADF(a.relu = 2, codes, MCGMIL_E_INVALID);
    BADF(a.x = nullptr, codes, MCGMIL_E_INVALID);
    BADF(a.y = nullptr, codes, MCGMIL_E_INVALID);
    BADF(a.batch_mean = nullptr, codes, MCGMIL_E_INVALID);
    BADF(a.batch_invstd = nullptr, codes, MCGMIL_E_INVALID);
    BADF((void)0, nullptr, MCGMIL_E_INVALID);                                         // no argmax
    BADF(a.x = fake(0x100002), codes, MCGMIL_E_ALIGN);
    BADF(a.y = fake(0x300008), codes, MCGMIL_E_ALIGN);
    BADF((void)0, fake8(0x200004), MCGMIL_E_ALIGN);
    BADF((a.height = 1, a.width = 1, a.batch = 189, a.pool_stride = 1, a.pool_pad = 0), codes, MCGMIL_E_INVALID);   // window larger than the input
    // overlaps with 2-byte elements: x is 24,192 bytes, y 7,680, the codes 3,840
    BADF(a.y = fake(0x100000 + 24192 - 16), codes, MCGMIL_E_INVALID);
    BADF((void)0, fake8(0x100000 + 24192 - 8), MCGMIL_E_INVALID);
    BADF((void)0, fake8(0x300000 + 7680 - 8), MCGMIL_E_INVALID);
    BADF(a.y = fake(0x100000 + 24192), codes, MCGMIL_E_WORKSPACE);                    // right behind x: no overlap
    BADF((void)0, fake8(0x300000 + 7680), MCGMIL_E_WORKSPACE);                        // right behind y
    // the workspace last: missing, then (through the statistics' validation) too small
    BADF(a.workspace = nullptr, codes, MCGMIL_E_WORKSPACE);
    BADF((void)0, codes, MCGMIL_E_WORKSPACE);
    BADF((a.workspace = fake(0x1000010), a.workspace_bytes = 1 << 20), codes, MCGMIL_E_WORKSPACE);   // misaligned
#undef BADF
    // mcgmil_batchnorm_pool_train keeps refusing bf16
    a = forward_args();
    expect_error(mcgmil_batchnorm_pool_train(&a, codes, nullptr), MCGMIL_E_UNSUPPORTED);
}

int main() {
    sizes();
    overflow();
    backward_errors();
    forward_errors();
    printf("pool_grad_bf16_host_check: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
