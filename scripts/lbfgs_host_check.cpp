// lbfgs_host_check.cpp -- the host-side pieces of csrc/lbfgs_common.h that need
// no device, as a stand-alone program for a sanitizer build: the state
// registry (insert, replace, lookup across the two engines), the tensor table
// builder's range checks and check_shape.  No HIP call is made.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -I include -I sgc_amd/csrc scripts/lbfgs_host_check.cpp -o /tmp/lbfgs_host_check
//   /tmp/lbfgs_host_check        (prints "lbfgs_host_check: ok")
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "lbfgs_common.h"

namespace sgc {
static thread_local char g_error[512];
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace sgc

using namespace sgc;

static std::atomic<int> failures{0};
#define EXPECT(cond)                                                            \
    do {                                                                        \
        if (!(cond)) {                                                          \
            ++failures;                                                         \
            fprintf(stderr, "line %d: %s   [%s]\n", __LINE__, #cond, g_error);  \
        }                                                                       \
    } while (0)

static bool says(const char *text) { return strstr(g_error, text) != nullptr; }

template <typename Off> static void table_checks(const Engine &E, int64_t too_many) {
    Tensors<Off> T;
    int64_t n = 0;
    float a[4], b[4];
    float *const params[3] = {a, b, nullptr};
    const float *const grads[3] = {nullptr, b, nullptr};
    const int64_t numels[3] = {3, 4, 0};
    EXPECT(build_table("t", E, 3, params, grads, numels, T, n) == SGC_OK && n == 7);
    EXPECT(T.count == 3 && T.off[0] == 0 && T.off[1] == 3 && T.off[2] == 7 && T.off[3] == 7 &&
           T.off[kMaxTensors] == 7);
    EXPECT(T.p[0] == a && T.p[1] == b && T.g[0] == nullptr && T.g[1] == b && T.p[3] == nullptr &&
           T.g[kMaxTensors - 1] == nullptr);
    const int64_t neg[2] = {4, -1};
    EXPECT(build_table("t", E, 2, params, grads, neg, T, n) == SGC_EINVAL && says("numels[1]=-1"));
    const int64_t zero[2] = {0, 0};
    EXPECT(build_table("t", E, 2, params, grads, zero, T, n) == SGC_EINVAL && says("n=0 < 1"));
    const int64_t big[2] = {too_many - 1, 1};
    EXPECT(build_table("t", E, 2, params, grads, big, T, n) == SGC_ERANGE && says(E.limit));
    const int64_t most[2] = {too_many - 2, 1};
    EXPECT(build_table("t", E, 2, params, grads, most, T, n) == SGC_OK && n == too_many - 1 &&
           (int64_t)T.off[1] == too_many - 2 && (int64_t)T.off[2] == n);
    // a full table: 16 tensors
    float *p16[kMaxTensors];
    const float *g16[kMaxTensors];
    int64_t k16[kMaxTensors];
    for (int i = 0; i < kMaxTensors; ++i) p16[i] = a, g16[i] = b, k16[i] = i + 1;
    EXPECT(build_table("t", E, kMaxTensors, p16, g16, k16, T, n) == SGC_OK && n == 136 &&
           T.off[kMaxTensors] == 136 && T.off[kMaxTensors - 1] == 120);
}

int main() {
    // check_shape: each engine's limit and wording
    EXPECT(check_shape("w", 65536, 1024, kNarrowEngine) == SGC_OK);
    EXPECT(check_shape("w", 65537, 10, kNarrowEngine) == SGC_ERANGE && says("n=65537 > 65536"));
    EXPECT(check_shape("w", 0, 10, kNarrowEngine) == SGC_EINVAL && says("n=0 < 1"));
    EXPECT(check_shape("w", 10, 0, kWideEngine) == SGC_EINVAL && says("history_size=0 < 1"));
    EXPECT(check_shape("w", 10, 1025, kWideEngine) == SGC_ERANGE && says("1025 > 1024"));
    EXPECT(check_shape("w", INT32_MAX - 1, 1, kWideEngine) == SGC_OK);
    EXPECT(check_shape("w", INT32_MAX, 1, kWideEngine) == SGC_ERANGE && says(">= 2^31 - 1"));

    table_checks<int32_t>(kNarrowEngine, 65537);
    table_checks<int64_t>(kWideEngine, INT32_MAX);

    // the registry: insert, lookup by kind, replacement by either init
    char s1[1], s2[1];
    StateShape sh;
    EXPECT(find_state("f", s1, kNarrowEngine, sh) == SGC_EINVAL &&
           says("f: state not initialised by sgc_lbfgs_init"));
    record_state(s1, 40, 3, kNarrowEngine);
    EXPECT(find_state("f", s1, kNarrowEngine, sh) == SGC_OK && sh.n == 40 && sh.m == 3 && !sh.wide);
    EXPECT(find_state("f", s1, kWideEngine, sh) == SGC_EINVAL &&
           says("not initialised by sgc_lbfgs_wide_init"));
    record_state(s1, 41, 2, kWideEngine);  // the other init on the same address replaces it
    EXPECT(find_state("f", s1, kWideEngine, sh) == SGC_OK && sh.n == 41 && sh.m == 2 && sh.wide);
    EXPECT(find_state("f", s1, kNarrowEngine, sh) == SGC_EINVAL &&
           says("not initialised by sgc_lbfgs_init"));
    EXPECT(find_state("f", s2, kWideEngine, sh) == SGC_EINVAL);
    record_state(s1, 40, 3, kNarrowEngine);
    EXPECT(find_state("f", s1, kNarrowEngine, sh) == SGC_OK && sh.n == 40);
    EXPECT(find_state("f", s1, kWideEngine, sh) == SGC_EINVAL);

    // concurrent inits and lookups on distinct addresses
    std::vector<char> pool(64);
    std::vector<std::thread> threads;
    for (int t = 0; t < 8; ++t)
        threads.emplace_back([&pool, t] {
            StateShape mine;
            for (int i = 0; i < 200; ++i) {
                const void *key = &pool[8 * t + i % 8];
                const Engine &E = i % 2 ? kWideEngine : kNarrowEngine;
                record_state(key, i + 1, 1, E);
                if (find_state("f", key, E, mine) != SGC_OK || mine.n != i + 1) ++failures;
            }
        });
    for (auto &th : threads) th.join();

    if (failures) {
        fprintf(stderr, "lbfgs_host_check: %d failure(s)\n", failures.load());
        return 1;
    }
    puts("lbfgs_host_check: ok");
    return 0;
}
