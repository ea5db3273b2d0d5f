// lag_profile_plan_sweep.cpp -- the planner and the argument checks of muse_batch_lag_profile under the host sanitizers: a stand-alone
// program over the test ABI (muse_test_lag_profile_plan; pure host code, no device), to be linked against a build of the library whose
// HOST code is compiled with -fsanitize=address,undefined:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined -Iinclude -Igo-muse_amd/csrc \
//         go-muse_amd/csrc/*.hip tools/lag_profile_plan_sweep.cpp -o lag_profile_plan_sweep && ./lag_profile_plan_sweep
// Sweeps every (N, lag_lo, lag_hi) of a small grid -- N over lengths at, below and above powers of two, every pair of lags from two
// below the lowest lag of the FFT length to two above the highest -- re-derives every plan (consecutive launches of up to 127 rows
// that cover the lags exactly) and every refusal, hands the planner arrays of exactly the entries it may fill, and walks the entry
// points' own refusals.  Prints "plan sweep ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "muse_hip.h"
#include "muse_hip_test.h"

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);                    \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

int main()
{
    long long plans = 0, refused = 0, multi = 0;
    const int lengths[] = {2, 3, 16, 63, 64, 65, 100, 255, 256, 257, 480, 512};
    for (const int N : lengths) {
        int n = 1;
        while (n < N)
            n *= 2;
        const int lo_min = -(n / 2 - 1), hi_max = n / 2;
        for (int lo = lo_min - 2; lo <= hi_max + 2; lo++)
            for (int hi = lo - 1; hi <= hi_max + 2; hi++) {
                int32_t launches = -7;
                const bool ok = lo <= hi && lo >= lo_min && hi <= hi_max;
                const int W = hi - lo + 1;
                const int want = ok ? (W + 126) / 127 : 0;
                // exactly `want` entries per array: an access behind them is the sanitizer's to report
                std::vector<int32_t> lo_of((size_t)want), rows_of((size_t)want);
                const int rc = muse_test_lag_profile_plan(N, lo, hi, &launches, lo_of.data(), rows_of.data(), want);
                if (!ok) {
                    REQUIRE(rc == MUSE_ERR_INVALID && launches == -7);
                    refused++;
                    continue;
                }
                REQUIRE(rc == MUSE_OK && launches == want);
                int next = lo;
                for (int j = 0; j < want; j++) {
                    REQUIRE(lo_of[(size_t)j] == next && rows_of[(size_t)j] >= 1 && rows_of[(size_t)j] <= 127);
                    REQUIRE(j == want - 1 || rows_of[(size_t)j] == 127);
                    next += rows_of[(size_t)j];
                }
                REQUIRE(next == hi + 1);
                plans++;
                multi += want > 1;
                if (want > 1 && (lo + hi) % 7 == 0) { // a shorter array: the count is whole, nothing behind cap is written
                    std::vector<int32_t> a(1), b(1);
                    REQUIRE(muse_test_lag_profile_plan(N, lo, hi, &launches, a.data(), b.data(), 1) == MUSE_OK && launches == want);
                    REQUIRE(a[0] == lo && b[0] == 127);
                    REQUIRE(muse_test_lag_profile_plan(N, lo, hi, &launches, nullptr, nullptr, 0) == MUSE_OK && launches == want);
                }
            }
    }
    int32_t one = 0, n = 0;
    REQUIRE(muse_test_lag_profile_plan(1, 0, 0, &n, &one, &one, 1) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_lag_profile_plan(480, 0, 3, nullptr, &one, &one, 1) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_lag_profile_plan(480, 0, 3, &n, nullptr, &one, 1) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_lag_profile_plan(480, 0, 3, &n, &one, &one, -1) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_lag_profile_plan(480, INT32_MIN, INT32_MAX, &n, &one, &one, 1) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_lag_profile_plan(480, INT32_MAX, INT32_MIN, &n, &one, &one, 1) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_lag_profile_plan(65537, -7, 7, &n, &one, &one, 1) == MUSE_ERR_UNSUPPORTED);
    REQUIRE(muse_test_lag_profile_plan(65536, -32767, 32768, &n, nullptr, nullptr, 0) == MUSE_OK && n == 517);
    // the entry points' own argument checks need no device either: they refuse before they reach one
    double out = 0.0;
    int64_t idx = 0;
    REQUIRE(muse_batch_lag_profile(nullptr, nullptr, 0, -7, 7, &out, 15) == MUSE_ERR_INVALID);
    REQUIRE(muse_batch_lag_profile(nullptr, &idx, 1, -7, 7, &out, 15) == MUSE_ERR_INVALID);
    REQUIRE(muse_batch_lag_profile_device(nullptr, nullptr, 0, -7, 7, &out, 15) == MUSE_ERR_INVALID);
    REQUIRE(out == 0.0);
    REQUIRE(plans > 100000 && refused > 1000 && multi > 10000);
    std::printf("plan sweep ok: %lld plans (%lld of several launches), %lld refusals\n", plans, multi, refused);
    return 0;
}
