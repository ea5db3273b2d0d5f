// many_lag_bands_plan_sweep.cpp -- the planner and the argument checks of muse_batch_score_many_in_lag_bands under the host
// sanitizers: a stand-alone program over the test ABI (muse_test_many_lag_bands_plan; pure host code, no device), to be linked against
// a build of the library whose HOST code is compiled with -fsanitize=address,undefined:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -Xarch_host -fsanitize=address,undefined -Iinclude -Igo-muse_amd/csrc \
//         go-muse_amd/csrc/*.hip tools/many_lag_bands_plan_sweep.cpp -o many_lag_bands_plan_sweep && ./many_lag_bands_plan_sweep
// Sweeps R = 1 .. 17 over random lists of table rows (bands and ranges anywhere inside +-300, every sign), re-derives the invariants
// of every plan (tiles, rows, image placement, LDS) and walks the refusals.  Prints "plan sweep ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "muse_hip.h"
#include "muse_hip_test.h"

static unsigned long long state = 88172645463325252ULL;
static unsigned rnd(unsigned k)
{
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return (unsigned)(state % k);
}

#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) {                                                                 \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);                    \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

static int place(const std::vector<int> &w, int kc, std::vector<int> *at)
{
    int a = 0;
    for (int x : w) {
        if (at)
            at->push_back(a);
        int step = kc + x - 1;
        while (step % 32 != (x + 2) % 32)
            step++;
        a += step;
    }
    return a;
}

int main()
{
    long long plans = 0, packed = 0;
    for (int R = 1; R <= 17; R++) {
        for (int trial = 0; trial < 400; trial++) {
            const int tops[4] = {3, 17, 48, 140};
            const int top = tops[trial % 4];
            // exactly R entries per array: an access behind them is the sanitizer's to report
            std::vector<int32_t> lo((size_t)R), hi((size_t)R), sign((size_t)R), path((size_t)R), of((size_t)R), tiles((size_t)R), kc((size_t)R),
                img0((size_t)R);
            std::vector<int> W((size_t)R);
            for (int r = 0; r < R; r++) {
                W[(size_t)r] = 1 + (int)rnd((unsigned)top);
                lo[(size_t)r] = -300 + (int32_t)rnd((unsigned)(601 - W[(size_t)r]));
                hi[(size_t)r] = lo[(size_t)r] + W[(size_t)r] - 1;
                sign[(size_t)r] = (int32_t)rnd(3) - 1;
            }
            int32_t launches = -1;
            REQUIRE(muse_test_many_lag_bands_plan(1000, 0, R, lo.data(), hi.data(), trial % 5 ? sign.data() : nullptr, path.data(), of.data(),
                                                  &launches, tiles.data(), kc.data(), img0.data()) == MUSE_OK);
            REQUIRE(launches >= 0 && launches <= R);
            plans++;
            for (int l = 0; l < launches; l++) {
                std::vector<int> w, at;
                int rows = 0;
                for (int r = 0; r < R; r++)
                    if (of[(size_t)r] == l) {
                        w.push_back(W[(size_t)r]);
                        rows += W[(size_t)r];
                    }
                REQUIRE(!w.empty() && rows <= 128 && tiles[(size_t)l] == (rows + 15) / 16 && tiles[(size_t)l] >= 1 && tiles[(size_t)l] <= 8);
                if (w.size() == 1) {
                    REQUIRE(kc[(size_t)l] == 1024);
                    continue;
                }
                packed++;
                const int end = place(w, kc[(size_t)l], &at);
                REQUIRE(end <= 4608 && (kc[(size_t)l] == 256 || kc[(size_t)l] == 512 || kc[(size_t)l] == 1024));
                size_t k = 0;
                for (int r = 0; r < R; r++)
                    if (of[(size_t)r] == l) {
                        REQUIRE(W[(size_t)r] <= 48 && img0[(size_t)r] == at[k]);
                        k++;
                    }
                const int parts = 16 / (int)w.size() > 1 ? 16 / (int)w.size() : 1;
                const int buf = end > tiles[(size_t)l] * 256 ? end : tiles[(size_t)l] * 256;
                REQUIRE(8 * (buf + 128 + (int)w.size() * parts * 48) <= 64 * 1024);
            }
            for (int r = 0; r < R; r++)
                REQUIRE((W[(size_t)r] <= 127) == (of[(size_t)r] >= 0) && (of[(size_t)r] < 0 || path[(size_t)r] == MUSE_IN_WINDOW_MFMA));
            // the refusals, one index at a time
            const int bad = (int)rnd((unsigned)R);
            std::vector<int32_t> x = lo;
            x[(size_t)bad] = hi[(size_t)bad] + 1;
            REQUIRE(muse_test_many_lag_bands_plan(1000, 0, R, x.data(), hi.data(), sign.data(), path.data(), of.data(), &launches, tiles.data(),
                                                  kc.data(), img0.data()) == MUSE_ERR_INVALID);
            x = sign;
            x[(size_t)bad] = 2;
            REQUIRE(muse_test_many_lag_bands_plan(1000, 0, R, lo.data(), hi.data(), x.data(), path.data(), of.data(), &launches, tiles.data(),
                                                  kc.data(), img0.data()) == MUSE_ERR_INVALID);
            x = lo;
            std::vector<int32_t> y = hi;
            x[(size_t)bad] = 600;
            y[(size_t)bad] = 700; // nothing of it is left at FFT length 1024
            REQUIRE(muse_test_many_lag_bands_plan(1000, 0, R, x.data(), y.data(), sign.data(), path.data(), of.data(), &launches, tiles.data(),
                                                  kc.data(), img0.data()) == MUSE_ERR_INVALID);
        }
    }
    int32_t one = 0, n = 0;
    REQUIRE(muse_test_many_lag_bands_plan(1000, 0, 1, nullptr, &one, nullptr, &one, &one, &n, &one, &one, &one) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_many_lag_bands_plan(1000, 0, 0, &one, &one, nullptr, &one, &one, &n, &one, &one, &one) == MUSE_ERR_INVALID);
    REQUIRE(muse_test_many_lag_bands_plan(1, 0, 1, &one, &one, nullptr, &one, &one, &n, &one, &one, &one) == MUSE_ERR_INVALID);
    // the entry points' own argument checks need no device either: they refuse before they reach one
    REQUIRE(muse_batch_score_many_in_lag_bands(nullptr, 2, &one, &one, nullptr) == MUSE_ERR_INVALID);
    REQUIRE(muse_batch_run_many_in_lag_bands(nullptr, 0, nullptr, 0, &one, &one, &one, nullptr, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr,
                                             nullptr) == MUSE_ERR_INVALID);
    REQUIRE(plans == 17 * 400 && packed > 2000);
    std::printf("plan sweep ok: %lld plans, %lld packed launches\n", plans, packed);
    return 0;
}
