// muse_lag_profile_test.cpp -- Batch::LagProfile and Batch::LagProfiles of the C++ host mirror (muse_batch_lag_profile: the correlation
// at every lag of lagLo .. lagHi, written out).  The program builds the series of host/muse_lag_band_test.cpp from integer arithmetic
// alone (the same numbers in any language), runs RunInLagBand({"graph"}, 1, 15), and prints the curve behind every Score Fetch returns,
// one line per Score:
//     curve <id label of the series> <lag of the Score> <cc at lags 1 .. 15, %.17g each>
// and the whole-group profile's rows 0, 17 and M - 1 over the lags -3 .. 20:
//     row <index> <cc at lags -3 .. 20, %.17g each>
// tests/test_gpu_lag_profile.py rebuilds the series and compares the lines with its long-double table.  It also checks here that the
// Score's value is the curve's value at the Score's lag bit for bit (where Run has not clamped it), that a listed row is the whole
// group's row bit for bit, that a Run behind the profile calls is the Run it was, and that lags outside the length and labels outside
// the group are refused.  Exit code 0 = ran through ("lag-profile ok").  Needs a gfx950 GPU.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "muse.hpp"

using namespace muse;

static uint32_t lcg(uint32_t &s)
{
    s = s * 1664525u + 1013904223u;
    return s;
}
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) / 16777216.0 - 0.5; } // [-0.5, 0.5), exact

// series i: a pulse of 24 samples moved by shift(i), scaled, plus noise (muse_lag_band_test.cpp's); negated when i % 4 == 1
static std::vector<double> series(int N, int i)
{
    uint32_t s = 12345u + 977u * (uint32_t)i;
    const int shift = i < 0 ? 0 : (i % 3 == 0 ? 0 : (int)(lcg(s) % 241u) - 120);
    const double amp = 1.0 + 2.0 * (unit(s) + 0.5);
    const double sgn = i >= 0 && i % 4 == 1 ? -1.0 : 1.0;
    std::vector<double> y((size_t)N);
    for (int t = 0; t < N; t++) {
        const int u = t - shift;
        y[(size_t)t] = sgn * ((u >= N / 2 - 12 && u < N / 2 + 12 ? amp : 0.0) + 0.5 * unit(s));
    }
    return y;
}

static int differ(const std::pair<Scores, double> &a, const std::pair<Scores, double> &b)
{
    int d = a.first.size() != b.first.size();
    for (size_t i = 0; i < a.first.size() && i < b.first.size(); i++)
        d += a.first[i].Lag != b.first[i].Lag || std::memcmp(&a.first[i].PercentScore, &b.first[i].PercentScore, 8) != 0 ||
             a.first[i].Labels->ID() != b.first[i].Labels->ID();
    return d;
}

template <class F> static bool refuses(int status, F &&f)
{
    try {
        f();
    } catch (const Error &e) {
        return e.status == status;
    }
    return false;
}

int main()
{
    const int N = 1000, M = 240, MAXLAG = 300;
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / 6)}})));
    auto ref = NewSeries(series(N, -1), NewLabels({{"id", "ref"}}));
    int failures = 0;
    try {
        auto before = NewResults(MAXLAG, 12, 0.0, SignFilter_ANY);
        NewBatch(ref, g, before, 4)->Run({});
        const auto fb = before->Fetch();

        auto res = NewResults(MAXLAG, 12, 0.0, SignFilter_ANY);
        auto b = NewBatch(ref, g, res, 4);
        b->RunInLagBand({"graph"}, 1, 15);
        const auto f = res->Fetch();
        const auto curves = b->LagProfiles(1, 15, f.first);
        failures += curves.size() != f.first.size() || f.first.empty();
        for (auto &c : curves) {
            std::string id;
            c.score.Labels->Get("id", &id);
            printf("curve %s %d", id.c_str(), c.score.Lag);
            for (double v : c.cc)
                printf(" %.17g", v);
            printf("\n");
            failures += c.lags.size() != 15 || c.cc.size() != 15 || c.lags.front() != 1 || c.lags.back() != 15;
            // Batch reports magnitudes (muse_batch.go:74), clamped at 1
            if (c.score.Lag >= 1 && c.score.Lag <= 15 && std::fabs(c.score.PercentScore) < 1.0) {
                const double at = std::fabs(c.cc[(size_t)c.score.Lag - 1]);
                failures += std::memcmp(&at, &c.score.PercentScore, 8) != 0;
            }
        }
        const int W = 24;
        const std::vector<double> all = b->LagProfile(-3, 20);
        failures += all.size() != (size_t)M * W;
        const std::vector<int64_t> rows = {0, 17, M - 1, 17};
        const std::vector<double> some = b->LagProfile(-3, 20, rows);
        failures += some.size() != rows.size() * W;
        for (size_t k = 0; k < rows.size() && failures == 0; k++) {
            failures += std::memcmp(&some[k * W], &all[(size_t)rows[k] * W], W * sizeof(double)) != 0;
            if (k == 3)
                break;
            printf("row %lld", (long long)rows[k]);
            for (int v = 0; v < W; v++)
                printf(" %.17g", some[k * W + v]);
            printf("\n");
        }
        failures += !b->LagProfile(1, 15, {}, false).empty(); // a list of no entries: nothing
        b->Run({}); // the Run of a batch that has written profiles is the Run it was
        failures += differ(res->Fetch(), fb);
        // FFT length 1024: lags -511 .. 512, not clipped
        failures += !refuses(MUSE_ERR_INVALID, [&] { b->LagProfile(0, 513); });
        failures += !refuses(MUSE_ERR_INVALID, [&] { b->LagProfile(-512, 0); });
        failures += !refuses(MUSE_ERR_INVALID, [&] { b->LagProfile(7, 1); });
        failures += !refuses(MUSE_ERR_INVALID, [&] { b->LagProfile(1, 15, {M}); });
        failures += !refuses(MUSE_ERR_INVALID, [&] { b->LagProfiles(1, 15, Scores{Score{NewLabels({{"id", "nobody"}}), 1, 0.5}}); });
        failures += b->LagProfile(-511, 512, {3}).size() != 1024;
    } catch (const Error &e) {
        printf("FAIL: %s\n", e.what());
        return 1;
    }
    if (failures) {
        printf("FAIL: %d checks\n", failures);
        return 1;
    }
    printf("lag-profile ok\n");
    return 0;
}
