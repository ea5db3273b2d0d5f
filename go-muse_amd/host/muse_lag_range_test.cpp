// muse_lag_range_test.cpp -- Batch::RunInLagRange of the C++ host mirror (muse_batch_run_in_lag_range: a one-sided or asymmetric
// lag window).  The program builds its series from integer arithmetic alone (host/muse_window_test.cpp's generator: the same numbers
// in any language), runs RunInLagRange(nil) and RunInLagRange({"graph"}) over the lags -15 .. 0 (the direct product: one accumulator
// tile) and -100 .. 300 (the transform kernels with a masked argmax) and prints what Fetch returns, one line per Score:
//     <case> <id label of the winning series> <lag> <score, %.17g>
// tests/test_gpu_lag_range.py rebuilds the series and compares the lines with the CPU oracle's.  It also checks here that a Run
// behind a RunInLagRange is the Run it was before and that a range without lag 0 is refused.  Exit code 0 = ran through
// ("lag-range ok").  Needs a gfx950 GPU.
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

// series i: a pulse of 24 samples moved by shift(i), scaled, plus noise
static std::vector<double> series(int N, int i)
{
    uint32_t s = 12345u + 977u * (uint32_t)i;
    const int shift = i < 0 ? 0 : (i % 3 == 0 ? 0 : (int)(lcg(s) % 241u) - 120);
    const double amp = 1.0 + 2.0 * (unit(s) + 0.5);
    std::vector<double> y((size_t)N);
    for (int t = 0; t < N; t++) {
        const int u = t - shift;
        y[(size_t)t] = (u >= N / 2 - 12 && u < N / 2 + 12 ? amp : 0.0) + 0.5 * unit(s);
    }
    return y;
}

static void print(const char *what, int lo, int hi, const std::pair<Scores, double> &f)
{
    for (auto &sc : f.first) {
        std::string id;
        sc.Labels->Get("id", &id);
        printf("%s[%d,%d] %s %d %.17g\n", what, lo, hi, id.c_str(), sc.Lag, sc.PercentScore);
    }
}

int main()
{
    const int N = 1000, M = 240, MAXLAG = 300;
    const int ranges[2][2] = {{-15, 0}, {-100, 300}};
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
        for (auto &r : ranges) {
            b->RunInLagRange({}, r[0], r[1]);
            print("nil", r[0], r[1], res->Fetch());
            b->RunInLagRange({"graph"}, r[0], r[1]);
            print("graph", r[0], r[1], res->Fetch());
        }
        b->Run({}); // the range was an argument: the Run of a batch that never saw one
        const auto fa = res->Fetch();
        if (fa.first.size() != fb.first.size())
            failures++;
        for (size_t i = 0; i < fa.first.size() && i < fb.first.size(); i++)
            if (fa.first[i].Lag != fb.first[i].Lag || std::memcmp(&fa.first[i].PercentScore, &fb.first[i].PercentScore, 8) != 0 ||
                fa.first[i].Labels->ID() != fb.first[i].Labels->ID())
                failures++;
        bool refused = false; // a range that excludes lag 0
        try {
            b->RunInLagRange({}, 1, 7);
        } catch (const Error &e) {
            refused = e.status == MUSE_ERR_INVALID;
        }
        if (!refused)
            failures++;
    } catch (const Error &e) {
        printf("FAIL: %s\n", e.what());
        return 1;
    }
    if (failures) {
        printf("FAIL: %d checks\n", failures);
        return 1;
    }
    printf("lag-range ok\n");
    return 0;
}
