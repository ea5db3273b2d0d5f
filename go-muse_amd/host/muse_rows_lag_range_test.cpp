// muse_rows_lag_range_test.cpp -- Muse::RunInLagRange of the C++ host mirror (Muse.Run inside the lags lagLo .. lagHi: the group's
// winner among every series' best match inside the range; muse_batch_run_row_ptrs_in_lag_range).  The program builds its series from
// integer arithmetic alone (muse_window_test.cpp's 32-bit linear congruential generator: the same numbers in any language), runs
// RunInLagRange over three label groups of six series of 2500 samples -- the lags -15 .. 0 (the window kernels) and -300 .. 20 (the
// panel kernels: three panels) -- and prints what Fetch returns, one line per Score:
//     <case> <id label of the winning series> <lag> <score, %.17g>
// case "narrow" / "wide": the three RunInLagRange calls of a range; "run": three Run calls on the SAME Muse behind them (Run is what
// it was).  tests/test_gpu_rows_lag_range.py rebuilds the series and compares the lines with the CPU oracle's.  It also checks that
// a range without lag 0 is refused.  Exit code 0 = ran through ("rows lag range ok").  Needs a gfx950 GPU.
#include <cstdio>
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

static void print(const char *what, const std::pair<Scores, double> &f)
{
    for (auto &sc : f.first) {
        std::string id;
        sc.Labels->Get("id", &id);
        printf("%s %s %d %.17g\n", what, id.c_str(), sc.Lag, sc.PercentScore);
    }
}

int main()
{
    const int N = 2500, G = 3, K = 6, MAXLAG = 400;
    std::vector<std::vector<SeriesPtr>> groups((size_t)G);
    for (int i = 0; i < G * K; i++)
        groups[(size_t)(i / K)].push_back(
            NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / K)}})));
    auto ref = NewSeries(series(N, -1), NewLabels({{"id", "ref"}}));
    int failures = 0;
    try {
        auto res = NewResults(MAXLAG, 12, 0.0, SignFilter_ANY);
        auto m = New(ref, res);
        for (auto &g : groups)
            m->RunInLagRange(g, -15, 0);
        print("narrow", res->Fetch());
        for (auto &g : groups)
            m->RunInLagRange(g, -300, 20);
        print("wide", res->Fetch());
        for (auto &g : groups)
            m->Run(g);
        print("run", res->Fetch());
        m->RunInLagRange({}, -300, 20); // nothing to compare: nothing happens (muse.go:47-50)
        if (!res->Fetch().first.empty())
            failures++;
        bool refused = false;
        try {
            m->RunInLagRange(groups[0], 1, 7);
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
    printf("rows lag range ok\n");
    return 0;
}
