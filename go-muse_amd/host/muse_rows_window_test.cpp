// muse_rows_window_test.cpp -- Muse::RunWindowed of the C++ host mirror (Muse.Run with Results.MaxLag as a lag window: the group's
// winner among every series' best match inside +-MaxLag; muse_batch_run_row_ptrs_windowed).  The program builds its series from
// integer arithmetic alone (muse_window_test.cpp's 32-bit linear congruential generator: the same numbers in any language), runs
// RunWindowed over three label groups of six series and prints what Fetch returns, one line per Score:
//     <case> <id label of the winning series> <lag> <score, %.17g>
// case "win": the three RunWindowed calls; "run": three Run calls on the SAME Muse behind them (Run is what it was).
// tests/test_gpu_window_rows.py rebuilds the series and compares the lines with the CPU oracle's.  Exit code 0 = ran through
// ("rows window ok").  Needs a gfx950 GPU.
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
    const int N = 480, G = 3, K = 6, L = 15;
    std::vector<std::vector<SeriesPtr>> groups((size_t)G);
    for (int i = 0; i < G * K; i++)
        groups[(size_t)(i / K)].push_back(
            NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / K)}})));
    auto ref = NewSeries(series(N, -1), NewLabels({{"id", "ref"}}));
    int failures = 0;
    try {
        auto res = NewResults(L, 12, 0.0, SignFilter_ANY);
        auto m = New(ref, res);
        for (auto &g : groups)
            m->RunWindowed(g);
        print("win", res->Fetch());
        for (auto &g : groups)
            m->Run(g);
        print("run", res->Fetch());
        m->RunWindowed({}); // nothing to compare: nothing happens (muse.go:47-50)
        if (!res->Fetch().first.empty())
            failures++;
        auto wide = NewResults(MUSE_LAG_WINDOW_MAX + 1, 12, 0.0, SignFilter_ANY);
        bool refused = false;
        try {
            New(ref, wide)->RunWindowed(groups[0]);
        } catch (const Error &e) {
            refused = e.status == MUSE_ERR_UNSUPPORTED;
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
    printf("rows window ok\n");
    return 0;
}
