// muse_in_window_test.cpp -- Batch::RunInWindow of the C++ host mirror (muse_batch_run_in_window: Results.MaxLag as a lag window of
// any width).  The program builds its series from integer arithmetic alone (host/muse_window_test.cpp's generator: the same numbers
// in any language), runs RunInWindow(nil) and RunInWindow({"graph"}) with MaxLag = 100 -- wider than MUSE_LAG_WINDOW_MAX, where
// RunWindowed refuses -- and prints what Fetch returns, one line per Score:
//     <case> <id label of the winning series> <lag> <score, %.17g>
// tests/test_gpu_in_window.py rebuilds the series and compares the lines with the CPU oracle's.  It also checks here that a Run
// behind a RunInWindow is the Run it was before.  Exit code 0 = ran through ("in-window ok").  Needs a gfx950 GPU.
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
static std::vector<double> series(int N, int i, int *shift_out)
{
    uint32_t s = 12345u + 977u * (uint32_t)i;
    const int shift = i < 0 ? 0 : (i % 3 == 0 ? 0 : (int)(lcg(s) % 241u) - 120);
    const double amp = 1.0 + 2.0 * (unit(s) + 0.5);
    std::vector<double> y((size_t)N);
    for (int t = 0; t < N; t++) {
        const int u = t - shift;
        y[(size_t)t] = (u >= N / 2 - 12 && u < N / 2 + 12 ? amp : 0.0) + 0.5 * unit(s);
    }
    if (shift_out)
        *shift_out = shift;
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
    const int N = 1000, M = 240, L = 100;
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(series(N, i, nullptr), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / 6)}})));
    auto ref = NewSeries(series(N, -1, nullptr), NewLabels({{"id", "ref"}}));
    int failures = 0;
    try {
        auto before = NewResults(L, 12, 0.0, SignFilter_ANY);
        NewBatch(ref, g, before, 4)->Run({});
        const auto fb = before->Fetch();

        auto res = NewResults(L, 12, 0.0, SignFilter_ANY);
        auto b = NewBatch(ref, g, res, 4);
        b->RunInWindow({});
        print("nil", res->Fetch());
        b->RunInWindow({"graph"});
        print("graph", res->Fetch());
        b->Run({}); // the window was an argument: the Run of a batch that never saw one
        const auto fa = res->Fetch();
        if (fa.first.size() != fb.first.size())
            failures++;
        for (size_t i = 0; i < fa.first.size() && i < fb.first.size(); i++)
            if (fa.first[i].Lag != fb.first[i].Lag || std::memcmp(&fa.first[i].PercentScore, &fb.first[i].PercentScore, 8) != 0 ||
                fa.first[i].Labels->ID() != fb.first[i].Labels->ID())
                failures++;
        bool refused = false; // RunWindowed keeps its cap
        try {
            b->RunWindowed({});
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
    printf("in-window ok\n");
    return 0;
}
