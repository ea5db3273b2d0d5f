// muse_many_in_window_test.cpp -- Batch::RunManyInWindow of the C++ host mirror (muse_batch_run_many_in_window: several references
// against one Group, Results.MaxLag as a lag window of any width, one masked pass of the many-references transform kernels).  The
// series come from the integer generator of muse_window_test.cpp (the same numbers in any language); three references (series
// -1 .. -3 of it: the pulse moved by 0, 45 and 90 samples) are run with RunManyInWindow(nil) and ({"graph"}) at MaxLag = 100 --
// wider than MUSE_LAG_WINDOW_MAX, where RunManyWindowed refuses -- and the program prints what every batch Fetches, one line per
// Score:
//     <case><reference> <id label of the winning series> <lag> <score, %.17g>
// tests/test_gpu_many_in_window.py rebuilds the series and compares the lines with the CPU oracle's.  Here every batch must also
// Fetch what its own RunInWindow Fetches (the same series and lags, scores to 1e-6: the many-references kernels' arithmetic
// differs in rounding), and batches whose Results differ fall back to one RunInWindow each.  Exit code 0 = ran through
// ("many in-window ok").  Needs a gfx950 GPU.
#include <cmath>
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

// series i: a pulse of 24 samples moved by shift, scaled, plus noise (i < 0: the references, moved by 45 (-i - 1))
static std::vector<double> series(int N, int i)
{
    uint32_t s = 12345u + 977u * (uint32_t)i;
    const int shift = i < 0 ? 45 * (-i - 1) : (i % 3 == 0 ? 0 : (int)(lcg(s) % 241u) - 120);
    const double amp = 1.0 + 2.0 * (unit(s) + 0.5);
    std::vector<double> y((size_t)N);
    for (int t = 0; t < N; t++) {
        const int u = t - shift;
        y[(size_t)t] = (u >= N / 2 - 12 && u < N / 2 + 12 ? amp : 0.0) + 0.5 * unit(s);
    }
    return y;
}

static void print(const char *what, int r, const std::pair<Scores, double> &f)
{
    for (auto &sc : f.first) {
        std::string id;
        sc.Labels->Get("id", &id);
        printf("%s%d %s %d %.17g\n", what, r, id.c_str(), sc.Lag, sc.PercentScore);
    }
}

static int differ(const std::pair<Scores, double> &a, const std::pair<Scores, double> &b)
{
    int bad = a.first.size() != b.first.size() || a.first.empty();
    for (size_t i = 0; i < a.first.size() && i < b.first.size(); i++)
        bad += a.first[i].Lag != b.first[i].Lag || a.first[i].Labels->ID() != b.first[i].Labels->ID() ||
               !(std::fabs(a.first[i].PercentScore - b.first[i].PercentScore) <= 1e-6 * std::fabs(b.first[i].PercentScore) + 1e-12);
    return bad;
}

int main()
{
    const int N = 1000, M = 240, L = 100, R = 3;
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / 6)}})));
    std::vector<std::shared_ptr<Series>> refs;
    for (int r = 0; r < R; r++)
        refs.push_back(NewSeries(series(N, -1 - r), NewLabels({{"id", "ref" + std::to_string(r)}})));
    int failures = 0;
    try {
        for (int grouped = 0; grouped < 2; grouped++) {
            const std::vector<std::string> by = grouped ? std::vector<std::string>{"graph"} : std::vector<std::string>{};
            std::vector<std::shared_ptr<Batch>> many;
            std::vector<ResultsPtr> results;
            for (int r = 0; r < R; r++) {
                results.push_back(NewResults(L, 12, 0.0, SignFilter_ANY));
                many.push_back(NewBatch(refs[(size_t)r], g, results.back(), 4));
            }
            Batch::RunManyInWindow(many, by);
            for (int r = 0; r < R; r++) {
                const auto fetched = results[(size_t)r]->Fetch(); // (Fetch empties the Results)
                print(grouped ? "graph" : "nil", r, fetched);
                auto res = NewResults(L, 12, 0.0, SignFilter_ANY);
                NewBatch(refs[(size_t)r], g, res, 4)->RunInWindow(by);
                const int bad = differ(fetched, res->Fetch());
                if (bad)
                    printf("case %d reference %d: %d differences\n", grouped, r, bad);
                failures += bad;
            }
        }
        // different Results settings: one RunInWindow per batch
        std::vector<std::shared_ptr<Batch>> odd;
        std::vector<ResultsPtr> odd_results;
        for (int r = 0; r < 2; r++) {
            odd_results.push_back(NewResults(L + r, 12, 0.0, SignFilter_ANY));
            odd.push_back(NewBatch(refs[(size_t)r], g, odd_results.back(), 4));
        }
        Batch::RunManyInWindow(odd, {});
        for (int r = 0; r < 2; r++) {
            auto res = NewResults(L + r, 12, 0.0, SignFilter_ANY);
            NewBatch(refs[(size_t)r], g, res, 4)->RunInWindow({});
            failures += differ(odd_results[(size_t)r]->Fetch(), res->Fetch());
        }
        bool refused = false; // RunManyWindowed keeps its cap
        try {
            std::vector<std::shared_ptr<Batch>> wide;
            for (int r = 0; r < 2; r++)
                wide.push_back(NewBatch(refs[(size_t)r], g, NewResults(L, 12, 0.0, SignFilter_ANY), 4));
            Batch::RunManyWindowed(wide, {});
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
    printf("many in-window ok\n");
    return 0;
}
