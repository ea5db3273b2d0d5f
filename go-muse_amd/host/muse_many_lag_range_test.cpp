// muse_many_lag_range_test.cpp -- Batch::RunManyInLagRange of the C++ host mirror (muse_batch_run_many_in_lag_range: several
// references against one Group, every series' best match inside the lags lagLo .. lagHi, one pass over the rows).  The series come
// from the integer generator of muse_window_test.cpp (the same numbers in any language); three references (series -1 .. -3 of it:
// the pulse moved by 0, 45 and 90 samples) are run with RunManyInLagRange(nil) and ({"graph"}) over the lags -15 .. 0 (the direct
// product, the three references' 16 table rows each packed into three accumulator tiles of one launch) and -300 .. 20 (one masked
// pass of the many-references transform kernels), and the program prints what every batch Fetches, one line per Score:
//     <case>[<lo>,<hi>]<reference> <id label of the winning series> <lag> <score, %.17g>
// tests/test_gpu_many_lag_range.py rebuilds the series and compares the lines with the CPU oracle's.  Here every batch must also
// Fetch what its own RunInLagRange Fetches (the same series and lags, scores to 1e-6: the many-references transform kernels'
// arithmetic differs in rounding), batches whose Results differ fall back to one RunInLagRange each, a RunMany behind it is the
// RunMany it was before, and a range without lag 0 is refused.  Exit code 0 = ran through ("many lag-range ok").  Needs a gfx950 GPU.
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

static void print(const char *what, int lo, int hi, int r, const std::pair<Scores, double> &f)
{
    for (auto &sc : f.first) {
        std::string id;
        sc.Labels->Get("id", &id);
        printf("%s[%d,%d]%d %s %d %.17g\n", what, lo, hi, r, id.c_str(), sc.Lag, sc.PercentScore);
    }
}

static int differ(const std::pair<Scores, double> &a, const std::pair<Scores, double> &b, bool bits)
{
    int bad = a.first.size() != b.first.size() || a.first.empty();
    for (size_t i = 0; i < a.first.size() && i < b.first.size(); i++) {
        bad += a.first[i].Lag != b.first[i].Lag || a.first[i].Labels->ID() != b.first[i].Labels->ID();
        if (bits)
            bad += std::memcmp(&a.first[i].PercentScore, &b.first[i].PercentScore, 8) != 0;
        else
            bad += !(std::fabs(a.first[i].PercentScore - b.first[i].PercentScore) <= 1e-6 * std::fabs(b.first[i].PercentScore) + 1e-12);
    }
    return bad;
}

int main()
{
    const int N = 1000, M = 240, MAXLAG = 300, R = 3;
    const int ranges[2][2] = {{-15, 0}, {-300, 20}};
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / 6)}})));
    std::vector<std::shared_ptr<Series>> refs;
    for (int r = 0; r < R; r++)
        refs.push_back(NewSeries(series(N, -1 - r), NewLabels({{"id", "ref" + std::to_string(r)}})));
    int failures = 0;
    try {
        const auto fresh = [&](std::vector<ResultsPtr> &results, int count, int maxlag_step) {
            std::vector<std::shared_ptr<Batch>> bs;
            results.clear();
            for (int r = 0; r < count; r++) {
                results.push_back(NewResults(MAXLAG + maxlag_step * r, 12, 0.0, SignFilter_ANY));
                bs.push_back(NewBatch(refs[(size_t)r], g, results.back(), 4));
            }
            return bs;
        };
        std::vector<ResultsPtr> before_results;
        auto before = fresh(before_results, R, 0);
        Batch::RunMany(before, {});
        std::vector<std::pair<Scores, double>> fb;
        for (int r = 0; r < R; r++)
            fb.push_back(before_results[(size_t)r]->Fetch());

        std::vector<ResultsPtr> results;
        auto many = fresh(results, R, 0);
        for (auto &lr : ranges)
            for (int grouped = 0; grouped < 2; grouped++) {
                const std::vector<std::string> by = grouped ? std::vector<std::string>{"graph"} : std::vector<std::string>{};
                Batch::RunManyInLagRange(many, by, lr[0], lr[1]);
                for (int r = 0; r < R; r++) {
                    const auto fetched = results[(size_t)r]->Fetch(); // (Fetch empties the Results)
                    print(grouped ? "graph" : "nil", lr[0], lr[1], r, fetched);
                    auto res = NewResults(MAXLAG, 12, 0.0, SignFilter_ANY);
                    NewBatch(refs[(size_t)r], g, res, 4)->RunInLagRange(by, lr[0], lr[1]);
                    const int bad = differ(fetched, res->Fetch(), false);
                    if (bad)
                        printf("range %d .. %d case %d reference %d: %d differences\n", lr[0], lr[1], grouped, r, bad);
                    failures += bad;
                }
            }
        Batch::RunMany(many, {}); // the range was an argument: the RunMany of batches that never saw one
        for (int r = 0; r < R; r++)
            failures += differ(results[(size_t)r]->Fetch(), fb[(size_t)r], true);
        // different Results settings: one RunInLagRange per batch
        std::vector<ResultsPtr> odd_results;
        auto odd = fresh(odd_results, 2, 1);
        Batch::RunManyInLagRange(odd, {}, -15, 0);
        for (int r = 0; r < 2; r++) {
            auto res = NewResults(MAXLAG + r, 12, 0.0, SignFilter_ANY);
            NewBatch(refs[(size_t)r], g, res, 4)->RunInLagRange({}, -15, 0);
            failures += differ(odd_results[(size_t)r]->Fetch(), res->Fetch(), true);
        }
        bool refused = false; // a range that excludes lag 0
        try {
            Batch::RunManyInLagRange(many, {}, 1, 7);
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
    printf("many lag-range ok\n");
    return 0;
}
