// muse_many_lag_band_test.cpp -- Batch::RunManyInLagBand and Batch::RunManySignedInLagBand of the C++ host mirror
// (muse_batch_run_many_in_lag_band: several references against one Group, every series' best match inside a lag band that need not
// hold lag 0, by magnitude or under a sign, one pass over the rows).  The series come from the integer generator of
// muse_many_lag_range_test.cpp (the same numbers in any language; three references: the pulse moved by 0, 45 and 90 samples).  They
// are run with RunManyInLagBand(nil) and ({"graph"}) under SignFilter_ANY and with RunManySignedInLagBand under SignFilter_POS and
// SignFilter_NEG over the lags 1 .. 15 (the direct product, the three references' 15 table rows each packed into the accumulator
// tiles of one launch) and -300 .. -20 (one masked pass of the many-references transform kernel), and the program prints what every
// batch Fetches, one line per Score:
//     <case><0, + or ->[<lo>,<hi>]<reference> <id label of the winning series> <lag> <score, %.17g>
// tests/test_gpu_many_lag_band.py rebuilds the series and compares the lines with the CPU oracle's.  Here every batch must also Fetch
// what its own RunInLagBand / RunSignedInLagBand Fetches (the same series and lags, scores to 1e-6: the many-references transform
// kernels' arithmetic differs in rounding), batches whose Results differ fall back to one single call each, a RunMany behind it is
// the RunMany it was before, and lagLo > lagHi and an empty band are refused.  Exit code 0 = ran through ("many lag-band ok").
// Needs a gfx950 GPU.
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

static void print(const char *what, char sign, int lo, int hi, int r, const std::pair<Scores, double> &f)
{
    for (auto &sc : f.first) {
        std::string id;
        sc.Labels->Get("id", &id);
        printf("%s%c[%d,%d]%d %s %d %.17g\n", what, sign, lo, hi, r, id.c_str(), sc.Lag, sc.PercentScore);
    }
}

static int differ(const std::pair<Scores, double> &a, const std::pair<Scores, double> &b, bool bits)
{
    int bad = a.first.size() != b.first.size();
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
    const int bands[2][2] = {{1, 15}, {-300, -20}};
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / 6)}})));
    std::vector<std::shared_ptr<Series>> refs;
    for (int r = 0; r < R; r++)
        refs.push_back(NewSeries(series(N, -1 - r), NewLabels({{"id", "ref" + std::to_string(r)}})));
    int failures = 0;
    try {
        const auto fresh = [&](std::vector<ResultsPtr> &results, int count, int maxlag_step, SignFilter filter) {
            std::vector<std::shared_ptr<Batch>> bs;
            results.clear();
            for (int r = 0; r < count; r++) {
                results.push_back(NewResults(MAXLAG + maxlag_step * r, 12, 0.0, filter));
                bs.push_back(NewBatch(refs[(size_t)r], g, results.back(), 4));
            }
            return bs;
        };
        std::vector<ResultsPtr> before_results;
        auto before = fresh(before_results, R, 0, SignFilter_ANY);
        Batch::RunMany(before, {});
        std::vector<std::pair<Scores, double>> fb;
        for (int r = 0; r < R; r++)
            fb.push_back(before_results[(size_t)r]->Fetch());

        for (const SignFilter filter : {SignFilter_ANY, SignFilter_POS, SignFilter_NEG}) {
            const char sign = filter == SignFilter_ANY ? '0' : filter == SignFilter_POS ? '+' : '-';
            std::vector<ResultsPtr> results;
            auto many = fresh(results, R, 0, filter);
            for (auto &lr : bands)
                for (int grouped = 0; grouped < 2; grouped++) {
                    const std::vector<std::string> by = grouped ? std::vector<std::string>{"graph"} : std::vector<std::string>{};
                    if (filter == SignFilter_ANY)
                        Batch::RunManyInLagBand(many, by, lr[0], lr[1]);
                    else
                        Batch::RunManySignedInLagBand(many, by, lr[0], lr[1]);
                    for (int r = 0; r < R; r++) {
                        const auto fetched = results[(size_t)r]->Fetch(); // (Fetch empties the Results)
                        print(grouped ? "graph" : "nil", sign, lr[0], lr[1], r, fetched);
                        auto res = NewResults(MAXLAG, 12, 0.0, filter);
                        auto single = NewBatch(refs[(size_t)r], g, res, 4);
                        if (filter == SignFilter_ANY)
                            single->RunInLagBand(by, lr[0], lr[1]);
                        else
                            single->RunSignedInLagBand(by, lr[0], lr[1]);
                        const int bad = differ(fetched, res->Fetch(), false);
                        if (bad)
                            printf("band %d .. %d sign %c case %d reference %d: %d differences\n", lr[0], lr[1], sign, grouped, r, bad);
                        failures += bad;
                    }
                }
            if (filter == SignFilter_ANY) {
                Batch::RunMany(many, {}); // the band was an argument: the RunMany of batches that never saw one
                for (int r = 0; r < R; r++)
                    failures += differ(results[(size_t)r]->Fetch(), fb[(size_t)r], true);
            }
            // different Results settings: one single call per batch
            std::vector<ResultsPtr> odd_results;
            auto odd = fresh(odd_results, 2, 1, filter);
            if (filter == SignFilter_ANY)
                Batch::RunManyInLagBand(odd, {}, 1, 15);
            else
                Batch::RunManySignedInLagBand(odd, {}, 1, 15);
            for (int r = 0; r < 2; r++) {
                auto res = NewResults(MAXLAG + r, 12, 0.0, filter);
                auto single = NewBatch(refs[(size_t)r], g, res, 4);
                if (filter == SignFilter_ANY)
                    single->RunInLagBand({}, 1, 15);
                else
                    single->RunSignedInLagBand({}, 1, 15);
                failures += differ(odd_results[(size_t)r]->Fetch(), res->Fetch(), true);
            }
            for (auto &lr : {std::pair<int, int>{7, 1}, std::pair<int, int>{600, 700}}) { // lagLo > lagHi; nothing left at FFT length 1024
                bool refused = false;
                try {
                    Batch::RunManyInLagBand(many, {}, lr.first, lr.second);
                } catch (const Error &e) {
                    refused = e.status == MUSE_ERR_INVALID;
                }
                if (!refused)
                    failures++;
            }
        }
    } catch (const Error &e) {
        printf("FAIL: %s\n", e.what());
        return 1;
    }
    if (failures) {
        printf("FAIL: %d checks\n", failures);
        return 1;
    }
    printf("many lag-band ok\n");
    return 0;
}
