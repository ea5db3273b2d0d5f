// muse_lag_band_test.cpp -- Batch::RunInLagBand and Batch::RunSignedInLagBand of the C++ host mirror (muse_batch_run_in_lag_band: the
// best match inside lags lagLo .. lagHi that need not hold lag 0).  The program builds the series of host/muse_signed_lag_range_test.cpp
// from integer arithmetic alone (the same numbers in any language; every series i with i % 4 == 1 negated, so that both signs have
// strong matches); it runs RunInLagBand(nil) and ({"graph"}) under SignFilter_ANY, and RunSignedInLagBand under SignFilter_POS and
// SignFilter_NEG, over the lags 1 .. 15 (the direct product over the band's own rows) and -300 .. -20 (the transform kernels masked
// to the one index interval), and prints what Fetch returns, one line per Score:
//     <case><0, + or -> [lo,hi] <id label of the winning series> <lag> <score, %.17g>
// tests/test_gpu_lag_band.py rebuilds the series and compares the lines with the CPU oracle's.  It also checks here that a band
// holding lag 0 gives RunSignedInLagRange's Scores bit for bit, that a Run behind the band calls is the Run it was, and that an
// empty band is refused.  Exit code 0 = ran through ("lag-band ok").  Needs a gfx950 GPU.
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

// series i: a pulse of 24 samples moved by shift(i), scaled, plus noise (muse_lag_range_test.cpp's); negated when i % 4 == 1
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

static void print(const char *what, char sign, int lo, int hi, const std::pair<Scores, double> &f)
{
    for (auto &sc : f.first) {
        std::string id;
        sc.Labels->Get("id", &id);
        printf("%s%c[%d,%d] %s %d %.17g\n", what, sign, lo, hi, id.c_str(), sc.Lag, sc.PercentScore);
    }
}

static int differ(const std::pair<Scores, double> &a, const std::pair<Scores, double> &b)
{
    int d = a.first.size() != b.first.size();
    for (size_t i = 0; i < a.first.size() && i < b.first.size(); i++)
        d += a.first[i].Lag != b.first[i].Lag || std::memcmp(&a.first[i].PercentScore, &b.first[i].PercentScore, 8) != 0 ||
             a.first[i].Labels->ID() != b.first[i].Labels->ID();
    return d;
}

int main()
{
    const int N = 1000, M = 240, MAXLAG = 300;
    const int bands[2][2] = {{1, 15}, {-300, -20}};
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(series(N, i), NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i / 6)}})));
    auto ref = NewSeries(series(N, -1), NewLabels({{"id", "ref"}}));
    int failures = 0;
    try {
        auto before = NewResults(MAXLAG, 12, 0.0, SignFilter_ANY);
        NewBatch(ref, g, before, 4)->Run({});
        const auto fb = before->Fetch();

        for (const SignFilter filter : {SignFilter_ANY, SignFilter_POS, SignFilter_NEG}) {
            const char sign = filter == SignFilter_ANY ? '0' : filter == SignFilter_POS ? '+' : '-';
            auto res = NewResults(MAXLAG, 12, 0.0, filter);
            auto b = NewBatch(ref, g, res, 4);
            for (auto &r : bands) {
                if (filter == SignFilter_ANY)
                    b->RunInLagBand({}, r[0], r[1]);
                else
                    b->RunSignedInLagBand({}, r[0], r[1]);
                print("nil", sign, r[0], r[1], res->Fetch());
                if (filter == SignFilter_ANY)
                    b->RunInLagBand({"graph"}, r[0], r[1]);
                else
                    b->RunSignedInLagBand({"graph"}, r[0], r[1]);
                print("graph", sign, r[0], r[1], res->Fetch());
            }
            // a band that holds lag 0 is the signed range call, bit for bit
            b->RunSignedInLagBand({"graph"}, -15, 40);
            const auto fs = res->Fetch();
            b->RunSignedInLagRange({"graph"}, -15, 40);
            failures += differ(fs, res->Fetch());
        }

        auto res = NewResults(MAXLAG, 12, 0.0, SignFilter_ANY);
        auto b = NewBatch(ref, g, res, 4);
        b->RunInLagBand({"graph"}, 1, 15);
        b->Run({}); // the Run of a batch that has scored a band is the Run it was
        failures += differ(res->Fetch(), fb);
        bool refused = false; // nothing of the band is left at this length (FFT length 1024: lags -511 .. 512)
        try {
            b->RunInLagBand({}, 600, 700);
        } catch (const Error &e) {
            refused = e.status == MUSE_ERR_INVALID;
        }
        if (!refused)
            failures++;
        refused = false;
        try {
            b->RunInLagBand({}, 7, 1);
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
    printf("lag-band ok\n");
    return 0;
}
