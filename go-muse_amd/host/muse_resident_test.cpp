// muse_resident_test.cpp -- the C++ host mirror's reuse of resident rows (Group::ReuseResidentRows): a Group built from
// FilterByLabelValues of a resident Group, and Muse::Run over series that live in one, give bit for bit what the host path
// gives; a home that is released sends its series back to the host path.
// Exit code 0 = all passed ("resident ok").  Needs a gfx950 GPU (there is no CPU fallback).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "muse.hpp"

using namespace muse;
static int failures = 0;
#define EXPECT(cond, ...)                                                                       \
    do {                                                                                        \
        if (!(cond)) {                                                                          \
            failures++;                                                                         \
            printf("FAIL %s:%d: ", __FILE__, __LINE__);                                         \
            printf(__VA_ARGS__);                                                                \
            printf("\n");                                                                       \
        }                                                                                       \
    } while (0)

static std::vector<double> rows(int N, unsigned seed)
{
    std::mt19937_64 rng(seed);
    std::normal_distribution<double> nd;
    std::uniform_real_distribution<double> ud(0.5, 3.0);
    const double scale = ud(rng), shift = ud(rng) - 1.75;
    std::vector<double> y((size_t)N);
    for (auto &v : y)
        v = nd(rng) * scale + shift;
    return y;
}

static GroupPtr labelled(int M, int N, unsigned seed)
{
    auto g = NewGroup("all");
    for (int i = 0; i < M; i++)
        g->Add(NewSeries(rows(N, seed + (unsigned)i),
                         NewLabels({{"id", std::to_string(i)}, {"graph", "g" + std::to_string(i % 7)}, {"host", "h" + std::to_string(i % 3)}})));
    return g;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static void compare(const std::pair<Scores, double> &a, const std::pair<Scores, double> &b, const char *what, int N)
{
    EXPECT(a.first.size() == b.first.size(), "%s N=%d: %zu vs %zu scores", what, N, a.first.size(), b.first.size());
    for (size_t i = 0; i < a.first.size() && i < b.first.size(); i++) {
        EXPECT(a.first[i].Labels->ID() == b.first[i].Labels->ID(), "%s N=%d [%zu]: labels", what, N, i);
        EXPECT(a.first[i].Lag == b.first[i].Lag, "%s N=%d [%zu]: lag %d vs %d", what, N, i, a.first[i].Lag, b.first[i].Lag);
        EXPECT(same_bits(a.first[i].PercentScore, b.first[i].PercentScore), "%s N=%d [%zu]: score %.17g vs %.17g", what, N, i,
               a.first[i].PercentScore, b.first[i].PercentScore);
    }
    EXPECT(same_bits(a.second, b.second) || (std::isnan(a.second) && std::isnan(b.second)), "%s N=%d: mean", what, N);
}

int main()
{
    for (int N : {480, 4096}) {
        auto big = labelled(210, N, 1000u * (unsigned)N);
        auto ref = NewSeries(rows(N, 7), NewLabels({{"id", "ref"}}));
        NewBatch(ref, big, NewResults(N, 20, 0.0, SignFilter_ANY), 4)->Run({"graph"}); // big becomes resident: the series' home
        big->indexLabelValues({"host"});
        const auto members = big->FilterByLabelValues(*NewLabels({{"host", "h1"}}));
        EXPECT(members.size() == 70, "FilterByLabelValues: %zu members", members.size());

        // a sub-group: its rows gathered from big's (and one series without a home uploaded in between)
        std::pair<Scores, double> sub_out[2];
        for (int on = 1; on >= 0; on--) {
            Group::ReuseResidentRows = on != 0;
            auto sub = NewGroup("h1");
            for (size_t i = 0; i < members.size(); i++) {
                sub->Add(members[i]);
                if (i == 30)
                    sub->Add(NewSeries(rows(N, 99), NewLabels({{"id", "x"}, {"graph", "g1"}, {"host", "h1"}})));
            }
            auto res = NewResults(N, 10, 0.0, SignFilter_ANY);
            NewBatch(ref, sub, res, 4)->Run({"graph"});
            sub_out[on] = res->Fetch();
        }
        compare(sub_out[1], sub_out[0], "sub-group", N);

        // Muse.Run over label groups of the resident group, one caller and sixteen
        big->indexLabelValues({"graph"});
        std::vector<std::vector<SeriesPtr>> graphs;
        for (int g = 0; g < 7; g++)
            graphs.push_back(big->FilterByLabelValues(*NewLabels({{"graph", "g" + std::to_string(g)}})));
        std::pair<Scores, double> run_out[2];
        for (int on = 1; on >= 0; on--) {
            Group::ReuseResidentRows = on != 0;
            auto res = NewResults(N, 7, 0.0, SignFilter_ANY);
            auto m = std::make_shared<Muse>(ref, res);
            for (auto &g : graphs)
                m->Run(g);
            run_out[on] = res->Fetch();
        }
        compare(run_out[1], run_out[0], "Muse.Run", N);
        Group::ReuseResidentRows = true;
        {
            // sixteen callers on one Muse: every caller's seven Scores are the serial ones (as multisets: the heap's order among
            // equal scores depends on arrival)
            auto res = NewResults(N, 1000, 0.0, SignFilter_ANY);
            auto m = std::make_shared<Muse>(ref, res);
            std::vector<std::thread> th;
            for (int t = 0; t < 16; t++)
                th.emplace_back([&, t] {
                    for (int g = 0; g < 7; g++)
                        m->Run(graphs[(size_t)((t + g) % 7)]);
                });
            for (auto &t : th)
                t.join();
            auto key = [](const Score &s) {
                char b[64];
                snprintf(b, sizeof(b), "|%d|%a", s.Lag, s.PercentScore);
                return s.Labels->ID() + b;
            };
            std::vector<std::string> got, want;
            for (auto &s : res->Fetch().first)
                got.push_back(key(s));
            for (int t = 0; t < 16; t++)
                for (auto &s : run_out[0].first)
                    want.push_back(key(s));
            std::sort(got.begin(), got.end());
            std::sort(want.begin(), want.end());
            EXPECT(got == want, "Muse.Run x16 N=%d: %zu scores vs %zu", N, got.size(), want.size());
        }
        // the home goes: the same series take the host path again
        big.reset();
        {
            auto res = NewResults(N, 7, 0.0, SignFilter_ANY);
            auto m = std::make_shared<Muse>(ref, res);
            for (auto &g : graphs)
                m->Run(g);
            compare(res->Fetch(), run_out[0], "Muse.Run after the home is freed", N);
        }
    }
    if (failures == 0)
        printf("resident ok\n");
    return failures == 0 ? 0 : 1;
}
