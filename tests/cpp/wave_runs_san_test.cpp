// wave_runs_san_test.cpp -- the index rule of the heard form's full-lane record copies (rm_device.hpp: kCopySpan, run_of,
// run_place; wave_copy_lists walks by it on the device) in a stand-alone program for a host sanitizer build.  For length vectors
// of 64 runs -- random and adversarial: all empty, one long run at either end, totals at and around every multiple of the span,
// runs at the list limit -- the wave's walk is replayed exactly as the kernel does it (spans of kCopyRounds rounds of 64 lanes)
// and held to a plain expansion of the runs: every entry j < total is taken exactly once and lands on the right run and the
// right place in it.  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Iradio-sim_amd/csrc -x hip \
//       tests/cpp/wave_runs_san_test.cpp -o wave_runs_san_test
// Exit status 0 and "ok": every vector passed.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rm_device.hpp"

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) // [0, n)
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t((g_rng >> 33) % n);
}

static int check(const std::vector<uint32_t> &cnt)
{
    EXPECT(cnt.size() == 64);
    // what the kernels' prologue gives every lane: the inclusive running counts
    std::vector<uint32_t> inc(64);
    uint32_t total = 0;
    for (int f = 0; f < 64; ++f) inc[f] = (total += cnt[f]);
    // the plain expansion: entry j -> (run, place)
    std::vector<int> run;
    std::vector<uint32_t> place;
    for (int f = 0; f < 64; ++f)
        for (uint32_t k = 0; k < cnt[f]; ++k) {
            run.push_back(f);
            place.push_back(k);
        }
    EXPECT(run.size() == total);
    const uint32_t *const inc_p = inc.data();
    auto inc_at = [inc_p](const int i) { return inc_p[i]; };
    // beyond the total: the last lane, as the kernels' shuffles need a lane that exists
    EXPECT(rm::run_of(inc_at, total) == 63 && rm::run_of(inc_at, total + 1000u) == 63 && rm::run_of(inc_at, 0xFFFFFFFFu) == 63);
    std::vector<uint8_t> taken(total, 0); // (exactly as long as the total: a j beyond it is the sanitizer's to find)
    for (uint32_t j0 = 0; j0 < total; j0 += rm::kCopySpan)
        for (int u = 0; u < rm::kCopyRounds; ++u)
            for (int lane = 0; lane < 64; ++lane) {
                const uint32_t j = j0 + uint32_t(u * 64 + lane);
                const int f = rm::run_of(inc_at, j);
                EXPECT(f >= 0 && f < 64);
                if (j >= total) continue; // (the copy's guard)
                const uint32_t k = rm::run_place(inc[f], cnt[f], j);
                EXPECT(f == run[j] && k == place[j] && k < cnt[f]);
                EXPECT(taken[j] == 0);
                taken[j] = 1;
            }
    for (uint32_t j = 0; j < total; ++j) EXPECT(taken[j] == 1);
    return 0;
}

int main()
{
    static_assert(rm::kCopySpan == 256u && rm::kCopyRounds == 4, "the cases below are written for spans of 256");
    std::vector<std::vector<uint32_t>> cases;
    cases.push_back(std::vector<uint32_t>(64, 0u));             // nothing at all
    cases.push_back(std::vector<uint32_t>(64, 1u));             // one entry per run
    cases.push_back(std::vector<uint32_t>(64, 1024u));          // every run at the list limit (kNcListCap): 65536 entries
    for (const int at : {0, 1, 31, 62, 63}) {                  // one run alone, short and long
        for (const uint32_t len : {1u, 63u, 64u, 65u, 255u, 256u, 257u, 1024u}) {
            std::vector<uint32_t> c(64, 0u);
            c[at] = len;
            cases.push_back(c);
        }
    }
    // totals at, one below and one above every multiple of the span up to 16 spans and beyond: 4 per run, two runs moved by one
    for (uint32_t m = 1; m <= 40; ++m)
        for (const int d : {-1, 0, 1}) {
            const uint32_t total = m * 256u + uint32_t(d);
            std::vector<uint32_t> c(64, total / 64u);
            uint32_t rest = total - (total / 64u) * 64u;
            for (int f = 63; rest > 0; --f, --rest) c[f] += 1u;
            cases.push_back(c);
            // the same total in few runs with empty ones between them
            std::vector<uint32_t> s(64, 0u);
            uint32_t left = total;
            for (int f = 3; f < 64 && left > 0; f += 7) {
                const uint32_t take = left < 1024u ? left : 1024u;
                s[f] = take;
                left -= take;
            }
            for (int f = 0; f < 64 && left > 0; ++f) {
                const uint32_t take = (1024u - s[f]) < left ? (1024u - s[f]) : left;
                s[f] += take;
                left -= take;
            }
            cases.push_back(s);
        }
    // random: lengths like the lists' (tens), sparse ones, and the whole range up to the list limit
    for (int it = 0; it < 300; ++it) {
        std::vector<uint32_t> c(64);
        for (int f = 0; f < 64; ++f) {
            const uint32_t kind = it % 3;
            if (kind == 0) c[f] = rnd(90);
            else if (kind == 1) c[f] = rnd(4) ? 0u : rnd(300);
            else c[f] = rnd(1025);
        }
        cases.push_back(c);
    }
    for (const std::vector<uint32_t> &c : cases)
        if (check(c)) return 1;
    std::printf("%zu length vectors\nok\n", cases.size());
    return 0;
}
