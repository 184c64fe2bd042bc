// flood_host_san_test.cpp -- the pure host functions of the dissemination floods (rm_flood_defaults, rm_flood_validate,
// rm_flood_fire; extension E20) and the validation paths of its calls that end before any device is asked, in a stand-alone program
// for a host sanitizer build: schedules against the rule written out here, the largest parameters the rule allows (a signed
// overflow or a shift by 64 is the sanitizer's to find), and every call's refusal of a NULL context.  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_flood.cpp \
//       tests/cpp/flood_host_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o flood_host_san_test
// Exit status 0 and "ok": every case gave the outcome written down here.
#include <algorithm>
#include <cstdio>

#include "../../include/radiomedium_hip.h"

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static uint64_t mix(uint64_t z)
{
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the rule of DESIGN.md section 6, E20: the sum written as the loop the text gives
static void rule(const rm_flood_params &p, int32_t node, int64_t first, int32_t m, int64_t *start, int64_t *fire)
{
    if (m >= p.max_intervals) {
        *start = *fire = -1;
        return;
    }
    int64_t s = first;
    for (int i = 0; i < m; ++i) s += p.imin_us << std::min(i, p.doublings);
    const uint64_t half = uint64_t(p.imin_us << std::min(m, p.doublings)) / 2;
    uint64_t h = mix(mix(mix(p.seed + 0x9E3779B97F4A7C15ull) ^ uint64_t(uint32_t(node))) ^ uint64_t(first));
    h = mix(h ^ uint64_t(m));
    *start = s;
    *fire = s + int64_t(half) + int64_t(uint64_t((static_cast<unsigned __int128>(h) * half) >> 64));
}

int main()
{
    rm_flood_params p;
    rm_flood_defaults(&p);
    rm_flood_defaults(nullptr);
    EXPECT(p.imin_us == 8000 && p.doublings == 4 && p.max_intervals == 8 && p.redundancy == 2 && p.max_hops == 255 && p.seed == 0);
    EXPECT(rm_flood_validate(&p) == RM_OK && rm_flood_validate(nullptr) == RM_ERR_INVALID);
    // ---- validate: every field at and beyond its ends
    {
        const int64_t imin[] = {-1, 0, 1, 2, 3, int64_t(1) << 32, (int64_t(1) << 32) + 1};
        for (int64_t v : imin) {
            rm_flood_params b = p;
            b.imin_us = v;
            EXPECT((rm_flood_validate(&b) == RM_OK) == (v >= 2 && v <= (int64_t(1) << 32)));
        }
        for (int v = -2; v <= 70; ++v) {
            rm_flood_params b = p;
            b.doublings = v;
            EXPECT((rm_flood_validate(&b) == RM_OK) == (v >= 0 && v <= 16));
            b = p, b.max_intervals = v;
            EXPECT((rm_flood_validate(&b) == RM_OK) == (v >= 1 && v <= 64));
        }
        const int k[] = {-1, 0, 1, 255, 256}, hops[] = {-1, 0, 1, 65535, 65536};
        for (int v : k) {
            rm_flood_params b = p;
            b.redundancy = v;
            EXPECT((rm_flood_validate(&b) == RM_OK) == (v >= 0 && v <= 255));
        }
        for (int v : hops) {
            rm_flood_params b = p;
            b.max_hops = v;
            EXPECT((rm_flood_validate(&b) == RM_OK) == (v >= 1 && v <= 65535));
        }
    }
    // ---- fire: against the rule, up to the largest parameters
    {
        const uint64_t seeds[] = {0, 1, 0xDEADBEEFCAFEF00Dull, ~0ull};
        const int64_t imins[] = {2, 3, 8000, int64_t(1) << 32};
        const int ds[] = {0, 1, 4, 16}, nodes[] = {0, 1, 77, 2147483647};
        const int64_t firsts[] = {0, 1, 4356, int64_t(1) << 40};
        for (uint64_t seed : seeds)
            for (int64_t imin : imins)
                for (int d : ds) {
                    rm_flood_params q = p;
                    q.seed = seed, q.imin_us = imin, q.doublings = d, q.max_intervals = 64;
                    for (int node : nodes)
                        for (int64_t first : firsts)
                            for (int m = 0; m <= 64; ++m) {
                                int64_t s = -7, f = -7, ws, wf;
                                EXPECT(rm_flood_fire(&q, node, first, m, &s, &f) == RM_OK);
                                rule(q, node, first, m, &ws, &wf);
                                EXPECT(s == ws && f == wf);
                                if (m < 64) {
                                    const int64_t len = imin << std::min(m, d);
                                    EXPECT(f >= s + len / 2 && f < s + len);
                                }
                            }
                }
        int64_t s = -7, f = -7;
        EXPECT(rm_flood_fire(&p, -1, 0, 0, &s, &f) == RM_ERR_INVALID && rm_flood_fire(&p, 0, -1, 0, &s, &f) == RM_ERR_INVALID);
        EXPECT(rm_flood_fire(&p, 0, 0, -1, &s, &f) == RM_ERR_INVALID && rm_flood_fire(&p, 0, 0, 9, &s, &f) == RM_ERR_INVALID);
        EXPECT(rm_flood_fire(&p, 0, 0, 0, nullptr, &f) == RM_ERR_INVALID && rm_flood_fire(&p, 0, 0, 0, &s, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_flood_fire(nullptr, 0, 0, 0, &s, &f) == RM_ERR_INVALID && s == -7 && f == -7);
        rm_flood_params bad = p;
        bad.imin_us = 1;
        EXPECT(rm_flood_fire(&bad, 0, 0, 0, &s, &f) == RM_ERR_INVALID && s == -7);
        EXPECT(rm_flood_fire(&p, 0, 0, 8, &s, &f) == RM_OK && s == -1 && f == -1);
    }
    // ---- every call refuses a NULL context before anything else
    {
        int32_t list[3] = {0, 1, 2}, count = -7;
        rm_flood_node row;
        rm_flood_totals tot;
        const rm_flood_node *dn = nullptr;
        const rm_flood_totals *dt = nullptr;
        EXPECT(rm_flood_enable(nullptr, &p) == RM_ERR_INVALID && rm_flood_disable(nullptr) == RM_ERR_INVALID && rm_flood_enabled(nullptr) == 0);
        EXPECT(rm_flood_get_params(nullptr, &p) == RM_ERR_INVALID && rm_flood_reset(nullptr) == RM_ERR_INVALID);
        EXPECT(rm_flood_seed(nullptr, list, 3, 0) == RM_ERR_INVALID && rm_flood_seed_device(nullptr, list, 3, 0) == RM_ERR_INVALID);
        EXPECT(rm_flood_sources(nullptr, 0, 3, list, &count) == RM_ERR_INVALID && rm_flood_sources_device(nullptr, 0, 3, list, &count) == RM_ERR_INVALID);
        EXPECT(rm_flood_advance(nullptr, 0, list, 3) == RM_ERR_INVALID && rm_flood_advance_device(nullptr, 0, nullptr, 0) == RM_ERR_INVALID);
        EXPECT(rm_flood_read(nullptr, list, 1, &row, &tot) == RM_ERR_INVALID && rm_flood_device(nullptr, &dn, &dt) == RM_ERR_INVALID);
        EXPECT(rm_flood_tree_device(nullptr, list, nullptr) == RM_ERR_INVALID);
        EXPECT(count == -7 && list[0] == 0 && list[2] == 2 && dn == nullptr && dt == nullptr);
    }
    std::printf("ok\n");
    return 0;
}
