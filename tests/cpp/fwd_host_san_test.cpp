// fwd_host_san_test.cpp -- the pure host functions of the forwarding queues (rm_fwd_defaults, rm_fwd_validate, rm_fwd_backoff;
// extension E19) and the validation paths of its calls that end before any device is asked, in a stand-alone program for a host
// sanitizer build: backoff delays against the rule written out here, the largest parameters the rule allows (a signed overflow or
// a shift by 64 is the sanitizer's to find), and every call's refusal of a NULL context.  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_fwd.cpp \
//       tests/cpp/fwd_host_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o fwd_host_san_test
// Exit status 0 and "ok": every case gave the outcome written down here.
#include <algorithm>
#include <cstdio>
#include <vector>

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

// the rule of DESIGN.md section 6, E19
static int64_t delay(const rm_fwd_params &p, int32_t node, int64_t start, int32_t tries)
{
    const int be = std::min(p.min_be + tries - 1, p.max_be);
    if (be == 0) return 0;
    const uint64_t h1 = mix(mix(mix(p.seed + 0x9E3779B97F4A7C15ull) ^ uint64_t(uint32_t(node))) ^ uint64_t(start));
    return int64_t(mix(h1 ^ uint64_t(tries)) >> (64 - be)) * p.backoff_unit_us;
}

int main()
{
    rm_fwd_params p;
    rm_fwd_defaults(&p);
    rm_fwd_defaults(nullptr);
    EXPECT(p.queue_slots == 8 && p.max_retries == 3 && p.min_be == 3 && p.max_be == 5 && p.max_hops == 64 && p.backoff_unit_us == 320 && p.seed == 0 &&
           p.reserved == 0);
    EXPECT(rm_fwd_validate(&p) == RM_OK && rm_fwd_validate(nullptr) == RM_ERR_INVALID);
    // ---- validate: every field at and beyond its ends
    {
        for (int q = -2; q <= 40; ++q) {
            rm_fwd_params b = p;
            b.queue_slots = q;
            EXPECT((rm_fwd_validate(&b) == RM_OK) == (q == 1 || q == 2 || q == 4 || q == 8 || q == 16));
        }
        for (int lo = -1; lo <= 9; ++lo)
            for (int hi = -1; hi <= 9; ++hi) {
                rm_fwd_params b = p;
                b.min_be = lo, b.max_be = hi;
                EXPECT((rm_fwd_validate(&b) == RM_OK) == (0 <= lo && lo <= hi && hi <= 8));
            }
        rm_fwd_params b = p;
        b.max_retries = 15; EXPECT(rm_fwd_validate(&b) == RM_OK);
        b.max_retries = 16; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b.max_retries = -1; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b = p;
        b.max_hops = 255; EXPECT(rm_fwd_validate(&b) == RM_OK);
        b.max_hops = 256; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b.max_hops = 0; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b = p;
        b.backoff_unit_us = int64_t(1) << 32; EXPECT(rm_fwd_validate(&b) == RM_OK);
        b.backoff_unit_us += 1; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b.backoff_unit_us = -1; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b = p;
        b.reserved = 1; EXPECT(rm_fwd_validate(&b) == RM_ERR_INVALID);
        b = p;
        b.seed = ~0ull; EXPECT(rm_fwd_validate(&b) == RM_OK);
    }
    // ---- backoff: the rule, at the ends of every argument
    {
        int64_t d = -7;
        const uint64_t seeds[] = {0ull, 1ull, 0xDEADBEEFCAFEF00Dull, ~0ull};
        const int bes[][2] = {{0, 0}, {0, 8}, {3, 5}, {8, 8}, {1, 1}};
        const int64_t units[] = {0, 320, int64_t(1) << 32};
        const int32_t nodes[] = {0, 1, 77, 2147483647};
        const int64_t starts[] = {0, 1, 4356, (int64_t(1) << 62) + 5, INT64_MAX};
        const int32_t tries[] = {1, 2, 3, 16, 2147483647};
        int nonzero = 0;
        for (uint64_t seed : seeds)
            for (const int(&be)[2] : bes)
                for (int64_t unit : units) {
                    rm_fwd_params b = p;
                    b.seed = seed, b.min_be = be[0], b.max_be = be[1], b.backoff_unit_us = unit;
                    for (int32_t node : nodes)
                        for (int64_t start : starts)
                            for (int32_t t : tries) {
                                const int64_t grown = int64_t(b.min_be) + t - 1; // (in 64 bits: tries may be 2^31 - 1)
                                EXPECT(rm_fwd_backoff(&b, node, start, t, &d) == RM_OK);
                                const int bexp = int(std::min<int64_t>(grown, b.max_be));
                                EXPECT(d >= 0 && (unit == 0 ? d == 0 : (d % unit == 0 && d / unit < (int64_t(1) << bexp))));
                                if (t <= 16) EXPECT(d == delay(b, node, start, t));
                                nonzero += d != 0;
                            }
                }
        EXPECT(nonzero > 1000);
        d = -7;
        EXPECT(rm_fwd_backoff(&p, -1, 0, 1, &d) == RM_ERR_INVALID && rm_fwd_backoff(&p, 0, -1, 1, &d) == RM_ERR_INVALID);
        EXPECT(rm_fwd_backoff(&p, 0, 0, 0, &d) == RM_ERR_INVALID && rm_fwd_backoff(&p, 0, 0, -1, &d) == RM_ERR_INVALID);
        EXPECT(rm_fwd_backoff(nullptr, 0, 0, 1, &d) == RM_ERR_INVALID && rm_fwd_backoff(&p, 0, 0, 1, nullptr) == RM_ERR_INVALID && d == -7);
        rm_fwd_params bad = p;
        bad.queue_slots = 3;
        EXPECT(rm_fwd_backoff(&bad, 0, 0, 1, &d) == RM_ERR_INVALID && d == -7);
    }
    // ---- every call refuses a NULL context before anything else
    {
        std::vector<int32_t> list = {0, 1, 2};
        int32_t count = -7;
        rm_fwd_node row;
        rm_fwd_totals tot;
        rm_fwd_packet pk[16];
        const rm_fwd_node *dn = nullptr;
        EXPECT(rm_fwd_enable(nullptr, &p) == RM_ERR_INVALID && rm_fwd_disable(nullptr) == RM_ERR_INVALID && rm_fwd_enabled(nullptr) == 0);
        EXPECT(rm_fwd_reset(nullptr) == RM_ERR_INVALID);
        rm_fwd_params got = p;
        EXPECT(rm_fwd_get_params(nullptr, &got) == RM_ERR_INVALID && got.queue_slots == p.queue_slots);
        EXPECT(rm_fwd_set_next(nullptr, list.data(), list.data(), 3, 0) == RM_ERR_INVALID);
        EXPECT(rm_fwd_set_next_device(nullptr, list.data(), list.data(), 3, 0) == RM_ERR_INVALID);
        EXPECT(rm_fwd_inject(nullptr, list.data(), 3, 0) == RM_ERR_INVALID && rm_fwd_inject_device(nullptr, list.data(), 3, 0) == RM_ERR_INVALID);
        EXPECT(rm_fwd_sources(nullptr, 0, 3, list.data(), &count) == RM_ERR_INVALID && count == -7);
        EXPECT(rm_fwd_sources_device(nullptr, 0, 3, list.data(), &count) == RM_ERR_INVALID);
        EXPECT(rm_fwd_advance(nullptr, 0, list.data(), 3) == RM_ERR_INVALID && rm_fwd_advance_device(nullptr, 0, nullptr, 0) == RM_ERR_INVALID);
        EXPECT(rm_fwd_read(nullptr, nullptr, 1, &row, &tot) == RM_ERR_INVALID && rm_fwd_queue_read(nullptr, list.data(), 1, pk, &count) == RM_ERR_INVALID);
        EXPECT(rm_fwd_device(nullptr, &dn, nullptr, nullptr) == RM_ERR_INVALID && dn == nullptr);
        EXPECT(list[0] == 0 && list[1] == 1 && list[2] == 2);
    }
    std::printf("ok\n");
    return 0;
}
