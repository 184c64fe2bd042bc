// csma_carry_san_test.cpp -- the pure host functions of the CSMA-CA carry (rm_csma_schedule_carry, rm_csma_carry_collect; extension E9) in a
// stand-alone program for a host sanitizer build: RM_MAX_BATCH ticks, max_be 8, a full carry list.  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_csma.cpp \
//       tests/cpp/csma_carry_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o csma_carry_san_test
// Exit status 0 and "ok": both functions ran over every case and their results are consistent with each other.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/radiomedium_hip.h"

static uint64_t g_state = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t((g_state >> 33) % n);
}

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    const int nt = RM_MAX_BATCH;
    rm_csma_params p;
    rm_csma_defaults(&p);
    p.max_backoffs = 5, p.min_be = 6, p.max_be = 8, p.seed = 0x8000000000000011ull;
    std::vector<int32_t> n_src(nt, 0);
    std::vector<int64_t> cca(nt);
    std::vector<std::vector<int32_t>> src(nt);
    std::vector<const int32_t *> lists(nt, nullptr);
    int64_t n_pkt = 0;
    for (int b = 0; b < nt; ++b) {
        cca[size_t(b)] = 1000ll * b + 128;
        if (b % 25 == 0 || b == nt - 1) n_src[size_t(b)] = 40;
        for (int k = 0; k < n_src[size_t(b)]; ++k) src[size_t(b)].push_back(int32_t(rnd(100000)));
        lists[size_t(b)] = src[size_t(b)].empty() ? nullptr : src[size_t(b)].data();
        n_pkt += n_src[size_t(b)];
    }
    for (int n_carry : {0, 1, 30000}) {
        std::vector<rm_csma_carry> carry;
        for (int c = 0; c < n_carry; ++c) // ticks from 0 to behind the batch (and INT32_MAX), every attempt number
            carry.push_back(rm_csma_carry{-1000ll * (1 + rnd(8)) + 128, int32_t(rnd(5000)), int32_t(rnd(100000)),
                                          c % 97 == 0 ? INT32_MAX : int32_t(rnd(nt + 40)), 1 + int32_t(rnd(5))});
        std::vector<int32_t> n_exp(nt, -1);
        int64_t total = -1;
        EXPECT(rm_csma_schedule_carry(&p, nt, n_src.data(), cca.data(), carry.data(), n_carry, n_exp.data(), nullptr, nullptr, 0, &total) == RM_OK);
        int64_t sum = 0;
        for (int32_t v : n_exp) sum += v;
        EXPECT(sum == total && total >= n_pkt);
        std::vector<int32_t> origin(size_t(total), -1);
        std::vector<uint8_t> attempt(size_t(total), 0xEE);
        if (total > 0)
            EXPECT(rm_csma_schedule_carry(&p, nt, n_src.data(), cca.data(), carry.data(), n_carry, n_exp.data(), origin.data(), attempt.data(),
                                          total - 1, &total) == RM_ERR_CAPACITY);
        EXPECT(rm_csma_schedule_carry(&p, nt, n_src.data(), cca.data(), carry.data(), n_carry, n_exp.data(), origin.data(), attempt.data(), total,
                                      &total) == RM_OK);
        std::vector<int> slots(size_t(n_pkt + n_carry), 0);
        for (int64_t i = 0; i < total; ++i) {
            EXPECT(origin[size_t(i)] >= 0 && origin[size_t(i)] < n_pkt + n_carry && attempt[size_t(i)] <= p.max_backoffs);
            ++slots[size_t(origin[size_t(i)])];
        }
        for (int64_t o = 0; o < n_pkt; ++o) EXPECT(slots[size_t(o)] >= 1 && slots[size_t(o)] <= 6);
        for (int c = 0; c < n_carry; ++c) EXPECT((slots[size_t(n_pkt + c)] == 0) == (carry[size_t(c)].tick >= nt));
        // collect over made-up tables: every status, ticks behind the batch for the pending ones
        std::vector<uint8_t> st(size_t(n_pkt + n_carry) + 1), at(size_t(n_pkt + n_carry) + 1);
        std::vector<int32_t> tk(size_t(n_pkt + n_carry) + 1);
        int64_t pending = 0;
        for (size_t e = 0; e < size_t(n_pkt + n_carry); ++e) {
            st[e] = uint8_t(rnd(4));
            at[e] = uint8_t(1 + rnd(5));
            tk[e] = st[e] == RM_CSMA_PENDING ? nt + int32_t(rnd(256)) : -1;
            pending += st[e] == RM_CSMA_PENDING;
        }
        const rm_csma_result own = {st.data(), at.data(), tk.data(), nullptr, nullptr, nullptr};
        const rm_csma_result car = {st.data() + n_pkt, at.data() + n_pkt, tk.data() + n_pkt, nullptr, nullptr, nullptr};
        std::vector<rm_csma_carry> next(size_t(pending) + 1);
        int64_t count = -1;
        EXPECT(rm_csma_carry_collect(nt, lists.data(), n_src.data(), cca.data(), carry.data(), n_carry, &own, &car, next.data(), pending, &count) == RM_OK);
        EXPECT(count == pending);
        for (int64_t i = 0; i < count; ++i) EXPECT(next[size_t(i)].tick >= 0 && next[size_t(i)].tick < 256 && next[size_t(i)].attempt >= 1);
        if (pending > 0) {
            EXPECT(rm_csma_carry_collect(nt, lists.data(), n_src.data(), cca.data(), carry.data(), n_carry, &own, &car, next.data(), pending - 1,
                                         &count) == RM_ERR_CAPACITY);
            EXPECT(count == pending);
        }
        EXPECT(rm_csma_carry_collect(nt, lists.data(), n_src.data(), cca.data(), carry.data(), n_carry, &own, &car, nullptr, 0, &count) ==
               (pending > 0 ? RM_ERR_CAPACITY : RM_OK));
        // the carry-out is a carry list the next batch's schedule takes (attempts 1 .. max_backoffs by construction of `at`)
        EXPECT(rm_csma_schedule_carry(&p, nt, n_src.data(), cca.data(), next.data(), int32_t(count), n_exp.data(), nullptr, nullptr, 0, &total) == RM_OK);
        std::printf("n_carry %d: %lld slots, carry-out %lld\n", n_carry, (long long)total, (long long)count);
    }
    std::printf("ok\n");
    return 0;
}
