// unicast_host_san_test.cpp -- the pure host function of the unicast outcome query (rm_unicast_from_result; extension E12) in a
// stand-alone program for a host sanitizer build: small hand-made results (an empty segment, one link, a wanted node below /
// above / between the receivers), both rssi layouts, every output pointer NULL in turn.  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_unicast.cpp \
//       tests/cpp/unicast_host_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o unicast_host_san_test
// Exit status 0 and "ok": every case gave the outcome written down here.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/radiomedium_hip.h"

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    // five packets over 10 nodes: an empty segment, one link, three links, a padding entry, three links again
    // (every array is exactly as long as the result says: a read past an end is the sanitizer's to find)
    const std::vector<uint32_t> off = {0, 0, 1, 4, 4, 7};
    const std::vector<int32_t> dst = {5, 2, 4, 8, 1, 3, 9};
    const std::vector<uint8_t> ver = {RM_DELIVERED, RM_INTERFERED, RM_DELIVERED, RM_DELIVERED, RM_DELIVERED, RM_INTERFERED, RM_DELIVERED};
    const std::vector<double> rssi = {-50.0, -61.0, -62.0, -63.0, -71.0, -72.0, -73.0};
    const std::vector<double> sinr = {10.0, 1.0, 12.0, 13.0, 21.0, 2.0, 23.0};
    const std::vector<double> pkt_rssi = {0.0, 1.0, 2.0, 3.0, 4.0};
    const std::vector<int32_t> src = {0, 6, 7, -1, 0};
    const int n_nodes = 10, n = 5;
    rm_host_result r;
    std::memset(&r, 0, sizeof(r));
    r.count = 7, r.n_packets = 5, r.pkt_offset = off.data(), r.dst = dst.data(), r.verdict = ver.data(), r.rssi = rssi.data(), r.sinr = sinr.data();

    struct Case {
        std::vector<int32_t> want;
        std::vector<int> status, link;
    };
    const std::vector<Case> cases = {
        // below the first receiver, the one link, the first link, a padding entry, the last link
        {{0, 5, 2, 4, 9}, {RM_UC_UNHEARD, RM_UC_DELIVERED, RM_UC_INTERFERED, RM_UC_NOT_SENT, RM_UC_DELIVERED}, {-1, 0, 1, -1, 6}},
        // above the last receiver (the next segment's first receiver is not this one's), between two receivers, not asked
        {{9, 6, 9, -1, 2}, {RM_UC_UNHEARD, RM_UC_UNHEARD, RM_UC_UNHEARD, RM_UC_NONE, RM_UC_UNHEARD}, {-1, -1, -1, -1, -1}},
        // below the one link, the middle and the last of three, the source itself
        {{-1, 4, 4, 0, 3}, {RM_UC_NONE, RM_UC_UNHEARD, RM_UC_DELIVERED, RM_UC_NOT_SENT, RM_UC_INTERFERED}, {-1, -1, 2, -1, 5}},
        {{3, 9, 8, 9, 0}, {RM_UC_UNHEARD, RM_UC_UNHEARD, RM_UC_DELIVERED, RM_UC_NOT_SENT, RM_UC_UNHEARD}, {-1, -1, 3, -1, -1}},
    };
    for (int layout = 0; layout < 2; ++layout) {
        r.rssi = layout ? nullptr : rssi.data();
        r.pkt_rssi = layout ? pkt_rssi.data() : nullptr;
        for (int with_sinr = 0; with_sinr < 2; ++with_sinr) {
            r.sinr = with_sinr ? sinr.data() : nullptr;
            for (const Case &c : cases)
                for (int drop = -1; drop < 5; ++drop) { // every output pointer NULL in turn (-1: none)
                    std::vector<uint8_t> st(n, 0xEE);
                    std::vector<int32_t> lk(n, -7), rp(n, -7);
                    std::vector<double> rs(n, 99.0), sn(n, 99.0);
                    rm_unicast_out o = {st.data(), lk.data(), rs.data(), sn.data(), rp.data()};
                    if (drop == 0) o.status = nullptr;
                    if (drop == 1) o.link = nullptr;
                    if (drop == 2) o.rssi = nullptr;
                    if (drop == 3) o.sinr = nullptr;
                    if (drop == 4) o.reply_src = nullptr;
                    EXPECT(rm_unicast_from_result(&r, src.data(), n_nodes, c.want.data(), &o) == RM_OK);
                    for (int p = 0; p < n; ++p) {
                        const int i = c.link[size_t(p)];
                        if (drop != 0) EXPECT(st[size_t(p)] == c.status[size_t(p)]);
                        else EXPECT(st[size_t(p)] == 0xEE);
                        if (drop != 1) EXPECT(lk[size_t(p)] == i);
                        if (drop != 2) EXPECT(i < 0 ? std::isnan(rs[size_t(p)]) : rs[size_t(p)] == (layout ? pkt_rssi[size_t(p)] : rssi[size_t(i)]));
                        if (drop != 3) EXPECT((i < 0 || !with_sinr) ? std::isnan(sn[size_t(p)]) : sn[size_t(p)] == sinr[size_t(i)]);
                        if (drop != 4) EXPECT(rp[size_t(p)] == (c.status[size_t(p)] == RM_UC_DELIVERED ? c.want[size_t(p)] : -1));
                    }
                }
        }
    }
    // without the sources every packet counts as sent: the padding entry's segment is empty, so it reads as unheard
    {
        std::vector<uint8_t> st(n, 0xEE);
        rm_unicast_out o = {st.data(), nullptr, nullptr, nullptr, nullptr};
        const std::vector<int32_t> want = {0, 5, 2, 4, 9};
        r.rssi = rssi.data(), r.pkt_rssi = nullptr;
        EXPECT(rm_unicast_from_result(&r, nullptr, n_nodes, want.data(), &o) == RM_OK);
        EXPECT(st[3] == RM_UC_UNHEARD && st[1] == RM_UC_DELIVERED);
    }
    // a result without packets and without arrays
    {
        rm_host_result e;
        std::memset(&e, 0, sizeof(e));
        rm_unicast_out o = {nullptr, nullptr, nullptr, nullptr, nullptr};
        EXPECT(rm_unicast_from_result(&e, nullptr, n_nodes, nullptr, &o) == RM_OK);
    }
    // refusals: nothing is written
    {
        std::vector<uint8_t> st(n, 0xEE);
        rm_unicast_out o = {st.data(), nullptr, nullptr, nullptr, nullptr};
        const std::vector<int32_t> bad = {0, 5, n_nodes, 4, 9}, good = {0, 5, 2, 4, 9};
        EXPECT(rm_unicast_from_result(&r, src.data(), n_nodes, bad.data(), &o) == RM_ERR_INVALID);
        EXPECT(rm_unicast_from_result(nullptr, src.data(), n_nodes, good.data(), &o) == RM_ERR_INVALID);
        EXPECT(rm_unicast_from_result(&r, src.data(), n_nodes, nullptr, &o) == RM_ERR_INVALID);
        EXPECT(rm_unicast_from_result(&r, src.data(), n_nodes, good.data(), nullptr) == RM_ERR_INVALID);
        EXPECT(rm_unicast_from_result(&r, src.data(), -1, good.data(), &o) == RM_ERR_INVALID);
        for (uint8_t v : st) EXPECT(v == 0xEE);
    }
    std::printf("ok\n");
    return 0;
}
