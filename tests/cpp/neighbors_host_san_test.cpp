// neighbors_host_san_test.cpp -- the pure host function of the neighbour query (rm_neighbors_from_result; extension E16) in a
// stand-alone program for a host sanitizer build: packets without links, a K larger than any degree, ties, a NaN rssi, results
// whose arrays are exactly as long as their counts say (a read past an end is the sanitizer's to find).  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_neighbors.cpp \
//       tests/cpp/neighbors_host_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o neighbors_host_san_test
// Exit status 0 and "ok": every case gave the outcome written down here.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/radiomedium_hip.h"

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static uint64_t bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof(b));
    return b;
}

int main()
{
    const uint64_t kNoRssi = 0x7FF8000000000000ull;
    // four packets: no link; three links with a tie; one link; five links, a NaN and the two zeros among them
    const std::vector<uint32_t> off = {0, 0, 3, 4, 9};
    const std::vector<int32_t> dst = {2, 5, 7, 1, 0, 3, 4, 6, 8};
    const std::vector<double> rssi = {-80.0, -70.0, -80.0, -60.5, 0.0, std::nan(""), -0.0, -1.0, 1.0};
    rm_host_result r{};
    r.count = 9;
    r.n_packets = 4;
    r.pkt_offset = off.data();
    r.dst = dst.data();
    r.rssi = rssi.data();
    // ---- K larger than any degree: every link, in the rule's order, then the padding
    {
        const int K = 16;
        std::vector<int32_t> peer(4 * K, 77), deg(4, 77);
        std::vector<double> out(4 * K, 77.0);
        EXPECT(rm_neighbors_from_result(&r, 4, K, peer.data(), out.data(), deg.data()) == RM_OK);
        EXPECT(deg[0] == 0 && deg[1] == 3 && deg[2] == 1 && deg[3] == 4);
        for (int k = 0; k < K; ++k) EXPECT(peer[k] == -1 && bits(out[k]) == kNoRssi);
        EXPECT(peer[K] == 5 && peer[K + 1] == 2 && peer[K + 2] == 7 && peer[K + 3] == -1); // the tie at -80: node 2 before node 7
        EXPECT(out[K] == -70.0 && out[K + 1] == -80.0 && out[K + 2] == -80.0 && bits(out[K + 3]) == kNoRssi);
        EXPECT(peer[2 * K] == 1 && out[2 * K] == -60.5 && peer[2 * K + 1] == -1);
        // 1.0 first; +0.0 and -0.0 are equal: nodes 0 and 4 by index, each with its own bits; -1.0; the NaN is no link
        EXPECT(peer[3 * K] == 8 && peer[3 * K + 1] == 0 && peer[3 * K + 2] == 4 && peer[3 * K + 3] == 6 && peer[3 * K + 4] == -1);
        EXPECT(bits(out[3 * K + 1]) == bits(0.0) && bits(out[3 * K + 2]) == bits(-0.0));
    }
    // ---- K = 1 and 2: the first links alone; rssi and degree may be NULL; exactly n_pkt * K entries are written
    {
        std::vector<int32_t> peer(4);
        EXPECT(rm_neighbors_from_result(&r, 4, 1, peer.data(), nullptr, nullptr) == RM_OK);
        EXPECT(peer[0] == -1 && peer[1] == 5 && peer[2] == 1 && peer[3] == 8);
        std::vector<int32_t> two(2 * 2), deg(2);
        std::vector<double> out(2 * 2);
        EXPECT(rm_neighbors_from_result(&r, 2, 2, two.data(), out.data(), deg.data()) == RM_OK); // the first two packets
        EXPECT(two[0] == -1 && two[1] == -1 && two[2] == 5 && two[3] == 2 && deg[0] == 0 && deg[1] == 3);
        EXPECT(rm_neighbors_from_result(&r, 0, 2, two.data(), nullptr, nullptr) == RM_OK && two[2] == 5); // no packet: nothing written
    }
    // ---- a full row meets better and worse links: 40 links of descending then ascending rssi, ties in pairs
    {
        std::vector<uint32_t> o2 = {0, 40};
        std::vector<int32_t> d2;
        std::vector<double> r2;
        for (int i = 0; i < 40; ++i) {
            d2.push_back(i);
            r2.push_back(i < 20 ? -50.0 - double(i / 2) : -90.0 + double((i - 20) / 2) * 5.0);
        }
        rm_host_result q{};
        q.count = 40;
        q.n_packets = 1;
        q.pkt_offset = o2.data();
        q.dst = d2.data();
        q.rssi = r2.data();
        std::vector<int32_t> peer(4), deg(1);
        std::vector<double> out(4);
        EXPECT(rm_neighbors_from_result(&q, 1, 4, peer.data(), out.data(), deg.data()) == RM_OK);
        // the ascending part ends at -90 + 9 * 5 = -45 (nodes 38, 39), then -50 (nodes 0, 1, 36, 37)
        EXPECT(deg[0] == 40 && peer[0] == 38 && peer[1] == 39 && peer[2] == 0 && peer[3] == 1);
        EXPECT(out[0] == -45.0 && out[1] == -45.0 && out[2] == -50.0 && out[3] == -50.0);
    }
    // ---- one rssi per packet (the reference's media): every link ties, the order is the node order
    {
        const std::vector<double> pr = {1.0, 2.0, 3.0, 4.0};
        rm_host_result q = r;
        q.rssi = nullptr;
        q.pkt_rssi = pr.data();
        std::vector<int32_t> peer(4 * 2);
        std::vector<double> out(4 * 2);
        EXPECT(rm_neighbors_from_result(&q, 4, 2, peer.data(), out.data(), nullptr) == RM_OK);
        EXPECT(peer[2] == 2 && peer[3] == 5 && out[2] == 2.0 && peer[6] == 0 && peer[7] == 3 && out[7] == 4.0);
    }
    // ---- refusals
    {
        std::vector<int32_t> peer(4 * 16);
        EXPECT(rm_neighbors_from_result(nullptr, 4, 4, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_neighbors_from_result(&r, 4, 4, nullptr, nullptr, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_neighbors_from_result(&r, 4, 0, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_neighbors_from_result(&r, 4, 17, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_neighbors_from_result(&r, 5, 4, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_neighbors_from_result(&r, -1, 4, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        rm_host_result q = r;
        q.rssi = nullptr; // links without an rssi column
        EXPECT(rm_neighbors_from_result(&q, 4, 4, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        q = r;
        q.pkt_offset = nullptr;
        EXPECT(rm_neighbors_from_result(&q, 4, 4, peer.data(), nullptr, nullptr) == RM_ERR_INVALID);
        rm_host_result none{}; // an empty result needs no array
        none.n_packets = 2;
        EXPECT(rm_neighbors_from_result(&none, 2, 4, peer.data(), nullptr, nullptr) == RM_OK && peer[0] == -1 && peer[7] == -1);
    }
    std::printf("ok\n");
    return 0;
}
