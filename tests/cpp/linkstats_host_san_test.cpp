// linkstats_host_san_test.cpp -- the pure host functions of the watched-link statistics (rm_linkstats_q8, rm_linkstats_validate;
// extension E14) in a stand-alone program for a host sanitizer build: the fixed point's edge inputs with their answers written
// down, and watch lists that are exactly as long as their counts say (a read past an end is the sanitizer's to find).  No device
// is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_linkstats.cpp \
//       tests/cpp/linkstats_host_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o linkstats_host_san_test
// Exit status 0 and "ok": every case gave the outcome written down here.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/radiomedium_hip.h"

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    // ---- q8: 1/256 dB, rounded half up
    EXPECT(rm_linkstats_q8(0.0) == 0 && rm_linkstats_q8(-0.0) == 0);
    EXPECT(rm_linkstats_q8(1.0) == 256 && rm_linkstats_q8(-1.0) == -256);
    EXPECT(rm_linkstats_q8(-91.5) == -23424);
    // ties at (m + 0.5) / 256 go up: to m + 1, for negative m as well
    for (long long m : {-3LL, -2LL, -1LL, 0LL, 1LL, 2LL, 1000LL, -1000LL, 25599LL, -25600LL}) EXPECT(rm_linkstats_q8((double(m) + 0.5) / 256.0) == m + 1);
    EXPECT(rm_linkstats_q8(0.49 / 256.0) == 0 && rm_linkstats_q8(-0.51 / 256.0) == -1);
    EXPECT(rm_linkstats_q8(std::numeric_limits<double>::denorm_min()) == 0 && rm_linkstats_q8(-std::numeric_limits<double>::denorm_min()) == 0);
    // the range: just inside 2^31 on both sides, then 0 from 2^31 on
    EXPECT(rm_linkstats_q8(2147483647.99) == 549755813885LL && rm_linkstats_q8(-2147483647.99) == -549755813885LL);
    EXPECT(rm_linkstats_q8(2147483648.0) == 0 && rm_linkstats_q8(-2147483648.0) == 0);
    EXPECT(rm_linkstats_q8(1e300) == 0 && rm_linkstats_q8(-1e300) == 0);
    EXPECT(rm_linkstats_q8(std::nan("")) == 0);
    EXPECT(rm_linkstats_q8(std::numeric_limits<double>::infinity()) == 0 && rm_linkstats_q8(-std::numeric_limits<double>::infinity()) == 0);

    // ---- validate: 6 nodes
    const int n_nodes = 6;
    {
        // a whole table for every K: row j watches j + 1 .. j + K (cyclic), never itself, all distinct
        for (int K : {1, 2, 4}) {
            std::vector<int32_t> rows;
            for (int j = 0; j < n_nodes; ++j)
                for (int k = 0; k < K; ++k) rows.push_back((j + 1 + k) % n_nodes);
            EXPECT(rm_linkstats_validate(n_nodes, K, nullptr, n_nodes, rows.data()) == RM_OK);
            EXPECT(rm_linkstats_validate(n_nodes, K, nullptr, n_nodes - 1, rows.data()) == RM_ERR_INVALID); // no list, another count
        }
        // K = 8 on six nodes: five peers and three empty slots a row
        std::vector<int32_t> rows;
        for (int j = 0; j < n_nodes; ++j)
            for (int k = 0; k < 8; ++k) rows.push_back(k < 5 ? (j + 1 + k) % n_nodes : -1);
        EXPECT(rm_linkstats_validate(n_nodes, 8, nullptr, n_nodes, rows.data()) == RM_OK);
    }
    {
        const std::vector<int32_t> nodes = {4, 0, 5};
        std::vector<int32_t> rows = {0, 1, -1, 5, /**/ -1, -1, -1, -1, /**/ 4, 3, 2, 1};
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 3, rows.data()) == RM_OK);
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 0, nullptr) == RM_OK); // an empty list
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 3, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), -1, rows.data()) == RM_ERR_INVALID);
        for (int K : {0, 3, 5, 6, 7, 9, 16, -1}) EXPECT(rm_linkstats_validate(n_nodes, K, nodes.data(), 1, rows.data()) == RM_ERR_INVALID);
        std::vector<int32_t> bad = rows;
        bad[3] = 4; // node 4 watches itself
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 3, bad.data()) == RM_ERR_INVALID);
        bad = rows;
        bad[11] = 4; // a repeated peer in the last row
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 3, bad.data()) == RM_ERR_INVALID);
        bad = rows;
        bad[8] = n_nodes; // one past the last node
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 3, bad.data()) == RM_ERR_INVALID);
        bad = rows;
        bad[2] = -2; // only -1 marks an empty slot
        EXPECT(rm_linkstats_validate(n_nodes, 4, nodes.data(), 3, bad.data()) == RM_ERR_INVALID);
        const std::vector<int32_t> twice = {4, 0, 4};
        std::vector<int32_t> rows2 = rows;
        rows2[8] = 0, rows2[9] = 1, rows2[10] = 2, rows2[11] = 3; // (a valid row for node 4 as well)
        EXPECT(rm_linkstats_validate(n_nodes, 4, twice.data(), 3, rows2.data()) == RM_ERR_INVALID);
        const std::vector<int32_t> out_of_range = {4, n_nodes, 5}, negative = {4, -1, 5};
        EXPECT(rm_linkstats_validate(n_nodes, 4, out_of_range.data(), 3, rows.data()) == RM_ERR_INVALID);
        EXPECT(rm_linkstats_validate(n_nodes, 4, negative.data(), 3, rows.data()) == RM_ERR_INVALID);
        EXPECT(rm_linkstats_validate(-1, 4, nodes.data(), 0, nullptr) == RM_ERR_INVALID);
    }
    // a long list (the duplicate test sorts a copy of it)
    {
        const int big = 5000;
        std::vector<int32_t> nodes, rows;
        for (int r = 0; r < big; ++r) {
            nodes.push_back((r * 7) % big); // a permutation: 7 and 5000 are coprime
            rows.push_back(nodes.back() == 0 ? 1 : 0);
            rows.push_back(-1);
        }
        EXPECT(rm_linkstats_validate(big, 2, nodes.data(), big, rows.data()) == RM_OK);
        nodes[big - 1] = nodes[17];
        rows[2 * (big - 1)] = rows[2 * 17];
        EXPECT(rm_linkstats_validate(big, 2, nodes.data(), big, rows.data()) == RM_ERR_INVALID);
    }
    std::printf("ok\n");
    return 0;
}
