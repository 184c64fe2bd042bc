// traffic_host_san_test.cpp -- the pure host functions of the traffic schedules (rm_traffic_due, rm_traffic_validate; extension
// E15) in a stand-alone program for a host sanitizer build: due times with their answers written down, the largest packet numbers
// and periods the rule allows (a signed overflow is the sanitizer's to find), and lists that are exactly as long as their counts
// say (a read past an end likewise).  No device is touched.
// Build (host code only; never loaded into another process, never run on a GPU):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -x hip radio-sim_amd/csrc/rm_api_traffic.cpp \
//       tests/cpp/traffic_host_san_test.cpp -Lradio-sim_amd/csrc -lradiomedium_hip -Wl,-rpath,radio-sim_amd/csrc -o traffic_host_san_test
// Exit status 0 and "ok": every case gave the outcome written down here.
#include <cstdio>
#include <vector>

#include "../../include/radiomedium_hip.h"

#define EXPECT(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    const int64_t P40 = int64_t(1) << 40, T62 = int64_t(1) << 62;
    int64_t due = -1;
    // ---- due: without jitter phase + k * period
    {
        const rm_traffic_schedule s = {100, 30, 0, 0};
        for (int64_t k : {int64_t(0), int64_t(1), int64_t(2), int64_t(1000000)}) {
            EXPECT(rm_traffic_due(&s, 7, 3, k, &due) == 1 && due == 30 + k * 100);
        }
        EXPECT(rm_traffic_due(&s, 7, 3, T62 / 100, &due) == 1 && due == 30 + (T62 / 100) * 100);
        EXPECT(rm_traffic_due(&s, 7, 3, T62 / 100 + 1, &due) == RM_ERR_INVALID);
        EXPECT(rm_traffic_due(&s, 7, 3, -1, &due) == RM_ERR_INVALID && rm_traffic_due(&s, 7, -1, 0, &due) == RM_ERR_INVALID);
        EXPECT(rm_traffic_due(nullptr, 7, 3, 0, &due) == RM_ERR_INVALID && rm_traffic_due(&s, 7, 3, 0, nullptr) == RM_ERR_INVALID);
    }
    // jitter: inside [base, base + jitter), the same answer twice, another seed another answer somewhere
    {
        const rm_traffic_schedule s = {1000, 999, 1000, 0};
        int differ = 0;
        for (int64_t k = 0; k < 200; ++k) {
            int64_t a = -1, b = -1, c = -1;
            EXPECT(rm_traffic_due(&s, 1, 5, k, &a) == 1 && rm_traffic_due(&s, 1, 5, k, &b) == 1 && rm_traffic_due(&s, 2, 5, k, &c) == 1);
            EXPECT(a == b && a >= 999 + k * 1000 && a < 999 + (k + 1) * 1000 && c >= 999 + k * 1000 && c < 999 + (k + 1) * 1000);
            differ += a != c;
        }
        EXPECT(differ > 150);
        const rm_traffic_schedule one = {1000, 0, 1, 0}; // jitter 1: j < 1
        EXPECT(rm_traffic_due(&one, 1, 5, 77, &due) == 1 && due == 77000);
    }
    // the largest period, phase, jitter and packet numbers: every intermediate stays inside 64 bits
    {
        const rm_traffic_schedule s = {P40, P40 - 1, P40, 0};
        const int64_t k_top = T62 / P40; // 2^22
        EXPECT(rm_traffic_due(&s, ~0ull, 2147483647, k_top, &due) == 1 && due >= T62 + P40 - 1 && due < T62 + 2 * P40 - 1);
        EXPECT(rm_traffic_due(&s, ~0ull, 2147483647, k_top + 1, &due) == RM_ERR_INVALID);
        const rm_traffic_schedule fast = {1, 0, 1, 0};
        EXPECT(rm_traffic_due(&fast, 0, 0, T62, &due) == 1 && due == T62);
        EXPECT(rm_traffic_due(&fast, 0, 0, T62 + 1, &due) == RM_ERR_INVALID);
        const rm_traffic_schedule s22 = {int64_t(1) << 22, 0, 0, 0};
        EXPECT(rm_traffic_due(&s22, 0, 0, P40, &due) == 1 && due == T62);
        const rm_traffic_schedule none = {0, 0, 0, 0};
        due = -7;
        EXPECT(rm_traffic_due(&none, 0, 0, 0, &due) == 0 && due == -7);
    }
    // bad records
    {
        const rm_traffic_schedule bad[] = {{0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}, {-1, 0, 0, 0}, {100, 100, 0, 0}, {100, -1, 0, 0}, {100, 0, 101, 0},
                                           {100, 0, -1, 0}, {P40 + 1, 0, 0, 0}, {100, 0, 0, -1}};
        for (const rm_traffic_schedule &b : bad) {
            EXPECT(rm_traffic_due(&b, 1, 1, 0, &due) == RM_ERR_INVALID);
            EXPECT(rm_traffic_validate(1, nullptr, 1, &b) == RM_ERR_INVALID);
        }
    }
    // ---- validate: 6 nodes
    {
        const int n_nodes = 6;
        std::vector<rm_traffic_schedule> whole;
        for (int j = 0; j < n_nodes; ++j) whole.push_back(j % 2 ? rm_traffic_schedule{0, 0, 0, 0} : rm_traffic_schedule{1000 + j, j, 1000 + j, 0});
        EXPECT(rm_traffic_validate(n_nodes, nullptr, n_nodes, whole.data()) == RM_OK);
        EXPECT(rm_traffic_validate(n_nodes, nullptr, n_nodes - 1, whole.data()) == RM_ERR_INVALID); // no list, another count
        EXPECT(rm_traffic_validate(n_nodes + 1, nullptr, n_nodes, whole.data()) == RM_ERR_INVALID);
        const std::vector<int32_t> nodes = {4, 0, 5, 4}; // (a node may repeat: the last entry wins)
        std::vector<rm_traffic_schedule> recs = {{100, 0, 0, 0}, {0, 0, 0, 0}, {P40, P40 - 1, P40, 0}, {7, 6, 7, 0}};
        EXPECT(rm_traffic_validate(n_nodes, nodes.data(), 4, recs.data()) == RM_OK);
        EXPECT(rm_traffic_validate(n_nodes, nodes.data(), 0, nullptr) == RM_OK); // an empty list
        EXPECT(rm_traffic_validate(n_nodes, nodes.data(), 4, nullptr) == RM_ERR_INVALID);
        EXPECT(rm_traffic_validate(n_nodes, nodes.data(), -1, recs.data()) == RM_ERR_INVALID);
        EXPECT(rm_traffic_validate(-1, nodes.data(), 0, nullptr) == RM_ERR_INVALID);
        const std::vector<int32_t> out_of_range = {4, 0, n_nodes, 4}, negative = {4, -1, 5, 4};
        EXPECT(rm_traffic_validate(n_nodes, out_of_range.data(), 4, recs.data()) == RM_ERR_INVALID);
        EXPECT(rm_traffic_validate(n_nodes, negative.data(), 4, recs.data()) == RM_ERR_INVALID);
        recs[3].jitter_us = 8; // the last record of the list is read as well
        EXPECT(rm_traffic_validate(n_nodes, nodes.data(), 4, recs.data()) == RM_ERR_INVALID);
    }
    std::printf("ok\n");
    return 0;
}
