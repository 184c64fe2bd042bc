// energy_mirror_test.cpp -- the C++ mirror's clear-channel assessment (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::getChannelEnergy / isChannelClear) after a few packets have been handed to the SINR medium.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ; <packets> ; per packet: <source index> <start> <hex length> ;
//        <time> <threshold> <queries> ; per query: <node index>
// Prints per query "energy <node> <bits of the double, hex> <clear 0|1>"; tests/test_gpu_energy_mirror.py compares the bits with
// the Python engine's.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    double sigma, threshold;
    long long seed, time_us;
    int n, np, nq;
    in >> sigma >> seed >> n;
    Simulator sim(1);
    std::vector<Node *> nodes;
    for (int i = 0; i < n; ++i) {
        double x, y;
        in >> x >> y;
        Node *nd = sim.addNode(std::to_string(i + 1));
        nd->getPosition().set(x, y, 0.0);
        nodes.push_back(nd);
    }
    try {
        LogDistanceRadioMedium medium;
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.setSinr(true);
        sim.setRadioMedium(&medium);
        in >> np;
        std::vector<std::unique_ptr<RadioPacket>> packets;
        for (int p = 0; p < np; ++p) {
            int src, hex;
            long long start;
            in >> src >> start >> hex;
            packets.emplace_back(new RadioPacket(nodes[size_t(src)], start, std::string(size_t(hex), '0')));
            medium.transmit(*packets.back());
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        }
        in >> time_us >> threshold >> nq;
        for (int q = 0; q < nq; ++q) {
            int j;
            in >> j;
            const double e = medium.getChannelEnergy(*nodes[size_t(j)], time_us);
            const bool clear = medium.isChannelClear(*nodes[size_t(j)], time_us, threshold);
            uint64_t bits;
            std::memcpy(&bits, &e, 8);
            std::printf("energy %d %016" PRIx64 " %d\n", j, bits, clear ? 1 : 0);
        }
        if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
