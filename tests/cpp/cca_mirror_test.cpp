// cca_mirror_test.cpp -- the C++ mirror's listen-before-talk call (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::transmitIfClear) over the SINR medium.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ; <rounds> ; per round: <start> <hex length> <cca time> <threshold> <senders> ;
//        per sender: <node index>
// Prints per round "flags <round> <one digit per sender>", then per call the medium made "tx <source>" or
// "rx <source> <destination> <bits of the rssi, hex> <deliver 0|1>"; tests/test_gpu_cca_mirror.py compares with the Python engine's.
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
    double sigma;
    long long seed;
    int n, rounds;
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
        in >> rounds;
        for (int r = 0; r < rounds; ++r) {
            long long start, cca;
            int hex, ns;
            double threshold;
            in >> start >> hex >> cca >> threshold >> ns;
            std::vector<Node *> senders;
            for (int k = 0; k < ns; ++k) {
                int j;
                in >> j;
                senders.push_back(nodes[size_t(j)]);
            }
            const size_t before = sim.calls.size();
            const std::vector<uint8_t> flags = medium.transmitIfClear(senders, start, hex, cca, threshold);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            std::printf("flags %d ", r);
            for (uint8_t f : flags) std::printf("%d", int(f));
            std::printf("\n");
            for (size_t k = before; k < sim.calls.size(); ++k) {
                const MediumCall &c = sim.calls[k];
                if (c.kind == MediumCall::TRANSMISSION_EVENTS) {
                    std::printf("tx %d\n", c.packet->getSource()->index);
                } else {
                    uint64_t bits;
                    std::memcpy(&bits, &c.rssi, 8);
                    std::printf("rx %d %d %016" PRIx64 " %d\n", c.packet->getSource()->index, c.destination->index, bits, c.doDeliver ? 1 : 0);
                }
            }
        }
        // a sample after the start is refused and says so
        const std::vector<uint8_t> none = medium.transmitIfClear({nodes[0]}, 100000, 10, 100001, -90.0);
        std::printf("refused %d %d\n", none.empty() ? 1 : 0, medium.lastError.empty() ? 0 : 1);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
