// cca_batch_mirror_test.cpp -- the C++ mirror's listen-before-talk call across a batch of ticks (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::transmitIfClearBatch) over the SINR medium.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ; <batches> ; per batch: <hex length> <threshold> <ticks> ;
//        per tick: <t_begin> <start> <cca time> <senders> ; per sender: <node index>
// Prints per batch and tick "flags <batch> <tick> <one digit per sender>", then per call the medium made for the batch "tx <source>" or
// "rx <source> <destination> <bits of the rssi, hex> <deliver 0|1>"; tests/test_gpu_cca_batch_mirror.py compares with the oracle's chain.
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
    int n, batches;
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
        in >> batches;
        for (int r = 0; r < batches; ++r) {
            int hex, nt;
            double threshold;
            in >> hex >> threshold >> nt;
            std::vector<std::vector<Node *>> senders;
            senders.resize(size_t(nt));
            std::vector<int64_t> t_begin(size_t(nt), 0), start(size_t(nt), 0), cca(size_t(nt), 0);
            for (int b = 0; b < nt; ++b) {
                long long tb, ts, tc;
                int ns;
                in >> tb >> ts >> tc >> ns;
                t_begin[size_t(b)] = tb, start[size_t(b)] = ts, cca[size_t(b)] = tc;
                for (int k = 0; k < ns; ++k) {
                    int j;
                    in >> j;
                    senders[size_t(b)].push_back(j >= 0 ? nodes[size_t(j)] : nullptr);
                }
            }
            const size_t before = sim.calls.size();
            const std::vector<std::vector<uint8_t>> flags = medium.transmitIfClearBatch(senders, t_begin, start, hex, cca, threshold);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            for (size_t b = 0; b < flags.size(); ++b) {
                std::printf("flags %d %d ", r, int(b));
                for (uint8_t f : flags[b]) std::printf("%d", int(f));
                std::printf("\n");
            }
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
        // a sample after its tick's start is refused and says so; so are lists of different lengths
        const std::vector<std::vector<uint8_t>> none = medium.transmitIfClearBatch({{nodes[0]}}, {1000000}, {1000000}, 10, {1000001}, -90.0);
        std::printf("refused %d %d\n", none.empty() ? 1 : 0, medium.lastError.empty() ? 0 : 1);
        const std::vector<std::vector<uint8_t>> odd = medium.transmitIfClearBatch({{nodes[0]}, {nodes[1]}}, {1000000}, {1000000}, 10, {1000000}, -90.0);
        std::printf("refused %d %d\n", odd.empty() ? 1 : 0, medium.lastError.empty() ? 0 : 1);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
