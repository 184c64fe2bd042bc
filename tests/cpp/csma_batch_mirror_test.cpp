// csma_batch_mirror_test.cpp -- the C++ mirror's CSMA-CA calls (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::csmaSchedule and ::transmitCsmaBatch) over the SINR medium.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ; <batches> ; per batch: <hex length> <threshold> <max_backoffs> <min_be> <max_be>
//        <csma seed> <ticks> ; per tick: <t_begin> <start> <cca time> <senders> ; per sender: <node index>
// Prints per batch "n_exp <batch> <one per tick>", per packet "pkt <batch> <status> <attempts> <tick> <pkt> <flags>", then per call the
// medium made for the batch "tx <source>" or "rx <source> <destination> <bits of the rssi, hex> <deliver 0|1>";
// tests/test_gpu_csma_mirror.py compares with the oracle's chain.
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
        rm_csma_params p;
        rm_csma_defaults(&p);
        for (int r = 0; r < batches; ++r) {
            int hex, nt;
            double threshold;
            long long cseed;
            in >> hex >> threshold >> p.max_backoffs >> p.min_be >> p.max_be >> cseed >> nt;
            p.seed = uint64_t(cseed);
            std::vector<std::vector<Node *>> senders;
            senders.resize(size_t(nt));
            std::vector<int64_t> t_begin(size_t(nt), 0), start(size_t(nt), 0), cca(size_t(nt), 0);
            std::vector<int32_t> n_src;
            for (int b = 0; b < nt; ++b) {
                long long tb, ts, tc;
                int ns;
                in >> tb >> ts >> tc >> ns;
                t_begin[size_t(b)] = tb, start[size_t(b)] = ts, cca[size_t(b)] = tc;
                n_src.push_back(ns);
                for (int k = 0; k < ns; ++k) {
                    int j;
                    in >> j;
                    senders[size_t(b)].push_back(j >= 0 ? nodes[size_t(j)] : nullptr);
                }
            }
            LogDistanceRadioMedium::CsmaSchedule sched;
            if (!medium.csmaSchedule(p, n_src, cca, sched)) std::printf("error %s\n", medium.lastError.c_str());
            std::printf("n_exp %d", r);
            for (int32_t v : sched.n_exp) std::printf(" %d", v);
            std::printf("\n");
            const size_t before = sim.calls.size();
            const std::vector<LogDistanceRadioMedium::CsmaOutcome> out = medium.transmitCsmaBatch(senders, t_begin, start, hex, cca, threshold, p);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            for (const LogDistanceRadioMedium::CsmaOutcome &o : out)
                std::printf("pkt %d %d %d %d %d %d\n", r, int(o.status), int(o.attempts), o.tick, o.pkt, int(o.flags));
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
        // parameters out of range are refused and say so; so are lists of different lengths
        p.max_backoffs = 6;
        const std::vector<LogDistanceRadioMedium::CsmaOutcome> none = medium.transmitCsmaBatch({{nodes[0]}}, {1000000}, {1000000}, 10, {1000000}, -90.0, p);
        std::printf("refused %d %d\n", none.empty() ? 1 : 0, medium.lastError.empty() ? 0 : 1);
        p.max_backoffs = 2;
        const std::vector<LogDistanceRadioMedium::CsmaOutcome> odd = medium.transmitCsmaBatch({{nodes[0]}, {nodes[1]}}, {1000000}, {1000000}, 10, {1000000}, -90.0, p);
        std::printf("refused %d %d\n", odd.empty() ? 1 : 0, medium.lastError.empty() ? 0 : 1);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
