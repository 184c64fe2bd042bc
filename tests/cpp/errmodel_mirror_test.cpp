// errmodel_mirror_test.cpp -- the C++ mirror with a frame error model (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::setErrorModel / getErrorModel) over the SINR medium: its per-packet path and its CSMA-CA batch.
// Input: <sigma> <seed> <nodes> <sensitivity> <noise> <error model seed> ; per node: <x> <y> ;
//        <packets> ; per packet: <node index> <start> <hex length> ;
//        <hex length> <threshold> <max_backoffs> <min_be> <max_be> <csma seed> <ticks> ; per tick: <t_begin> <start> <cca time> <senders> ;
//        per sender: <node index>
// Prints "model <kind> <us per bit> <seed>" as getErrorModel gives it after the parameters were applied again, then per call the medium
// made "tx <source>" or "rx <source> <destination> <bits of the rssi, hex> <deliver 0|1>" -- the per-packet section, a line "batch", the
// batch's "pkt <status> <attempts> <tick> <pkt> <flags>" lines and its calls -- and "refused <0|1>" for a model on a medium without SINR;
// tests/test_gpu_errmodel_mirror.py compares with the oracle and tests/errmodel_ref.py.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

static void print_calls(const Simulator &sim, size_t before)
{
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

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    double sigma, sens, noise;
    long long seed, em_seed;
    int n;
    in >> sigma >> seed >> n >> sens >> noise >> em_seed;
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
        medium.setSinr(true);
        if (!medium.setErrorModel(RM_EM_OQPSK_250K, 4.0, uint64_t(em_seed))) std::printf("error %s\n", medium.lastError.c_str());
        // the parameters change after the model was set: the medium keeps its model
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.params().ld_sensitivity_dbm = sens;
        medium.params().ld_noise_dbm = noise;
        medium.params().ld_capture_db = -INFINITY;
        medium.apply();
        const rm_error_model e = medium.getErrorModel();
        std::printf("model %d %.17g %llu\n", e.kind, e.us_per_bit, (unsigned long long)e.seed);
        sim.setRadioMedium(&medium);
        int packets;
        in >> packets;
        std::vector<std::unique_ptr<RadioPacket>> sent;
        for (int k = 0; k < packets; ++k) {
            int src, hex;
            long long start;
            in >> src >> start >> hex;
            const size_t before = sim.calls.size();
            sent.emplace_back(new RadioPacket(nodes[size_t(src)], start, std::string(size_t(hex), '0')));
            medium.transmit(*sent.back());
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            print_calls(sim, before);
        }
        std::printf("batch\n");
        rm_csma_params p;
        rm_csma_defaults(&p);
        int hex, nt;
        double threshold;
        long long cseed;
        in >> hex >> threshold >> p.max_backoffs >> p.min_be >> p.max_be >> cseed >> nt;
        p.seed = uint64_t(cseed);
        std::vector<std::vector<Node *>> senders(static_cast<size_t>(nt));
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
        const std::vector<LogDistanceRadioMedium::CsmaOutcome> out = medium.transmitCsmaBatch(senders, t_begin, start, hex, cca, threshold, p);
        if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        for (const LogDistanceRadioMedium::CsmaOutcome &o : out)
            std::printf("pkt %d %d %d %d %d\n", int(o.status), int(o.attempts), o.tick, o.pkt, int(o.flags));
        print_calls(sim, before);
        // a medium without the SINR extension refuses the model and says so
        LogDistanceRadioMedium plain;
        std::printf("refused %d\n", (!plain.setErrorModel(RM_EM_OQPSK_250K) && !plain.lastError.empty() && plain.getErrorModel().kind == RM_EM_NONE) ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
