// linkstats_mirror_test.cpp -- the C++ mirror with watched-link statistics (radio-sim_amd/host/radiomedium.hpp:
// GpuRadioMedium::setLinkWatch / watchLinks / getLinkStatistics) over the SINR medium: its tick mode and its per-packet path.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ;
//        <K> <rows> ; per row: <node index> <peers of the row> <that many peer indices, -1: an empty slot> ;
//        <step time> <tick packets> ; per packet: <node index> <start> <hex length> ;
//        <packets> ; per packet: <node index> <start> <hex length>
// Prints "enabled <K>" as the medium says after the parameters were applied again, a line "tick" and the calls of the tick-mode
// section -- "tx <source>" or "rx <source> <destination> <bits of the rssi, hex> <deliver 0|1>" --, a line "packets" and the calls of the
// per-packet section, then "entry <node> <slot> <heard> <delivered> <rssi_q8_sum> <sinr_q8_sum> <first_start_us> <last_start_us>" for
// every entry with heard > 0 through getLinkStatistics(node), "totals <counted> <skipped>", and "same <0|1>": whether all entries and
// the totals equal rm_linkstats_read over the whole table and the peer rows equal what was set; tests/test_gpu_linkstats_mirror.py
// compares with the oracle and tests/linkstats_ref.py.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

struct Medium : LogDistanceRadioMedium {
    rm_context *context() { return ctx_; }
};

static size_t print_calls(const Simulator &sim, size_t before)
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
    return sim.calls.size();
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    double sigma;
    long long seed;
    int n;
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
        Medium medium;
        medium.setSinr(true);
        sim.setRadioMedium(&medium);
        int K, nr;
        in >> K >> nr;
        if (!medium.setLinkWatch(K)) std::printf("error %s\n", medium.lastError.c_str());
        std::vector<int32_t> set(size_t(n) * size_t(K), -1);
        for (int r = 0; r < nr; ++r) {
            int i, np;
            in >> i >> np;
            std::vector<const Node *> peers;
            for (int k = 0; k < np; ++k) {
                int p;
                in >> p;
                peers.push_back(p >= 0 ? nodes[size_t(p)] : nullptr);
                set[size_t(i) * size_t(K) + size_t(k)] = p;
            }
            if (!medium.watchLinks(*nodes[size_t(i)], peers)) std::printf("error %s\n", medium.lastError.c_str());
        }
        // the parameters change after the rows were set: the medium keeps them
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.apply();
        std::printf("enabled %d\n", medium.getLinkWatch());
        std::vector<std::unique_ptr<RadioPacket>> sent;
        auto send = [&]() {
            int src, hex;
            long long start;
            in >> src >> start >> hex;
            sent.emplace_back(new RadioPacket(nodes[size_t(src)], start, std::string(size_t(hex), '0')));
            medium.transmit(*sent.back());
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        };
        std::printf("tick\n");
        long long step;
        int np;
        in >> step >> np;
        size_t printed = sim.calls.size();
        medium.setTickMode(true);
        for (int k = 0; k < np; ++k) send();
        sim.emulatorTimeStepDone(step);
        if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        printed = print_calls(sim, printed);
        std::printf("packets\n");
        medium.setTickMode(false);
        in >> np;
        for (int k = 0; k < np; ++k) {
            send();
            printed = print_calls(sim, printed);
        }
        std::vector<rm_link_stats> abi(size_t(n) * size_t(K));
        std::vector<int32_t> abi_peers(size_t(n) * size_t(K), -7);
        rm_stats_totals abi_tot = {0, 0}, tot = {0, 0};
        if (rm_linkstats_read(medium.context(), nullptr, n, abi.data(), &abi_tot) != RM_OK) std::printf("error %s\n", rm_last_error());
        if (rm_linkstats_peers_get(medium.context(), nullptr, n, abi_peers.data()) != RM_OK) std::printf("error %s\n", rm_last_error());
        bool same = abi_peers == set;
        for (int i = 0; i < n; ++i) {
            const std::vector<rm_link_stats> e = medium.getLinkStatistics(*nodes[size_t(i)], &tot);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            same = same && e.size() == size_t(K) && std::memcmp(e.data(), abi.data() + size_t(i) * size_t(K), size_t(K) * sizeof(rm_link_stats)) == 0;
            for (size_t k = 0; k < e.size(); ++k)
                if (e[k].heard)
                    std::printf("entry %d %zu %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", i, k, e[k].heard, e[k].delivered,
                                e[k].rssi_q8_sum, e[k].sinr_q8_sum, e[k].first_start_us, e[k].last_start_us);
        }
        same = same && tot.ticks_counted == abi_tot.ticks_counted && tot.ticks_skipped == abi_tot.ticks_skipped;
        std::printf("totals %" PRIu64 " %" PRIu64 "\n", tot.ticks_counted, tot.ticks_skipped);
        std::printf("same %d\n", same ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
