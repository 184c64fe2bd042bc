// nbtable_mirror_test.cpp -- the C++ mirror with neighbour tables (radio-sim_amd/host/radiomedium.hpp: GpuRadioMedium::setNeighbourTable /
// updateNeighbours / expireNeighbours / getNeighbourTableStatistics, over setLinkWatch / watchLinks / getLinkStatistics).
// Input: <admit_rssi_dbm> <timeout_us> <min_heard> <evict_cost> <require_delivered> ; <K> ; <nodes> ; per node: <x> <y> ;
//        <tick_us> <start_at_us> <hex length> ; <ops> ; per op one of
//          tick <time> <n> <the senders' indices>          in tick mode: every sender transmits a packet that starts at time + start_at_us
//          update <time> <n pins: 0 or nodes> <pins>       updateNeighbours over the last tick (-1: no pin)
//          expire <time> <n pins> <pins>
//          watch <node> <n> <peers>                        watchLinks (-1: an empty slot)
// Prints "refused <0|1>" (an update before the feature is on), per node "row <5 counters>", "peers <K indices or -1>" and per slot
// "entry <6 values>", "totals <7 values>", and "off <0|1>".
// tests/test_gpu_nbtable_mirror.py compares with tests/nbtable_ref.py over ticks the oracle evaluates.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>
#include <string>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    rm_nbtable_params p = GpuRadioMedium::neighbourTableDefaults();
    long long timeout;
    int K, n;
    in >> p.admit_rssi_dbm >> timeout >> p.min_heard >> p.evict_cost >> p.require_delivered >> K >> n;
    p.timeout_us = timeout;
    Simulator sim(1);
    std::vector<Node *> nodes;
    for (int i = 0; i < n; ++i) {
        double x, y;
        in >> x >> y;
        Node *nd = sim.addNode(std::to_string(i + 1));
        nd->getPosition().set(x, y, 0.0);
        nodes.push_back(nd);
    }
    auto pins = [&](std::vector<const Node *> &out) {
        int m;
        in >> m;
        for (int k = 0; k < m; ++k) {
            int j;
            in >> j;
            out.push_back(j >= 0 ? nodes[size_t(j)] : nullptr);
        }
    };
    try {
        UDGMRadioMedium medium;
        sim.setRadioMedium(&medium);
        std::printf("refused %d\n", (!medium.updateNeighbours(0) && !medium.lastError.empty()) ? 1 : 0);
        if (!medium.setLinkWatch(K)) std::printf("error %s\n", medium.lastError.c_str());
        if (!medium.setNeighbourTable(&p)) std::printf("error %s\n", medium.lastError.c_str());
        long long tick, start_at;
        int hex, ops;
        in >> tick >> start_at >> hex >> ops;
        medium.setTickMode(true);
        sim.recording = false;
        std::vector<std::unique_ptr<RadioPacket>> sent;
        for (int o = 0; o < ops; ++o) {
            std::string op;
            long long t;
            in >> op >> t;
            if (op == "tick") {
                int m;
                in >> m;
                sim.setTime(t);
                sent.clear();
                for (int k = 0; k < m; ++k) {
                    int j;
                    in >> j;
                    sent.emplace_back(new RadioPacket(nodes[size_t(j)], t + start_at, std::string(size_t(hex), '0')));
                    medium.transmit(*sent.back());
                }
                sim.emulatorTimeStepDone(t + tick);
                if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            } else if (op == "update" || op == "expire") {
                std::vector<const Node *> pinned;
                pins(pinned);
                if (!(op == "update" ? medium.updateNeighbours(t, pinned) : medium.expireNeighbours(t, pinned))) std::printf("error %s\n", medium.lastError.c_str());
            } else if (op == "watch") {
                std::vector<const Node *> peers;
                pins(peers);
                if (!medium.watchLinks(*nodes[size_t(t)], peers)) std::printf("error %s\n", medium.lastError.c_str());
            } else {
                return 2;
            }
        }
        rm_nbtable_totals tot{};
        for (size_t j = 0; j < nodes.size(); ++j) {
            rm_nbtable_node r;
            std::vector<Node *> peers;
            if (!medium.getNeighbourTableStatistics(*nodes[j], &r, &tot, &peers)) std::printf("error %s\n", medium.lastError.c_str());
            std::printf("row %u %u %u %u %u\npeers", r.admitted, r.evicted_stale, r.evicted_poor, r.refused, r.expired);
            for (const Node *nd : peers) std::printf(" %d", nd ? nd->index : -1);
            std::printf("\n");
            for (const rm_link_stats &e : medium.getLinkStatistics(*nodes[j]))
                std::printf("entry %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", e.heard, e.delivered, e.rssi_q8_sum, e.sinr_q8_sum,
                            e.first_start_us, e.last_start_us);
        }
        std::printf("totals %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot.updates, tot.skipped_slots, tot.admitted,
                    tot.evicted_stale, tot.evicted_poor, tot.refused, tot.expired);
        if (!medium.setNeighbourTable(nullptr)) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("off %d\n", medium.getNeighbourTable() ? 0 : 1);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
