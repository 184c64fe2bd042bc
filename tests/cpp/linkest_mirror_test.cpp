// linkest_mirror_test.cpp -- the C++ mirror with the link estimator (radio-sim_amd/host/radiomedium.hpp: GpuRadioMedium::setLinkEstimator /
// foldLinkEstimator / getLinkEstimates, over setLinkWatch and setNeighbourTable, which fill the watch table from the frames heard).
// Input: <beacon_window> <data_window> <beacon_alpha_q8> <data_alpha_q8> <max_etx> ; <K> ; <nodes> ; per node: <x> <y> ;
//        <tick_us> <start_at_us> <hex length> ; <ops> ; per op one of
//          tick <time> <n> <the senders' indices>     in tick mode: every sender transmits a packet that starts at time + start_at_us
//          update <time> 0                            updateNeighbours over the last tick, no pins
//          watch <node> <n> <peers>                   watchLinks (-1: an empty slot)
//          fold 0                                     foldLinkEstimator
// Prints "refused <0|1>" (a fold before the feature is on), "on <K>", per node per slot "est <6 values>" and "peers <K indices or
// -1>", per node "state <6 values>", "totals <8 values>", "tables <0|1>" and "off <0|1>".
// tests/test_gpu_linkest_mirror.py compares with tests/linkest_ref.py fed the reference's watch table over ticks the oracle evaluates.
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
    rm_linkest_params p = GpuRadioMedium::linkEstimatorDefaults();
    int K, n;
    in >> p.beacon_window >> p.data_window >> p.beacon_alpha_q8 >> p.data_alpha_q8 >> p.max_etx >> K >> n;
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
        UDGMRadioMedium medium;
        sim.setRadioMedium(&medium);
        std::printf("refused %d\n", (!medium.foldLinkEstimator() && !medium.lastError.empty()) ? 1 : 0);
        rm_nbtable_params nb = GpuRadioMedium::neighbourTableDefaults();
        nb.timeout_us = 0;
        nb.evict_cost = 0;
        if (!medium.setLinkWatch(K)) std::printf("error %s\n", medium.lastError.c_str());
        if (!medium.setNeighbourTable(&nb)) std::printf("error %s\n", medium.lastError.c_str());
        if (!medium.setLinkEstimator(&p)) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("on %d\n", medium.getLinkEstimator());
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
            } else if (op == "update" || op == "watch") {
                int m;
                in >> m;
                std::vector<const Node *> list;
                for (int k = 0; k < m; ++k) {
                    int j;
                    in >> j;
                    list.push_back(j >= 0 ? nodes[size_t(j)] : nullptr);
                }
                if (!(op == "update" ? medium.updateNeighbours(t, list) : medium.watchLinks(*nodes[size_t(t)], list)))
                    std::printf("error %s\n", medium.lastError.c_str());
            } else if (op == "fold") {
                if (!medium.foldLinkEstimator()) std::printf("error %s\n", medium.lastError.c_str());
            } else {
                return 2;
            }
        }
        rm_linkest_totals tot{};
        for (size_t j = 0; j < nodes.size(); ++j) {
            std::vector<rm_linkest_entry> est;
            std::vector<Node *> peers;
            rm_linkest_node st{};
            if (!medium.getLinkEstimates(*nodes[j], &est, &st, &tot, &peers)) std::printf("error %s\n", medium.lastError.c_str());
            for (const rm_linkest_entry &e : est)
                std::printf("est %" PRIu64 " %" PRIu64 " %u %u %u %d\n", e.base_heard, e.base_delivered, e.etx, e.windows, e.data_windows, e.peer);
            std::printf("peers");
            for (const Node *nd : peers) std::printf(" %d", nd ? nd->index : -1);
            std::printf("\nstate %" PRIu64 " %" PRIu64 " %d %u %u %u\n", st.base_tx, st.base_ack, st.base_next, st.data_samples, st.data_unmatched, st.restarted);
        }
        std::printf("totals %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot.folds, tot.beacon_samples,
                    tot.data_samples, tot.data_unmatched, tot.restarted, tot.cleared, tot.estimates, tot.reserved);
        rm_etx_tables tb{};
        std::printf("tables %d\n", (medium.linkEstimateTables(&tb) && tb.peer && tb.stats && tb.K == K) ? 1 : 0);
        if (!medium.setLinkEstimator(nullptr)) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("off %d\n", medium.getLinkEstimator() ? 0 : 1);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
