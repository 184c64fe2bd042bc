// stats_mirror_test.cpp -- the C++ mirror with per-node traffic counters (radio-sim_amd/host/radiomedium.hpp:
// GpuRadioMedium::setStatistics / resetStatistics / getStatistics) over the SINR medium: its per-packet path and its CSMA-CA batch.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ;
//        <packets> ; per packet: <node index> <start> <hex length> ;
//        <hex length> <threshold> <max_backoffs> <min_be> <max_be> <csma seed> <ticks> ; per tick: <t_begin> <start> <cca time> <senders> ;
//        per sender: <node index>
// Prints "enabled <0|1>" as the medium says after the parameters were applied again, then the per-packet section's table -- a line
// "totals <ticks counted> <ticks skipped>" and per node with a non-zero counter "node <index> <the eight counters>" -- then "one <index>
// <the eight counters>" for the first sender through getStatistics(node), a line "batch", the batch's "pkt <status> <attempts> <tick>
// <pkt> <flags>" lines, the table after a reset and the batch, and "refused <0|1>" for a read on a medium that never enabled statistics;
// tests/test_gpu_stats_mirror.py compares with the oracle and tests/stats_ref.py.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

static void print_record(const char *tag, int index, const rm_node_stats &s)
{
    std::printf("%s %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tag, index, s.tx_frames,
                s.tx_failed, s.tx_air_us, s.tx_links_heard, s.tx_links_delivered, s.rx_heard, s.rx_delivered, s.rx_air_us);
}

static void print_table(GpuRadioMedium &medium)
{
    rm_stats_totals tot{};
    const std::vector<rm_node_stats> t = medium.getStatistics(&tot);
    if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
    std::printf("totals %" PRIu64 " %" PRIu64 "\n", tot.ticks_counted, tot.ticks_skipped);
    for (size_t i = 0; i < t.size(); ++i) {
        const rm_node_stats &s = t[i];
        if (s.tx_frames | s.tx_failed | s.tx_air_us | s.tx_links_heard | s.tx_links_delivered | s.rx_heard | s.rx_delivered | s.rx_air_us)
            print_record("node", int(i), s);
    }
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
        LogDistanceRadioMedium medium;
        medium.setSinr(true);
        if (!medium.setStatistics(true)) std::printf("error %s\n", medium.lastError.c_str());
        // the parameters change after statistics were switched on: the medium keeps counting
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.apply();
        std::printf("enabled %d\n", medium.getStatisticsEnabled() ? 1 : 0);
        sim.setRadioMedium(&medium);
        int packets;
        in >> packets;
        std::vector<std::unique_ptr<RadioPacket>> sent;
        int first_src = 0;
        for (int k = 0; k < packets; ++k) {
            int src, hex;
            long long start;
            in >> src >> start >> hex;
            if (k == 0) first_src = src;
            sent.emplace_back(new RadioPacket(nodes[size_t(src)], start, std::string(size_t(hex), '0')));
            medium.transmit(*sent.back());
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        }
        print_table(medium);
        print_record("one", first_src, medium.getStatistics(*nodes[size_t(first_src)]));
        if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("batch\n");
        if (!medium.resetStatistics()) std::printf("error %s\n", medium.lastError.c_str());
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
        const std::vector<LogDistanceRadioMedium::CsmaOutcome> out = medium.transmitCsmaBatch(senders, t_begin, start, hex, cca, threshold, p);
        if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        for (const LogDistanceRadioMedium::CsmaOutcome &o : out)
            std::printf("pkt %d %d %d %d %d\n", int(o.status), int(o.attempts), o.tick, o.pkt, int(o.flags));
        print_table(medium);
        // a medium that never switched statistics on has no table, and says so
        UDGMRadioMedium plain;
        const bool none = plain.getStatistics().empty() && !plain.lastError.empty() && !plain.getStatisticsEnabled();
        std::printf("refused %d\n", none ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
