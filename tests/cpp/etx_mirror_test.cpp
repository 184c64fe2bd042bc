// etx_mirror_test.cpp -- the C++ mirror with the measured-route query (radio-sim_amd/host/radiomedium.hpp:
// GpuRadioMedium::measuredRoutes; extension E21) over the SINR medium's watched links, and over a caller's table.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ; <K> <step> <hex length> <ticks> ; per tick: <sources> and that many node
//        indices ; <roots> and that many node indices ; <band K> and per node and slot of the band table: <peer> <heard> <delivered>
// The medium watches every node's K strongest transmitters (watchStrongest), the ticks run in tick mode, then it prints
// "entry <node> <slot> <peer> <heard> <delivered>" for every watched slot as rm_linkstats_peers_get / rm_linkstats_read give them, and
// for the runs  0: defaults  1: RM_ETX_BOTH with run 0's parents as current ones  2: defaults with hysteresis 0 and run 1's parents
// 3: the band table under cap 2000  4: the band table, RM_ETX_BOTH, run 3's parents
// "totals <run> <reached> <roots> <kept> <switched> <lost> <max_cost>" and per node "row <run> <node> <cost> <parent or -1> <slot>
// <link cost> <children>"; "refused <0|1>" for a cap of 127.  tests/test_gpu_etx_mirror.py compares with tests/etx_ref.py.
#include <cinttypes>
#include <cstdio>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

struct Medium : LogDistanceRadioMedium {
    rm_context *context() { return ctx_; }
};

static std::vector<const Node *> print_tree(Medium &medium, int run, const GpuRadioMedium::MeasuredRouteTree &tree)
{
    if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
    const rm_etx_totals &t = tree.totals;
    std::printf("totals %d %d %d %d %d %d %" PRIu64 "\n", run, t.reached, t.roots, t.kept, t.switched, t.lost, t.max_cost);
    std::vector<const Node *> parents;
    for (size_t j = 0; j < tree.rows.size(); ++j) {
        const auto &r = tree.rows[j];
        std::printf("row %d %zu %" PRIu64 " %d %d %u %d\n", run, j, r.cost, r.parent ? r.parent->index : -1, r.slot, r.linkCost, r.children);
        parents.push_back(r.parent);
    }
    return parents;
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
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.setSinr(true);
        sim.setRadioMedium(&medium);
        int K, hex, ticks;
        long long step;
        in >> K >> step >> hex >> ticks;
        if (!medium.watchStrongest(K)) std::printf("error %s\n", medium.lastError.c_str());
        medium.setTickMode(true);
        std::vector<std::unique_ptr<RadioPacket>> sent;
        for (int t = 0; t < ticks; ++t) {
            int ns;
            in >> ns;
            for (int k = 0; k < ns; ++k) {
                int src;
                in >> src;
                sent.emplace_back(new RadioPacket(nodes[size_t(src)], step * t, std::string(size_t(hex), '0')));
                medium.transmit(*sent.back());
            }
            sim.emulatorTimeStepDone(step * (t + 1));
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        }
        std::vector<rm_link_stats> table(size_t(n) * size_t(K));
        std::vector<int32_t> peers(size_t(n) * size_t(K), -7);
        if (rm_linkstats_read(medium.context(), nullptr, n, table.data(), nullptr) != RM_OK) std::printf("error %s\n", rm_last_error());
        if (rm_linkstats_peers_get(medium.context(), nullptr, n, peers.data()) != RM_OK) std::printf("error %s\n", rm_last_error());
        for (size_t i = 0; i < peers.size(); ++i)
            if (peers[i] >= 0)
                std::printf("entry %zu %zu %d %" PRIu64 " %" PRIu64 "\n", i / size_t(K), i % size_t(K), peers[i], table[i].heard, table[i].delivered);
        int nr;
        in >> nr;
        std::vector<const Node *> roots;
        for (int k = 0; k < nr; ++k) {
            int j;
            in >> j;
            roots.push_back(nodes[size_t(j)]);
        }
        rm_etx_params p = GpuRadioMedium::measuredRouteDefaults();
        const auto first = print_tree(medium, 0, medium.measuredRoutes(p, roots));
        p.mode = RM_ETX_BOTH;
        const auto second = print_tree(medium, 1, medium.measuredRoutes(p, roots, first));
        p = GpuRadioMedium::measuredRouteDefaults();
        p.hysteresis = 0;
        print_tree(medium, 2, medium.measuredRoutes(p, roots, second));
        // a caller's table: the band
        int bandK;
        in >> bandK;
        std::vector<int32_t> bpeer(size_t(n) * size_t(bandK));
        std::vector<rm_link_stats> bstats(bpeer.size(), rm_link_stats{0, 0, 0, 0, INT64_MAX, INT64_MIN});
        for (size_t i = 0; i < bpeer.size(); ++i) in >> bpeer[i] >> bstats[i].heard >> bstats[i].delivered;
        const rm_etx_tables band{bpeer.data(), bstats.data(), bandK, 0};
        p = GpuRadioMedium::measuredRouteDefaults();
        p.max_link_cost = 2000;
        const auto third = print_tree(medium, 3, medium.measuredRoutes(p, {nodes[0]}, {}, &band));
        p.mode = RM_ETX_BOTH;
        print_tree(medium, 4, medium.measuredRoutes(p, {nodes[0]}, third, &band));
        p.max_link_cost = 127;
        std::printf("refused %d\n", medium.measuredRoutes(p, roots).rows.empty() && !medium.lastError.empty() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
