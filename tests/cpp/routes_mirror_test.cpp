// routes_mirror_test.cpp -- the C++ mirror with the route query (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::routes; extension E18).
// Input: <sigma> <seed> <sensitivity> <min rssi> <nodes> ; per node: <x> <y> <txpower> <channel> <enabled 0|1> <rxprob> ;
//        <roots> ; that many node indices
// Prints, for direction 0 then 1 and for the runs RM_EM_NONE, RM_EM_OQPSK_250K and RM_EM_OQPSK_250K with <min rssi> (4064 us
// frames, 4 us per bit, cap 1024), "totals <direction> <reached> <roots> <max_cost>" and per node
// "row <direction> <node> <cost> <parent index or -1> <bits of the rssi, hex> <link cost> <children>"; "refused <0|1>" for a cap
// of 127.  tests/test_gpu_routes_mirror.py compares with the Python engine and the reference.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <limits>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    double sigma, sens, min_rssi;
    long long seed;
    int n;
    in >> sigma >> seed >> sens >> min_rssi >> n;
    Simulator sim(1);
    std::vector<Node *> nodes;
    for (int i = 0; i < n; ++i) {
        double x, y, txpower, rxprob;
        int channel, enabled;
        in >> x >> y >> txpower >> channel >> enabled >> rxprob;
        Node *nd = sim.addNode(std::to_string(i + 1));
        nd->getPosition().set(x, y, 0.0);
        nd->getRadio().setTransmitPower(txpower);
        nd->getRadio().setWirelessChannel(channel);
        nd->getRadio().setEnabled(enabled != 0);
        nd->getRadio().setRxProbability(rxprob);
        nodes.push_back(nd);
    }
    int nr;
    in >> nr;
    std::vector<const Node *> roots;
    for (int k = 0; k < nr; ++k) {
        int j;
        in >> j;
        roots.push_back(nodes[size_t(j)]);
    }
    try {
        LogDistanceRadioMedium medium;
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.params().ld_sensitivity_dbm = sens;
        medium.apply();
        sim.setRadioMedium(&medium);
        const double ninf = -std::numeric_limits<double>::infinity();
        for (int d = 0; d < 2; ++d) {
            const rm_routes_params runs[3] = {LogDistanceRadioMedium::routeParams(d, RM_EM_NONE), LogDistanceRadioMedium::routeParams(d),
                                              LogDistanceRadioMedium::routeParams(d, RM_EM_OQPSK_250K, 4.0, 4064, min_rssi)};
            for (const rm_routes_params &p : runs) {
                const auto tree = medium.routes(p, roots);
                if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
                std::printf("totals %d %d %d %" PRIu64 "\n", d, tree.totals.reached, tree.totals.roots, tree.totals.max_cost);
                for (size_t j = 0; j < tree.rows.size(); ++j) {
                    uint64_t bits;
                    std::memcpy(&bits, &tree.rows[j].rssi, 8);
                    std::printf("row %d %zu %" PRIu64 " %d %016" PRIx64 " %u %d\n", d, j, tree.rows[j].cost,
                                tree.rows[j].parent ? tree.rows[j].parent->index : -1, bits, tree.rows[j].linkCost, tree.rows[j].children);
                }
            }
        }
        const rm_routes_params bad = LogDistanceRadioMedium::routeParams(0, RM_EM_OQPSK_250K, 4.0, 4064, ninf, 127);
        std::printf("refused %d\n", medium.routes(bad, roots).rows.empty() && !medium.lastError.empty() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
