// hops_mirror_test.cpp -- the C++ mirror with the hop query (radio-sim_amd/host/radiomedium.hpp: LogDistanceRadioMedium::hops;
// extension E17).
// Input: <sigma> <seed> <min rssi> <nodes> ; per node: <x> <y> <txpower> <channel> <enabled 0|1> <rxprob> ;
//        <roots> ; that many node indices
// Prints, for direction 0 then 1 and for the threshold -inf then <min rssi>, "totals <direction> <reached> <max_hop> <roots>" and
// per node "row <direction> <node> <hop> <parent index or -1> <bits of the rssi, hex> <children>"; "refused <0|1>" for an unknown
// direction.  tests/test_gpu_hops_mirror.py compares with the Python engine and the reference.
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
    double sigma, min_rssi;
    long long seed;
    int n;
    in >> sigma >> seed >> min_rssi >> n;
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
        medium.apply();
        sim.setRadioMedium(&medium);
        for (int d = 0; d < 2; ++d) {
            for (const double mr : {-std::numeric_limits<double>::infinity(), min_rssi}) {
                const auto tree = medium.hops(d, roots, mr);
                if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
                std::printf("totals %d %d %d %d\n", d, tree.totals.reached, tree.totals.max_hop, tree.totals.roots);
                for (size_t j = 0; j < tree.rows.size(); ++j) {
                    uint64_t bits;
                    std::memcpy(&bits, &tree.rows[j].rssi, 8);
                    std::printf("row %d %zu %d %d %016" PRIx64 " %d\n", d, j, tree.rows[j].hop, tree.rows[j].parent ? tree.rows[j].parent->index : -1, bits,
                                tree.rows[j].children);
                }
            }
        }
        std::printf("refused %d\n", medium.hops(2, roots).rows.empty() && !medium.lastError.empty() ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
