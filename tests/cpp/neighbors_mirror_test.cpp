// neighbors_mirror_test.cpp -- the C++ mirror with the neighbour query (radio-sim_amd/host/radiomedium.hpp:
// LogDistanceRadioMedium::neighbors / watchStrongest; extension E16).
// Input: <sigma> <seed> <K> <watch K> <nodes> ; per node: <x> <y> <txpower> <channel> <enabled 0|1> <rxprob> ;
//        <listed> ; that many node indices
// Prints, for direction 0 then 1, "row <direction> <node> <degree>" followed by "<peer>:<bits of the rssi, hex>" per listed link, for
// all nodes through neighbors(direction, K) and then "list <direction> <node> <degree> ..." for the listed ones; "watch <ok 0|1>
// <enabled K>" after watchStrongest(watch K); "peers <node> <watch K indices>" as rm_linkstats_peers_get has them; "kept <0|1>":
// whether the rows are the same after the parameters were applied again and a node joined the simulation (the engine drops its
// tables, the mirror sets the rows again).  tests/test_gpu_neighbors_mirror.py compares with the Python engine and the reference.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

struct Medium : LogDistanceRadioMedium {
    rm_context *context() { return ctx_; }
};

static void print_rows(const char *tag, int direction, const std::vector<LogDistanceRadioMedium::NeighborRow> &rows, const std::vector<int> &nodes)
{
    for (size_t e = 0; e < rows.size(); ++e) {
        std::printf("%s %d %d %d", tag, direction, nodes[e], rows[e].degree);
        for (size_t k = 0; k < rows[e].peers.size(); ++k) {
            uint64_t bits;
            std::memcpy(&bits, &rows[e].rssi[k], 8);
            std::printf(" %d:%016" PRIx64, rows[e].peers[k]->index, bits);
        }
        std::printf("\n");
    }
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    double sigma;
    long long seed;
    int K, WK, n;
    in >> sigma >> seed >> K >> WK >> n;
    Simulator sim(1);
    std::vector<Node *> nodes;
    std::vector<int> every;
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
        every.push_back(i);
    }
    int nl;
    in >> nl;
    std::vector<int> listed(static_cast<size_t>(nl));
    std::vector<const Node *> listed_nodes;
    for (int &j : listed) {
        in >> j;
        listed_nodes.push_back(nodes[size_t(j)]);
    }
    try {
        Medium medium;
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.apply();
        sim.setRadioMedium(&medium);
        for (int d = 0; d < 2; ++d) {
            const auto all = medium.neighbors(d, K);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            print_rows("row", d, all, every);
            const auto part = medium.neighbors(d, K, listed_nodes);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            print_rows("list", d, part, listed);
        }
        std::printf("refused %d\n", medium.neighbors(2, K).empty() && !medium.lastError.empty() ? 1 : 0);
        const bool ok = medium.watchStrongest(WK);
        if (!ok) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("watch %d %d\n", ok ? 1 : 0, medium.getLinkWatch());
        std::vector<int32_t> peers(size_t(n) * size_t(WK), -7);
        if (rm_linkstats_peers_get(medium.context(), nullptr, n, peers.data()) != RM_OK) std::printf("error %s\n", rm_last_error());
        for (int i = 0; i < n; ++i) {
            std::printf("peers %d", i);
            for (int k = 0; k < WK; ++k) std::printf(" %d", peers[size_t(i) * size_t(WK) + size_t(k)]);
            std::printf("\n");
        }
        // a far node joins: the engine's tables go with the node table of another size, the mirror sets the rows it read back
        Node *far = sim.addNode(std::to_string(n + 1));
        far->getPosition().set(1.0e6, 1.0e6, 0.0);
        const bool set_again = medium.watchLinks(*far, {}); // (the next watch call finds the feature off and restores it first)
        std::vector<int32_t> again(size_t(n + 1) * size_t(WK), -7);
        bool kept = set_again && rm_linkstats_peers_get(medium.context(), nullptr, n + 1, again.data()) == RM_OK;
        kept = kept && std::memcmp(again.data(), peers.data(), peers.size() * sizeof(int32_t)) == 0;
        for (int k = 0; k < WK; ++k) kept = kept && again[size_t(n) * size_t(WK) + size_t(k)] == -1;
        std::printf("kept %d\n", kept ? 1 : 0);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
