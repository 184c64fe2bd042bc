// traffic_mirror_test.cpp -- the C++ mirror with traffic schedules (radio-sim_amd/host/radiomedium.hpp:
// GpuRadioMedium::setTrafficSchedule / generateTraffic / clearTrafficSchedules).
// Input: <seed> <cap> <nodes> ; per node: <x> <y> ;
//        <schedules> ; per schedule: <node index> <period> <phase> <jitter> ;
//        <windows> ; per window: <win_lo> <win_hi> ;
//        <more nodes> ; per node: <x> <y>
// Prints "enabled <0|1>" as the medium says after the parameters were applied again; "generate" and, per window, "window <b>" followed
// by the indices of its nodes; "totals <packets> <coalesced> <truncated>"; then the further nodes join the simulation -- the engine
// drops its table with the node table of another size, the mirror sets its schedules again -- and the same once more behind
// "grown <nodes>"; then "cleared <enabled 0|1>" and "refused <0|1>": whether a generate without schedules is refused.
// tests/test_gpu_traffic_mirror.py compares with tests/traffic_ref.py.
#include <cinttypes>
#include <cstdio>
#include <fstream>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

static void generate(UDGMRadioMedium &medium, uint64_t seed, const std::vector<int64_t> &lo, const std::vector<int64_t> &hi, int cap)
{
    std::vector<std::vector<Node *>> sources;
    rm_traffic_totals tot{};
    if (!medium.generateTraffic(seed, lo, hi, cap, sources, &tot)) {
        std::printf("error %s\n", medium.lastError.c_str());
        return;
    }
    for (size_t b = 0; b < sources.size(); ++b) {
        std::printf("window %zu", b);
        for (const Node *nd : sources[b]) std::printf(" %d", nd->index);
        std::printf("\n");
    }
    std::printf("totals %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot.packets, tot.coalesced, tot.truncated);
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    unsigned long long seed;
    int cap, n;
    in >> seed >> cap >> n;
    Simulator sim(1);
    std::vector<Node *> nodes;
    auto add_nodes = [&](int count) {
        for (int i = 0; i < count; ++i) {
            double x, y;
            in >> x >> y;
            Node *nd = sim.addNode(std::to_string(nodes.size() + 1));
            nd->getPosition().set(x, y, 0.0);
            nodes.push_back(nd);
        }
    };
    add_nodes(n);
    try {
        UDGMRadioMedium medium;
        sim.setRadioMedium(&medium);
        int ns;
        in >> ns;
        for (int k = 0; k < ns; ++k) {
            int i;
            long long period, phase, jitter;
            in >> i >> period >> phase >> jitter;
            if (!medium.setTrafficSchedule(*nodes[size_t(i)], period, phase, jitter)) std::printf("error %s\n", medium.lastError.c_str());
        }
        // the parameters change after the schedules were set: the medium keeps them
        medium.setTransmissionRange(40.0);
        std::printf("enabled %d\n", medium.getTrafficEnabled() ? 1 : 0);
        int nw;
        in >> nw;
        std::vector<int64_t> lo, hi;
        for (int b = 0; b < nw; ++b) {
            long long a, z;
            in >> a >> z;
            lo.push_back(a);
            hi.push_back(z);
        }
        std::printf("generate\n");
        generate(medium, seed, lo, hi, cap);
        int more;
        in >> more;
        add_nodes(more);
        std::printf("grown %zu\n", nodes.size());
        generate(medium, seed, lo, hi, cap);
        // a bad record is refused and changes nothing
        std::printf("bad %d\n", medium.setTrafficSchedule(*nodes[0], 10, 10, 0) ? 1 : 0);
        if (!medium.clearTrafficSchedules()) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("cleared %d\n", medium.getTrafficEnabled() ? 1 : 0);
        std::vector<std::vector<Node *>> sources;
        std::printf("refused %d\n", medium.generateTraffic(seed, lo, hi, cap, sources) ? 0 : 1);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
