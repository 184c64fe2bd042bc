// flood_mirror_test.cpp -- the C++ mirror with dissemination floods (radio-sim_amd/host/radiomedium.hpp: GpuRadioMedium::setFlooding /
// floodSeed / floodSources / floodAdvance / getFloodStatistics / floodTree).
// Input: <imin_us> <doublings> <max_intervals> <redundancy> <max_hops> <seed> ; <nodes> ; per node: <x> <y> ;
//        <seeds> <seed time> ; the seeds' indices ; <steps> <tick_us> <start_at_us> <hex length> <cap> ; per step: its time
// Step k, in tick mode, at its time t: the nodes floodSources gives at t + start_at_us each transmit a packet that starts then; the
// step's end evaluates them in one tick; floodAdvance moves the flood.
// Prints "refused <0|1>" (an advance before the feature is on), "sources <k> <count> <indices>" per step, per node "row <12 values>"
// and "tree <parent index or -1> <hop>", "totals <10 values>", and "off <0|1>".
// tests/test_gpu_flood_mirror.py compares with tests/flood_ref.py over ticks the oracle evaluates.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    rm_flood_params p = GpuRadioMedium::floodingDefaults();
    long long imin;
    unsigned long long seed;
    int n;
    in >> imin >> p.doublings >> p.max_intervals >> p.redundancy >> p.max_hops >> seed >> n;
    p.imin_us = imin;
    p.seed = seed;
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
        std::printf("refused %d\n", (!medium.floodAdvance() && !medium.lastError.empty()) ? 1 : 0);
        if (!medium.setFlooding(&p)) std::printf("error %s\n", medium.lastError.c_str());
        int ns, steps, hex, cap;
        long long t_seed, tick, start_at;
        std::vector<const Node *> seeds;
        in >> ns >> t_seed;
        for (int k = 0; k < ns; ++k) {
            int j;
            in >> j;
            seeds.push_back(nodes[size_t(j)]);
        }
        if (!medium.floodSeed(seeds, t_seed)) std::printf("error %s\n", medium.lastError.c_str());
        in >> steps >> tick >> start_at >> hex >> cap;
        medium.setTickMode(true);
        sim.recording = false;
        std::vector<std::unique_ptr<RadioPacket>> sent;
        for (int k = 0; k < steps; ++k) {
            long long t;
            in >> t;
            sim.setTime(t);
            int32_t count = 0;
            const std::vector<Node *> src = medium.floodSources(t + start_at, cap, &count);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            std::printf("sources %d %d", k, count);
            for (const Node *nd : src) std::printf(" %d", nd->index);
            std::printf("\n");
            sent.clear();
            for (Node *nd : src) {
                sent.emplace_back(new RadioPacket(nd, t + start_at, std::string(size_t(hex), '0')));
                medium.transmit(*sent.back());
            }
            sim.emulatorTimeStepDone(t + tick);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            // (a step without a frame evaluates nothing: the last result is an older tick's and must not be read again)
            if (!src.empty() && !medium.floodAdvance()) std::printf("error %s\n", medium.lastError.c_str());
        }
        rm_flood_totals tot{};
        std::vector<Node *> parents;
        std::vector<int32_t> hops;
        if (!medium.floodTree(&parents, &hops)) std::printf("error %s\n", medium.lastError.c_str());
        for (size_t j = 0; j < nodes.size(); ++j) {
            rm_flood_node r;
            if (!medium.getFloodStatistics(*nodes[j], &r, &tot)) std::printf("error %s\n", medium.lastError.c_str());
            std::printf("row %" PRId64 " %" PRId64 " %" PRId64 " %" PRIu64 " %d %d %d %d %u %u %u %u\n", r.first_us, r.start_us, r.fire_us, r.rssi_bits,
                        r.parent, r.hop, r.interval, r.c, r.sent, r.suppressed, r.heard, r.deferred);
            std::printf("tree %d %d\n", parents[j] ? parents[j]->index : -1, hops[j]);
        }
        std::printf("totals %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tot.covered,
                    tot.seeds, tot.sent, tot.suppressed, tot.heard, tot.deferred, tot.stray, tot.skipped_slots, tot.max_hop, tot.last_first_us);
        if (!medium.setFlooding(nullptr)) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("off %d\n", medium.getFlooding() ? 0 : 1);
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
