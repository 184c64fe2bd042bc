// listen_mirror_test.cpp -- the C++ mirror with receiver listening schedules (radio-sim_amd/host/radiomedium.hpp:
// GpuRadioMedium::setListenSchedule / clearListenSchedules / getListenMissed) over the SINR medium: its tick mode and its per-packet path.
// Input: <sigma> <seed> <nodes> ; per node: <x> <y> ;
//        <schedules> ; per schedule: <node index> <period> <on> <phase> ;
//        <step time> <tick packets> ; per packet: <node index> <start> <hex length> ;
//        <packets> ; per packet: <node index> <start> <hex length> ;
//        <node index> <start> <hex length>   (one more packet, sent after clearListenSchedules)
// Prints "enabled <0|1>" as the medium says after the parameters were applied again, a line "tick" and the calls of the tick-mode
// section -- "tx <source>" or "rx <source> <destination> <bits of the rssi, hex> <deliver 0|1>" --, a line "packets" and the calls of the
// per-packet section, then "missed <node> <count>" for every node with a non-zero count through getListenMissed(node), "same <0|1>":
// whether those counts equal rm_listen_missed_read over the whole table, a line "cleared <enabled 0|1>" and the last packet's calls;
// tests/test_gpu_listen_mirror.py compares with the oracle and tests/listen_ref.py.
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
        int ns;
        in >> ns;
        for (int k = 0; k < ns; ++k) {
            int i;
            long long period, on, phase;
            in >> i >> period >> on >> phase;
            if (!medium.setListenSchedule(*nodes[size_t(i)], period, on, phase)) std::printf("error %s\n", medium.lastError.c_str());
        }
        // the parameters change after the schedules were set: the medium keeps them
        medium.params().ld_sigma_db = sigma;
        medium.params().ld_seed = uint64_t(seed);
        medium.apply();
        std::printf("enabled %d\n", medium.getListenEnabled() ? 1 : 0);
        std::vector<std::unique_ptr<RadioPacket>> sent;
        auto send = [&](bool report) {
            int src, hex;
            long long start;
            in >> src >> start >> hex;
            sent.emplace_back(new RadioPacket(nodes[size_t(src)], start, std::string(size_t(hex), '0')));
            medium.transmit(*sent.back());
            if (report && !medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        };
        std::printf("tick\n");
        long long step;
        int np;
        in >> step >> np;
        size_t printed = sim.calls.size();
        medium.setTickMode(true);
        for (int k = 0; k < np; ++k) send(true);
        sim.emulatorTimeStepDone(step);
        if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
        printed = print_calls(sim, printed);
        std::printf("packets\n");
        medium.setTickMode(false);
        in >> np;
        for (int k = 0; k < np; ++k) {
            send(true);
            printed = print_calls(sim, printed);
        }
        std::vector<uint64_t> abi(size_t(n), 0);
        if (rm_listen_missed_read(medium.context(), nullptr, n, abi.data()) != RM_OK) std::printf("error %s\n", rm_last_error());
        bool same = true;
        for (int i = 0; i < n; ++i) {
            const uint64_t m = medium.getListenMissed(*nodes[size_t(i)]);
            if (!medium.lastError.empty()) std::printf("error %s\n", medium.lastError.c_str());
            same = same && m == abi[size_t(i)];
            if (m) std::printf("missed %d %" PRIu64 "\n", i, m);
        }
        std::printf("same %d\n", same ? 1 : 0);
        if (!medium.clearListenSchedules()) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("cleared %d\n", medium.getListenEnabled() ? 1 : 0);
        send(true);
        print_calls(sim, printed);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    return 0;
}
