// fwd_mirror_test.cpp -- the C++ mirror with forwarding queues (radio-sim_amd/host/radiomedium.hpp: GpuRadioMedium::setForwarding /
// setNextHops / forwardInject / forwardSources / forwardAdvance / getForwardStatistics).
// Input: <medium: udgm|null> <queue_slots> <max_retries> <min_be> <max_be> <max_hops> <backoff_unit_us> <seed> ;
//        <nodes> ; per node: <x> <y> ; per node: <parent index or -1> ; <sinks> ; the sinks' indices ;
//        <injected> <inject time> ; the injected nodes' indices ;
//        <steps> <tick_us> <start_at_us> <hex length> <cap>
// Step k, in tick mode, at t = k * tick_us: the nodes forwardSources gives at t + start_at_us each transmit a packet that starts
// then; the step's end evaluates them in one tick; forwardAdvance moves the queues.  The run ends early once nothing is in flight.
// Prints "refused <0|1>" (an advance before the feature is on), "sources <k> <count> <indices>" per step, then "steps <k>", per node
// "row <17 values>" and "queue <node> <origin> <hops> <birth> <enq>" per queued packet, "totals <11 values>", and "off <0|1>".
// tests/test_gpu_fwd_mirror.py compares with tests/fwd_ref.py over ticks the oracle evaluates.
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <memory>

#include "../../radio-sim_amd/host/radiomedium.hpp"

using namespace emul8;

static int run(GpuRadioMedium &medium, Simulator &sim, std::ifstream &in, const std::vector<Node *> &nodes, const rm_fwd_params &p)
{
    const size_t n = nodes.size();
    std::printf("refused %d\n", (!medium.forwardAdvance() && !medium.lastError.empty()) ? 1 : 0);
    if (!medium.setForwarding(&p)) std::printf("error %s\n", medium.lastError.c_str());
    std::vector<const Node *> parents(n, nullptr), sinks, injected;
    for (size_t j = 0; j < n; ++j) {
        int par;
        in >> par;
        parents[j] = par >= 0 ? nodes[size_t(par)] : nullptr;
    }
    int ns, ni;
    long long t_inject;
    in >> ns;
    for (int k = 0; k < ns; ++k) {
        int j;
        in >> j;
        sinks.push_back(nodes[size_t(j)]);
    }
    if (!medium.setNextHops(parents, sinks, 0)) std::printf("error %s\n", medium.lastError.c_str());
    in >> ni >> t_inject;
    for (int k = 0; k < ni; ++k) {
        int j;
        in >> j;
        injected.push_back(nodes[size_t(j)]);
    }
    if (!medium.forwardInject(injected, t_inject)) std::printf("error %s\n", medium.lastError.c_str());
    int steps, hex, cap;
    long long tick, start_at;
    in >> steps >> tick >> start_at >> hex >> cap;
    medium.setTickMode(true);
    sim.recording = false;
    std::vector<std::unique_ptr<RadioPacket>> sent;
    int k = 0;
    while (k < steps) {
        const int64_t t = int64_t(k) * tick;
        sim.setTime(t);
        int32_t count = 0;
        const std::vector<Node *> src = medium.forwardSources(t + start_at, cap, &count);
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
        if (!src.empty() && !medium.forwardAdvance()) std::printf("error %s\n", medium.lastError.c_str());
        ++k;
        rm_fwd_node row;
        rm_fwd_totals tot;
        if (!medium.getForwardStatistics(*nodes[0], &row, &tot)) std::printf("error %s\n", medium.lastError.c_str());
        if (tot.in_flight == 0) break;
    }
    std::printf("steps %d\n", k);
    rm_fwd_totals tot{};
    for (size_t j = 0; j < n; ++j) {
        rm_fwd_node r;
        std::vector<rm_fwd_packet> q;
        if (!medium.getForwardStatistics(*nodes[j], &r, &tot, &q)) std::printf("error %s\n", medium.lastError.c_str());
        std::printf("row %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
                    " %" PRIu64 " %" PRId64 " %d %d %d %d\n",
                    r.generated, r.arrived, r.lost, r.latency_us_sum, r.latency_us_max, r.hops_sum, r.attempts, r.acked, r.failed, r.deferred, r.rejected,
                    r.dropped, r.ready_us, r.next, r.queue_len, r.queue_max, r.tries);
        for (const rm_fwd_packet &pk : q) std::printf("queue %zu %d %d %" PRId64 " %" PRId64 "\n", j, pk.origin, pk.hops, pk.birth_us, pk.enq_us);
    }
    std::printf("totals %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
                tot.generated, tot.arrived, tot.dropped_retries, tot.dropped_no_route, tot.dropped_full, tot.dropped_ttl, tot.in_flight, tot.stray,
                tot.skipped_slots, tot.latency_us_sum, tot.hops_sum);
    if (!medium.setForwarding(nullptr)) std::printf("error %s\n", medium.lastError.c_str());
    std::printf("off %d\n", medium.getForwarding() ? 0 : 1);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    std::ifstream in(argv[1]);
    std::string kind;
    rm_fwd_params p = GpuRadioMedium::forwardingDefaults();
    long long unit;
    unsigned long long seed;
    int n;
    in >> kind >> p.queue_slots >> p.max_retries >> p.min_be >> p.max_be >> p.max_hops >> unit >> seed >> n;
    p.backoff_unit_us = unit;
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
        if (kind == "null") {
            NullRadioMedium medium;
            sim.setRadioMedium(&medium);
            return run(medium, sim, in, nodes, p);
        }
        UDGMRadioMedium medium;
        sim.setRadioMedium(&medium);
        return run(medium, sim, in, nodes, p);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
}
