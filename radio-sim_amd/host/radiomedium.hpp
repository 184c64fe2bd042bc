// radiomedium.hpp -- C++ host-side mirror of the reference's radio-medium plug-in API, above the
// C ABI (include/radiomedium_hip.h).  Same class and method names, argument meaning and error
// behaviour as the reference's Java (paths relative to
// /root/reference/radio-medium/java/se/sics/emul8/radiomedium/), written from scratch:
//
//   Position            Position.java:35-65        x, y, z, set(x,y[,z]), getDistance
//   Transciever         Transciever.java:3-114     txpower 0.0, channel 26, enabled, rx/txProbability 1.0,
//                                                  getRSSI / getReceivingState / setReceiving / clearReceiving ...
//   Node                Node.java:39-99            id, getIdAsInteger (-1 if not numeric), position, radio
//   RadioPacket         RadioPacket.java:38-111    source, start time, txpower / channel copied from the source,
//                                                  getPacketAirTime = 32 us per hex character
//   Simulator           Simulator.java             only what a medium touches: addNode / getNodes / getNode,
//                                                  getTime, getRandom seed, generateTransmissionEvents,
//                                                  generateReceptionEvents, deliverRadioPacket (recorded, in call order)
//   RadioMedium         RadioMedium.java:35-45     getName / setSimulator / transmit / getBaseRSSI
//   AbstractRadioMedium AbstractRadioMedium.java   baseRSSI = -100.0, setBaseRSSI
//   NullRadioMedium, UDGMRadioMedium, UDGMConstantLossRadioMedium, N2NRadioMedium
//                       the four reference media, here backed by the MI355X engine: transmit() is one
//                       rm_transmit call, and the heard links -- returned in node order -- become exactly the
//                       Simulator calls the reference's loops make.
//
// Two more modes of the media, for hosts that batch (the reference consumes a tick's events only in
// emulatorTimeStepDone -> processAllEvents, Simulator.java:155-165, so nothing forces one evaluation per packet):
//   setTickMode(true)      transmit() only queues the packet; Simulator::emulatorTimeStepDone flushes the queue in
//                          ONE evaluation (rm_tick_begin / rm_enqueue_tx / rm_tick_flush_view) before the time moves,
//                          and the medium then makes the very calls of the per-packet mode, in arrival x node order.
//   setDeviceEvents(true)  the events never reach the host: the engine keeps packets, heard links and every
//                          node's radio state on the device (rm_events_*), Simulator::emulatorTimeStepDone hands
//                          out the drain's deliveries in the reference queue's order, nodeInfo() the time-step
//                          message's per-node fields.
//
// There is no CPU evaluation in this file: without a gfx950 device the medium's constructor throws.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <limits>
#include <memory>
#include <cstdio>
#include <stdexcept>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/radiomedium_hip.h"

namespace emul8 {

class Simulator;
class RadioMedium;
class RadioPacket;

class Position {
public:
    double x = 0, y = 0, z = 0;
    void set(double x_, double y_) { set(x_, y_, 0.0); }
    void set(double x_, double y_, double z_) { x = x_; y = y_; z = z_; }
};

class Node;

class Transciever {
public:
    static constexpr int LISTENING = 0, TRANSMITTING = 1, RECEIVING = 2, DISABLED = 3;
    explicit Transciever(Node *node) : node_(node) {}
    Node *getNode() const { return node_; }
    bool isEnabled() const { return enabled_; }
    void setEnabled(bool e) { enabled_ = e; }
    double getTransmitPower() const { return txpower_; }
    void setTransmitPower(double p) { txpower_ = p; }
    int getWirelessChannel() const { return channel_; }
    void setWirelessChannel(int c) { channel_ = c; }
    double getRxProbability() const { return rxProbability_; }
    void setRxProbability(double p) { rxProbability_ = p; }
    double getTxProbability() const { return txProbability_; }
    void setTxProbability(double p) { txProbability_ = p; }
    bool isReceiving() const { return receiving_ != nullptr; }
    double getRSSI() const; // latched rssi while receiving, else the medium's base RSSI, else -99.99
    int getReceivingState() const
    {
        if (!enabled_) return DISABLED;
        if (receiving_) return RECEIVING;
        if (sending_) return TRANSMITTING;
        return LISTENING;
    }
    void setReceiving(const RadioPacket *p, double rssi) { clearSending(); receiving_ = p; receivingRSSI_ = rssi; }
    void clearReceiving() { receiving_ = nullptr; }
    void setSending(const RadioPacket *p) { clearReceiving(); sending_ = p; }
    void clearSending() { sending_ = nullptr; }

private:
    Node *node_;
    double txpower_ = 0.0;
    int channel_ = 26;
    bool enabled_ = true;
    const RadioPacket *receiving_ = nullptr, *sending_ = nullptr;
    double receivingRSSI_ = 0.0;
    double rxProbability_ = 1.0, txProbability_ = 1.0;
};

class Node {
public:
    Node(const std::string &id, Simulator *sim) : id_(id), sim_(sim), radio_(this)
    {
        char *end = nullptr;
        const long v = std::strtol(id.c_str(), &end, 10);
        intID_ = (!id.empty() && end && *end == '\0') ? int(v) : -1; // Integer.parseInt failed -> -1
    }
    const std::string &getId() const { return id_; }
    int getIdAsInteger() const { return intID_; }
    Position &getPosition() { return pos_; }
    Transciever &getRadio() { return radio_; }
    Simulator *getSimulator() const { return sim_; }
    RadioMedium *getRadioMedium() const;
    int index = -1; // position in Simulator.getNodes() (registration order)

private:
    std::string id_;
    int intID_;
    Simulator *sim_;
    Position pos_;
    Transciever radio_;
};

class RadioPacket {
public:
    RadioPacket(Node *node, int64_t time, const std::string &packetData)
        : node_(node), time_(time), txpower_(node->getRadio().getTransmitPower()),
          channel_(node->getRadio().getWirelessChannel()), data_(packetData) {}
    Node *getSource() const { return node_; }
    int64_t getStartTime() const { return time_; }
    int64_t getEndTime() const { return time_ + getPacketAirTime(); }
    int64_t getPacketAirTime() const { return int64_t(data_.size()) * 32; }
    double getTransmitPower() const { return txpower_; }
    void setTransmitPower(double p) { txpower_ = p; }
    int getWirelessChannel() const { return channel_; }
    void setWirelessChannel(int c) { channel_ = c; }
    const std::string &getPacketDataAsHex() const { return data_; }
    // RadioPacket.java:97-99 (DatatypeConverter.parseHexBinary): two hex digits per byte
    std::vector<uint8_t> getPacketDataAsBytes() const
    {
        if (data_.size() % 2) throw std::invalid_argument("hexBinary needs to be even-length: " + data_);
        auto nib = [&](char ch) -> int {
            if (ch >= '0' && ch <= '9') return ch - '0';
            if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
            if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
            throw std::invalid_argument("contains illegal character for hexBinary: " + data_);
        };
        std::vector<uint8_t> out(data_.size() / 2);
        for (size_t i = 0; i < out.size(); ++i) out[i] = uint8_t(nib(data_[2 * i]) * 16 + nib(data_[2 * i + 1]));
        return out;
    }

private:
    Node *node_;
    int64_t time_;
    double txpower_;
    int channel_;
    std::string data_;
};

class RadioMedium {
public:
    virtual ~RadioMedium() = default;
    virtual std::string getName() = 0;
    virtual void setSimulator(Simulator *sim) = 0;
    virtual void transmit(RadioPacket &packet) = 0;
    virtual double getBaseRSSI(Node &node) = 0;
    // hooks of Simulator::emulatorTimeStepDone (not in the reference's interface; no-ops for a plain medium)
    virtual void flush() {}                       // evaluate the transmit() calls queued since the last tick end
    virtual void processEvents(int64_t /*time*/) {} // the tick-end drain, when the medium keeps the events itself
};

// what the medium hands back to the simulation core, recorded in call order
struct MediumCall {
    enum Kind { TRANSMISSION_EVENTS, RECEPTION_EVENTS, DELIVER } kind;
    const RadioPacket *packet;
    Node *destination;   // null for TRANSMISSION_EVENTS
    double rssi;
    bool doDeliver;
    int64_t timeStart, timeEnd; // Simulator.java:323-333: max(start, currentTime), + air time
};

// RadioListener.java:35-38: "will receive all packets transmitted during a simulation"
class RadioListener {
public:
    virtual ~RadioListener() {}
    virtual void packetTransmission(RadioPacket &packet) = 0;
};

class Simulator {
public:
    explicit Simulator(int64_t randomSeed = 0) : seed_(randomSeed) {}
    // Simulator.java:200-211; the JSON handler notifies the listeners right after medium.transmit
    // (net/SimulatorJSONHandler.java:92)
    void addRadioListener(RadioListener *l) { listeners_.push_back(l); }
    void notifyRadioListeners(RadioPacket &p)
    {
        for (RadioListener *l : listeners_) l->packetTransmission(p);
    }
    int64_t getRandomSeed() const { return seed_; }
    int64_t getTime() const { return currentTime_; }
    void setTime(int64_t t) { currentTime_ = t; }
    RadioMedium *getRadioMedium() const { return medium_; }
    void setRadioMedium(RadioMedium *m)
    {
        if (m) m->setSimulator(this);
        medium_ = m;
    }
    Node *getNode(const std::string &id)
    {
        auto it = table_.find(id);
        return it == table_.end() ? nullptr : it->second;
    }
    const std::vector<Node *> &getNodes() const { return nodes_; }
    uint64_t nodesVersion() const { return version_; }
    void nodesChanged() { ++version_; } // call after changing fields of existing nodes (no hook in the reference)
    // the finer hook: one node's fields changed (node-config-set, SimulatorJSONHandler.java:105-143);
    // the medium writes just these nodes to the device before its next evaluation (rm_node_update)
    void nodeChanged(const Node *n) { if (n) dirty_.push_back(n->index); }
    std::vector<int> takeChangedNodes()
    {
        std::vector<int> d;
        d.swap(dirty_);
        return d;
    }
    Node *addNode(const std::string &id)
    {
        if (Node *n = getNode(id)) return n; // already handled
        owned_.emplace_back(new Node(id, this));
        Node *n = owned_.back().get();
        n->index = int(nodes_.size());
        nodes_.push_back(n);
        table_[id] = n;
        ++version_;
        return n;
    }
    // Simulator.emulatorTimeStepDone (Simulator.java:155-165): currentTime = stepTime; processAllEvents(currentTime).
    // A medium in tick mode evaluates its queued transmit() calls first -- while currentTime is still the old one,
    // which is what the event times of those packets were computed with in the reference (:323-326).
    void emulatorTimeStepDone(int64_t stepTime)
    {
        if (medium_) medium_->flush();
        currentTime_ = stepTime;
        if (medium_) medium_->processEvents(stepTime);
    }
    void generateTransmissionEvents(RadioPacket &p) { record(MediumCall::TRANSMISSION_EVENTS, p, nullptr, 0.0, false); }
    void generateReceptionEvents(RadioPacket &p, Node *dst, double rssi, bool doDeliver)
    {
        record(MediumCall::RECEPTION_EVENTS, p, dst, rssi, doDeliver);
    }
    void deliverRadioPacket(RadioPacket &p, Node *dst, double rssi) { record(MediumCall::DELIVER, p, dst, rssi, true); }
    std::vector<MediumCall> calls;
    bool recording = true;   // false: the calls are only counted (timing runs: the list is this stub's, not the engine's, work)
    uint64_t callCount = 0;

private:
    void record(MediumCall::Kind k, RadioPacket &p, Node *dst, double rssi, bool deliver)
    {
        ++callCount;
        if (!recording) return;
        int64_t t0 = p.getStartTime();
        if (t0 < currentTime_) t0 = currentTime_;
        calls.push_back({k, &p, dst, rssi, deliver, t0, t0 + p.getPacketAirTime()});
    }
    std::vector<RadioListener *> listeners_;
    int64_t seed_;
    int64_t currentTime_ = 0;
    RadioMedium *medium_ = nullptr;
    std::vector<std::unique_ptr<Node>> owned_;
    std::vector<Node *> nodes_;
    std::unordered_map<std::string, Node *> table_;
    uint64_t version_ = 0;
    std::vector<int> dirty_;
};

// The receiver-side state machine the verdicts drive (events/ReceptionEvent.java:12-46,
// events/TransmissionEvent.java:18-26): the start flank latches packet + rssi (and clears a pending
// transmission), the end flank clears the reception -- whichever packet it belongs to -- and
// delivers only in delivery mode.
enum class ReceptionMode { start, interference, delivery };

struct ReceptionEvent {
    int64_t time;
    Simulator *simulator;
    RadioPacket *packet;
    Node *destination;
    double rssi;
    ReceptionMode mode;
    void execute(int64_t /*currentTime*/)
    {
        Transciever &t = destination->getRadio();
        if (mode == ReceptionMode::start) {
            t.setReceiving(packet, rssi);
        } else {
            t.clearReceiving();
            if (mode == ReceptionMode::delivery) simulator->deliverRadioPacket(*packet, destination, rssi);
        }
    }
};

struct TransmissionEvent {
    int64_t time;
    RadioPacket *packet;
    bool isStart;
    void execute(int64_t /*currentTime*/)
    {
        Transciever &t = packet->getSource()->getRadio();
        if (isStart) t.setSending(packet);
        else t.clearSending();
    }
};

// the two events generateReceptionEvents queues for one heard link (Simulator.java:321-335)
inline void makeReceptionEvents(Simulator &sim, const MediumCall &c, RadioPacket &p, ReceptionEvent &startEv, ReceptionEvent &endEv)
{
    startEv = {c.timeStart, &sim, &p, c.destination, c.rssi, ReceptionMode::start};
    endEv = {c.timeEnd, &sim, &p, c.destination, c.rssi, c.doDeliver ? ReceptionMode::delivery : ReceptionMode::interference};
}

inline RadioMedium *Node::getRadioMedium() const { return sim_->getRadioMedium(); }
inline double Transciever::getRSSI() const
{
    if (isReceiving()) return receivingRSSI_;
    RadioMedium *m = node_->getRadioMedium();
    return m ? m->getBaseRSSI(*node_) : -99.99;
}

class AbstractRadioMedium : public RadioMedium {
public:
    void setSimulator(Simulator *sim) override { simulator = sim; }
    double getBaseRSSI(Node &) override { return baseRSSI; }
    void setBaseRSSI(double rssi) { baseRSSI = rssi; }

protected:
    Simulator *simulator = nullptr;
    double baseRSSI = -100.0;
};

// One MI355X context behind the RadioMedium contract.
class GpuRadioMedium : public AbstractRadioMedium {
public:
    explicit GpuRadioMedium(int kind, int device = 0) : kind_(kind)
    {
        if (rm_abi_version() != RM_ABI_VERSION)
            throw std::runtime_error("libradiomedium_hip.so does not have the ABI version of the header this host was built against");
        if (rm_create(device, &ctx_) != RM_OK) throw std::runtime_error(std::string("no MI355X radio medium: ") + rm_last_error());
        rm_model_defaults(&params_, kind);
        apply();
    }
    ~GpuRadioMedium() override { rm_destroy(ctx_); }
    GpuRadioMedium(const GpuRadioMedium &) = delete;
    GpuRadioMedium &operator=(const GpuRadioMedium &) = delete;

    std::string getName() override { return rm_get_name(ctx_); }
    void setSimulator(Simulator *sim) override
    {
        simulator = sim;
        if (sim) rm_seed(ctx_, sim->getRandomSeed()); // Simulator.getRandom(): one generator for all packets
        uploaded_ = ~0ull;
    }
    double getBaseRSSI(Node &n) override { return rm_get_base_rssi(ctx_, n.index); }
    void setBaseRSSI(double rssi)
    {
        baseRSSI = rssi;
        rm_set_base_rssi(ctx_, rssi);
    }

    // ---- batching modes (see the top of this file)
    void setTickMode(bool on) { tickMode_ = on; }
    bool getTickMode() const { return tickMode_; }
    void setDeviceEvents(bool on)
    {
        if (on == deviceEvents_) return;
        if ((on ? rm_events_enable(ctx_, 0, 0) : rm_events_disable(ctx_)) != RM_OK) throw std::runtime_error(rm_last_error());
        deviceEvents_ = on;
        for (size_t i = inFlightHead_; i < inFlight_.size(); ++i) released_.push_back(inFlight_[i]);
        inFlight_.clear();
        inFlightHead_ = 0;
        firstInFlight_ = on ? rm_events_next_packet(ctx_) : 0;
    }
    bool getDeviceEvents() const { return deviceEvents_; }
    // Tick mode / device events: the medium refers to a RadioPacket from transmit() until it says so here -- the
    // packet's last event has fired on the device, or a failed evaluation dropped it.  A host that owns the
    // RadioPacket objects frees exactly these (by identity: a failed flush leaves no packet behind that an older,
    // still pending one could be mistaken for).  Without device events the packets handed to transmit() live in the
    // host Simulator's own events, as in the reference.
    void takeReleased(std::vector<RadioPacket *> &out)
    {
        out.insert(out.end(), released_.begin(), released_.end());
        released_.clear();
    }
    size_t inFlightCount() const { return queue_.size() + inFlight_.size() - inFlightHead_; }

    // the transmit() calls queued in tick mode, in ONE evaluation; then the calls the per-packet mode makes
    void flush() override
    {
        if (queue_.empty()) return;
        lastError.clear();
        Simulator *sim = simulator;
        std::vector<RadioPacket *> q;
        q.swap(queue_);
        // whatever fails from here on: the tick's packets were never numbered by the engine, nothing refers to them
        auto dropped = [&](const std::string &why) {
            lastError = why;
            if (deviceEvents_) released_.insert(released_.end(), q.begin(), q.end());
        };
        if (!sim) return dropped("No simulator");
        const std::vector<Node *> &nodes = sim->getNodes();
        if (!sync(sim, nodes)) return dropped(lastError);
        rm_set_time(ctx_, sim->getTime());
        int rc = rm_tick_begin(ctx_, sim->getTime(), sim->getTime());
        for (size_t k = 0; k < q.size() && rc == RM_OK; ++k) {
            const double txp = q[k]->getTransmitPower();
            const int32_t ch = q[k]->getWirelessChannel();
            rc = rm_enqueue_tx(ctx_, q[k]->getSource()->index, q[k]->getStartTime(), q[k]->getPacketAirTime(), &txp, &ch);
        }
        if (rc != RM_OK) return dropped(rm_last_error());
        if (deviceEvents_) { // nothing comes back: packets, links and events stay on the device
            const int64_t before = rm_events_next_packet(ctx_);
            if (rm_tick_run(ctx_) != RM_OK) return dropped(rm_last_error());
            // the engine numbers the packets of a tick it has taken, in enqueue order
            if (rm_events_next_packet(ctx_) - before != int64_t(q.size()) || before != firstInFlight_ + int64_t(inFlight_.size() - inFlightHead_))
                return dropped("radio medium: packet numbers out of step with the engine");
            for (RadioPacket *p : q) inFlight_.push_back(p);
            return;
        }
        rm_host_result r{};
        if (rm_tick_flush_view(ctx_, &r) != RM_OK) { lastError = rm_last_error(); return; }
        for (uint32_t k = 0; k < r.n_packets; ++k) { // arrival order, then node order: the per-packet calls
            RadioPacket &packet = *q[k];
            if (kind_ != RM_MODEL_UDGM_CONST) sim->generateTransmissionEvents(packet);
            for (uint32_t i = r.pkt_offset[k]; i < r.pkt_offset[k + 1]; ++i) {
                Node *node = nodes[size_t(r.dst[i])];
                // (the reference's media hand the packet's transmit power through -- UDGMRadioMedium.java:95 --: one value per packet)
                const double rssi = r.rssi ? r.rssi[i] : r.pkt_rssi[k];
                if (kind_ == RM_MODEL_UDGM_CONST) sim->deliverRadioPacket(packet, node, rssi);
                else sim->generateReceptionEvents(packet, node, rssi, r.verdict[i] == RM_DELIVERED);
            }
        }
    }

    // device events: Simulator.processAllEvents(time) as one drain on the device; the deliveries come back in the
    // order the reference's queue pops them and become Simulator.deliverRadioPacket calls (ReceptionEvent.java:41-44)
    void processEvents(int64_t time) override
    {
        if (!deviceEvents_) return;
        Simulator *sim = simulator;
        rm_delivery_view v{};
        if (rm_events_process(ctx_, time, &v) != RM_OK) { lastError = rm_last_error(); return; }
        const std::vector<Node *> &nodes = sim->getNodes();
        RadioPacket *const *const flying = inFlight_.data() + inFlightHead_;
        const size_t n_flying = inFlight_.size() - inFlightHead_;
        for (uint32_t r = 0; r < v.n_runs; ++r) { // a run = the deliveries of one packet (adjacent in the queue's pop order)
            const int64_t k = v.run_packet[r] - firstInFlight_;
            const uint32_t first = v.run_first[r], end = first + v.run_count[r];
            if (k < 0 || size_t(k) >= n_flying || end > v.count || end < first) {
                lastError = "radio medium: a delivery names a packet the host does not hold";
                continue;
            }
            for (uint32_t i = first; i < end; ++i) {
                if (v.dst[i] < 0 || size_t(v.dst[i]) >= nodes.size()) {
                    lastError = "radio medium: a delivery names a node the host does not hold";
                    continue;
                }
                sim->deliverRadioPacket(*flying[size_t(k)], nodes[size_t(v.dst[i])], v.rssi[i]);
            }
        }
        // packets whose last event has fired are forgotten: everything below the oldest number still queued
        while (firstInFlight_ < v.oldest_packet && inFlightHead_ < inFlight_.size()) {
            released_.push_back(inFlight_[inFlightHead_]);
            ++inFlightHead_;
            ++firstInFlight_;
        }
        if (inFlightHead_ > 4096 && inFlightHead_ * 2 > inFlight_.size()) { // the consumed front half goes away
            inFlight_.erase(inFlight_.begin(), inFlight_.begin() + long(inFlightHead_));
            inFlightHead_ = 0;
        }
    }

    // the per-node fields of a time-step message (net/JSONClientConnection.java:331-341) from the device's radio state
    bool nodeInfo(const std::vector<int32_t> &nodes, std::vector<double> &rssi, std::vector<int32_t> &receiving,
                  std::vector<int32_t> &channel)
    {
        rssi.resize(nodes.size()); receiving.resize(nodes.size()); channel.resize(nodes.size());
        if (simulator && !sync(simulator, simulator->getNodes())) return false; // the device mirrors the node table first
        if (rm_node_info(ctx_, nodes.data(), int32_t(nodes.size()), rssi.data(), receiving.data(), channel.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }

    // ... and only of the nodes whose fields differ from what this call reported for them last (every node the first time,
    // and after the node table has changed size): a host that keeps the text of its last time-step message re-serialises these
    bool nodeInfoChanged(std::vector<int32_t> &nodes, std::vector<double> &rssi, std::vector<int32_t> &receiving, std::vector<int32_t> &channel)
    {
        nodes.clear(); rssi.clear(); receiving.clear(); channel.clear();
        if (!simulator) return true;
        const size_t n = simulator->getNodes().size();
        if (!sync(simulator, simulator->getNodes())) return false; // the device mirrors the node table first
        if (n == 0) return true;
        // room for every node, kept between the calls (a step's answer is a few of them: four fresh vectors of n elements --
        // allocated, zeroed, paged in -- cost more than the query itself at 100 k nodes)
        if (chgNodes_.size() < n) {
            chgNodes_.resize(n); chgRssi_.resize(n); chgRecv_.resize(n); chgChan_.resize(n);
        }
        int32_t count = 0;
        if (rm_node_info_changed(ctx_, chgNodes_.data(), chgRssi_.data(), chgRecv_.data(), chgChan_.data(), int32_t(n), &count) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        nodes.assign(chgNodes_.begin(), chgNodes_.begin() + count);
        rssi.assign(chgRssi_.begin(), chgRssi_.begin() + count);
        receiving.assign(chgRecv_.begin(), chgRecv_.begin() + count);
        channel.assign(chgChan_.begin(), chgChan_.begin() + count);
        return true;
    }

    // transmit(): never throws (the reference's returns void); failures are reported through lastError
    void transmit(RadioPacket &packet) override
    {
        if (tickMode_) { // evaluated at the end of the tick, with everything else that was sent in it
            queue_.push_back(&packet);
            return;
        }
        lastError.clear();
        Simulator *sim = simulator;
        if (!sim) { lastError = "No simulator"; return; }
        const std::vector<Node *> &nodes = sim->getNodes();
        if (!sync(sim, nodes)) return;
        rm_set_time(ctx_, sim->getTime());
        const double txp = packet.getTransmitPower();
        const int32_t ch = packet.getWirelessChannel();
        uint32_t heard = 0;
        uint8_t interference = 0;
        const int64_t before = deviceEvents_ ? rm_events_next_packet(ctx_) : 0;
        const int rc = rm_transmit(ctx_, packet.getSource()->index, packet.getStartTime(),
                                   int64_t(packet.getPacketDataAsHex().size()), &txp, &ch, dst_.data(), verdict_.data(),
                                   rssi_.data(), sinr_.data(), uint32_t(dst_.size()), &heard, &interference);
        if (deviceEvents_) { // the engine queued the packet's events itself -- if it numbered the packet
            if (rm_events_next_packet(ctx_) == before + 1 && before == firstInFlight_ + int64_t(inFlight_.size() - inFlightHead_))
                inFlight_.push_back(&packet);
            else
                released_.push_back(&packet);
            if (rc != RM_OK) lastError = rm_last_error();
            else lastInterference = interference != 0;
            return;
        }
        if (rc != RM_OK) { lastError = rm_last_error(); return; }
        lastInterference = interference != 0;
        if (kind_ != RM_MODEL_UDGM_CONST) sim->generateTransmissionEvents(packet);
        for (uint32_t i = 0; i < heard; ++i) { // node order, as the reference's for (Node node : nodes)
            Node *node = nodes[dst_[i]];
            if (kind_ == RM_MODEL_UDGM_CONST) sim->deliverRadioPacket(packet, node, rssi_[i]);
            else sim->generateReceptionEvents(packet, node, rssi_[i], verdict_[i] == RM_DELIVERED);
        }
    }
    // Per-node traffic counters accumulated on the device (extension E11): with statistics on, every evaluating call of the medium
    // (transmit(), the tick mode, transmitIfClear(), transmitCsmaBatch()) adds its frames and heard links to one rm_node_stats per
    // node of Simulator.getNodes() -- frames sent and failed, links heard and delivered on both sides, air time sent and received.
    // The setting survives apply(); a node table of another size starts a zeroed table.  false and lastError on a refusal.
    bool setStatistics(bool on)
    {
        if (rm_stats_enable(ctx_, on ? 1 : 0) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        statistics_ = on;
        return true;
    }
    bool getStatisticsEnabled() const { return rm_stats_enabled(ctx_) != 0; }
    bool resetStatistics()
    {
        if (rm_stats_reset(ctx_) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // one node's counters (all zero and lastError on a refusal) / every node's, in the order of Simulator.getNodes() (empty and
    // lastError on a refusal); `totals`: the ticks counted and skipped
    rm_node_stats getStatistics(const Node &node, rm_stats_totals *totals = nullptr)
    {
        rm_node_stats out{};
        const int32_t i = node.index;
        if (!syncNodes()) return out; // the device mirrors the node table first: the table has its size
        if (rm_stats_read(ctx_, &i, 1, &out, totals) != RM_OK) {
            lastError = rm_last_error();
            out = rm_node_stats{};
        }
        return out;
    }
    std::vector<rm_node_stats> getStatistics(rm_stats_totals *totals = nullptr)
    {
        std::vector<rm_node_stats> out;
        if (!syncNodes()) return out;
        out.resize(simulator ? simulator->getNodes().size() : size_t(rm_node_count(ctx_)));
        if (rm_stats_read(ctx_, nullptr, int32_t(out.size()), out.data(), totals) != RM_OK) {
            lastError = rm_last_error();
            out.clear();
        }
        return out;
    }
    // Receiver listening schedules (extension E13): a duty-cycled radio that sleeps at a frame's first microsecond does not get the
    // frame -- with a schedule set, every evaluating call of the medium ends with one more pass over its verdicts, so the reception
    // events of transmit(), the tick mode, transmitIfClear() and transmitCsmaBatch() honour it.  period_us 0 (with on_us = phase_us
    // = 0): the node always listens.  The schedules survive apply(); false and lastError on a refusal.
    bool setListenSchedule(const Node &node, int64_t period_us, int64_t on_us, int64_t phase_us)
    {
        if (!syncNodes()) return false; // the device mirrors the node table first: the tables have its size
        const int32_t i = node.index;
        const rm_listen_schedule s = {period_us, on_us, phase_us};
        if (!restoreListenSchedules()) return false; // (a node table of another size has cleared the engine's tables: all of them again)
        if (rm_listen_set(ctx_, &i, 1, &s) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        listen_[i] = s;
        return true;
    }
    bool clearListenSchedules()
    {
        listen_.clear();
        if (rm_listen_clear(ctx_) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool getListenEnabled() const { return rm_listen_enabled(ctx_) != 0; }
    // frames everything else had delivered to the node and that sleep alone lost (0 and lastError on a refusal)
    uint64_t getListenMissed(const Node &node)
    {
        uint64_t out = 0;
        const int32_t i = node.index;
        if (!syncNodes()) return 0;
        if (rm_listen_missed_read(ctx_, &i, 1, &out) != RM_OK) {
            lastError = rm_last_error();
            return 0;
        }
        return out;
    }
    // Traffic schedules (extension E15): a node with period_us > 0 has a packet due at phase_us + k period_us + jitter (a hash of
    // seed, node and k below jitter_us) for k = 0, 1, ...; generateTraffic() gives, for every half-open window [win_lo[b],
    // win_hi[b]) -- in time order, disjoint -- the nodes with a packet due in it, in the order of Simulator.getNodes(), computed on
    // the device.  No call of the medium changes; period_us 0 (with the other values 0): the node generates nothing.  The schedules
    // survive apply(); false and lastError on a refusal.
    bool setTrafficSchedule(const Node &node, int64_t period_us, int64_t phase_us, int64_t jitter_us)
    {
        if (!syncNodes()) return false; // the device mirrors the node table first: the table has its size
        const int32_t i = node.index;
        const rm_traffic_schedule s = {period_us, phase_us, jitter_us, 0};
        if (!restoreTrafficSchedules()) return false; // (a node table of another size has cleared the engine's table: all of them again)
        if (rm_traffic_set(ctx_, &i, 1, &s) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        traffic_[i] = s;
        return true;
    }
    bool clearTrafficSchedules()
    {
        traffic_.clear();
        if (rm_traffic_clear(ctx_) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool getTrafficEnabled() const { return rm_traffic_enabled(ctx_) != 0; }
    // sources[b]: the nodes of window b, at most cap of them (the first in node order); totals (may be nullptr): packets due,
    // second and later packets of a node in one window, sources beyond cap
    bool generateTraffic(uint64_t seed, const std::vector<int64_t> &win_lo, const std::vector<int64_t> &win_hi, int32_t cap,
                         std::vector<std::vector<Node *>> &sources, rm_traffic_totals *totals = nullptr)
    {
        sources.clear();
        if (!simulator || !syncNodes() || !restoreTrafficSchedules()) return false;
        if (win_lo.size() != win_hi.size() || win_lo.empty() || cap < 1) {
            lastError = "generateTraffic: one win_hi per win_lo, one window at least, cap >= 1";
            return false;
        }
        const int32_t n_ticks = int32_t(win_lo.size());
        std::vector<int32_t> rows(win_lo.size() * size_t(cap)), count(win_lo.size());
        if (rm_traffic_generate(ctx_, seed, n_ticks, win_lo.data(), win_hi.data(), cap, rows.data(), count.data(), totals) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        const std::vector<Node *> &nodes = simulator->getNodes();
        sources.resize(win_lo.size());
        for (size_t b = 0; b < win_lo.size(); ++b)
            for (int32_t k = 0; k < std::min(count[b], cap); ++k) sources[b].push_back(nodes[size_t(rows[b * size_t(cap) + size_t(k)])]);
        return true;
    }
    // Watched-link statistics (extension E14): per-link counters for a node's routing parent and a handful of candidate parents.
    // setLinkWatch(K) gives every node K slots of watched peers (K = 1, 2, 4 or 8; 0 switches the feature off); watchLinks(node,
    // peers) fills the node's slots (nullptr: an empty slot; fewer than K peers: the rest empty) -- a slot whose peer stays keeps
    // its counters, one whose peer changes starts from a cleared entry --; every evaluating call of the medium then adds each heard
    // link from a watched peer to that (node, slot) entry.  K and the watch rows survive apply(); false and lastError on a refusal.
    bool setLinkWatch(int K)
    {
        if (K > 0 && !syncNodes()) return false; // the device mirrors the node table first: the tables have its size
        if (rm_linkstats_enable(ctx_, int32_t(K)) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        if (K != linkWatchK_) linkWatch_.clear();
        linkWatchK_ = K;
        return true;
    }
    int getLinkWatch() const { return rm_linkstats_enabled(ctx_); }
    bool watchLinks(const Node &node, const std::vector<const Node *> &peers)
    {
        if (!syncNodes()) return false;
        if (!restoreLinkWatch()) return false; // (a node table of another size has switched the engine's feature off: all rows again)
        if (linkWatchK_ <= 0 || peers.size() > size_t(linkWatchK_)) {
            lastError = "watchLinks: setLinkWatch(K) comes first, and a node has K slots";
            return false;
        }
        std::vector<int32_t> row(size_t(linkWatchK_), -1);
        for (size_t k = 0; k < peers.size(); ++k) row[k] = peers[k] ? peers[k]->index : -1;
        const int32_t i = node.index;
        if (rm_linkstats_watch(ctx_, &i, 1, row.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        linkWatch_[i] = row;
        return true;
    }
    // the node's K entries in slot order (empty and lastError on a refusal); `totals`: the ticks counted and skipped
    std::vector<rm_link_stats> getLinkStatistics(const Node &node, rm_stats_totals *totals = nullptr)
    {
        std::vector<rm_link_stats> out;
        if (!syncNodes()) return out;
        const int K = rm_linkstats_enabled(ctx_);
        out.resize(size_t(K > 0 ? K : 0));
        const int32_t i = node.index;
        if (K <= 0 || rm_linkstats_read(ctx_, &i, 1, out.data(), totals) != RM_OK) {
            lastError = K <= 0 ? "no watched-link statistics: setLinkWatch(K) comes first" : rm_last_error();
            out.clear();
        }
        return out;
    }
    // The measured-route query (extension E21): least path cost (measured ETX in units of 1/128) toward a set of roots over the
    // watched links' counters as they stand, and the parent on such a path -- the current parent (current[i] for node i of
    // Simulator.getNodes(), nullptr: none; an empty list: no current parents) kept while its path is within params.hysteresis of
    // the least cost.  tables: the caller's own watch table (host arrays, a row per node) in place of the medium's.  One row per
    // node in node order; empty rows and lastError on a refusal (without tables, setLinkWatch(K) comes first).
    struct MeasuredRouteRow {
        uint64_t cost; // RM_ROUTE_UNREACHED: not reached
        Node *parent;  // nullptr for a root and for a node that was not reached
        int slot;      // the watch slot of the link to the parent, -1 without one
        uint32_t linkCost;
        int children;
    };
    struct MeasuredRouteTree {
        std::vector<MeasuredRouteRow> rows;
        rm_etx_totals totals;
    };
    static rm_etx_params measuredRouteDefaults()
    {
        rm_etx_params p;
        rm_etx_defaults(&p);
        return p;
    }
    MeasuredRouteTree measuredRoutes(const rm_etx_params &params, const std::vector<const Node *> &roots, const std::vector<const Node *> &current = {},
                                     const rm_etx_tables *tables = nullptr)
    {
        lastError.clear();
        MeasuredRouteTree tree{{}, {0, 0, 0, 0, 0, 0, 0}};
        if (!simulator || !syncNodes()) return tree;
        const std::vector<Node *> &all = simulator->getNodes();
        const size_t n = all.size();
        if (!current.empty() && current.size() != n) {
            lastError = "measuredRoutes: one current parent (or nullptr) per node";
            return tree;
        }
        std::vector<int32_t> idx, cur;
        for (const Node *nd : roots) idx.push_back(nd ? nd->index : -1);
        for (const Node *nd : current) cur.push_back(nd ? nd->index : -1);
        std::vector<uint64_t> cost(n + 1);
        std::vector<int32_t> parent(n + 1), slot(n + 1), children(n + 1);
        std::vector<uint32_t> linkCost(n + 1);
        const rm_etx_out out{cost.data(), parent.data(), slot.data(), linkCost.data(), children.data()};
        if (rm_etx_query(ctx_, &params, tables, idx.data(), int32_t(idx.size()), cur.empty() ? nullptr : cur.data(), &out, &tree.totals) != RM_OK) {
            lastError = rm_last_error();
            tree.totals = {0, 0, 0, 0, 0, 0, 0};
            return tree;
        }
        tree.rows.resize(n);
        for (size_t j = 0; j < n; ++j)
            tree.rows[j] = MeasuredRouteRow{cost[j], parent[j] >= 0 ? all[size_t(parent[j])] : nullptr, slot[j], linkCost[j], children[j]};
        return tree;
    }
    // Forwarding queues (extension E19): per-node packet queues and a next-hop table on the device; packets move one hop per
    // evaluated tick.  setForwarding(&params) makes the queues (nullptr: releases them); setNextHops gives every node its next hop
    // (parents[i] for node i of Simulator.getNodes(), nullptr: no route) and makes the listed nodes sinks; forwardInject puts one
    // new packet at every listed node; forwardSources gives the nodes with a packet to send at `time` in node order (at most cap;
    // *count: their true number); forwardAdvance reads the LAST evaluated tick -- the tick mode's flush -- and moves the queues:
    // without candidates every frame's own source made the attempt, with them candidates[k] is packet k's.  The state is the
    // device's: it survives apply(), and a node table of another size switches the feature off (setForwarding again starts from
    // nothing).  false (or an empty list) and lastError on a refusal.
    static rm_fwd_params forwardingDefaults()
    {
        rm_fwd_params p;
        rm_fwd_defaults(&p);
        return p;
    }
    bool setForwarding(const rm_fwd_params *params)
    {
        lastError.clear();
        if (params && !syncNodes()) return false; // the device mirrors the node table first: the tables have its size
        if ((params ? rm_fwd_enable(ctx_, params) : rm_fwd_disable(ctx_)) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool getForwarding() const { return rm_fwd_enabled(ctx_) != 0; }
    bool setNextHops(const std::vector<const Node *> &parents, const std::vector<const Node *> &sinks, int64_t time)
    {
        lastError.clear();
        if (!simulator || !syncNodes()) return false;
        if (parents.size() != simulator->getNodes().size()) {
            lastError = "setNextHops: one parent (or nullptr) per node";
            return false;
        }
        std::vector<int32_t> par, roots;
        for (const Node *nd : parents) par.push_back(nd ? nd->index : -1);
        for (const Node *nd : sinks) roots.push_back(nd ? nd->index : -1);
        par.push_back(-1); // (never an empty array)
        if (rm_fwd_set_next(ctx_, par.data(), roots.empty() ? nullptr : roots.data(), int32_t(roots.size()), time) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool forwardInject(const std::vector<const Node *> &sources, int64_t time)
    {
        lastError.clear();
        if (!syncNodes()) return false;
        std::vector<int32_t> src;
        for (const Node *nd : sources) src.push_back(nd ? nd->index : -1);
        if (rm_fwd_inject(ctx_, src.empty() ? nullptr : src.data(), int32_t(src.size()), time) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    std::vector<Node *> forwardSources(int64_t time, int32_t cap, int32_t *count = nullptr)
    {
        lastError.clear();
        std::vector<Node *> out;
        if (count) *count = 0;
        if (!simulator || !syncNodes()) return out;
        std::vector<int32_t> src(size_t(cap > 0 ? cap : 0) + 1);
        int32_t n = 0;
        if (rm_fwd_sources(ctx_, time, cap, src.data(), &n) != RM_OK) {
            lastError = rm_last_error();
            return out;
        }
        const std::vector<Node *> &nodes = simulator->getNodes();
        for (int32_t k = 0; k < std::min(n, cap); ++k) out.push_back(nodes[size_t(src[size_t(k)])]);
        if (count) *count = n;
        return out;
    }
    bool forwardAdvance(const std::vector<const Node *> *candidates = nullptr)
    {
        lastError.clear();
        std::vector<int32_t> cand;
        if (candidates)
            for (const Node *nd : *candidates) cand.push_back(nd ? nd->index : -1);
        cand.push_back(-1); // (never an empty array; not counted)
        if (rm_fwd_advance(ctx_, 0, candidates ? cand.data() : nullptr, candidates ? int32_t(candidates->size()) : 0) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // the node's row; totals (may be nullptr); queue (may be nullptr): its packets in queue order
    bool getForwardStatistics(const Node &node, rm_fwd_node *out, rm_fwd_totals *totals = nullptr, std::vector<rm_fwd_packet> *queue = nullptr)
    {
        lastError.clear();
        const int32_t i = node.index;
        rm_fwd_params p;
        if (!out || !syncNodes()) return false;
        if (rm_fwd_get_params(ctx_, &p) != RM_OK || rm_fwd_read(ctx_, &i, 1, out, totals) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        if (queue) {
            int32_t len = 0;
            queue->assign(size_t(p.queue_slots), rm_fwd_packet{});
            if (rm_fwd_queue_read(ctx_, &i, 1, queue->data(), &len) != RM_OK) {
                lastError = rm_last_error();
                queue->clear();
                return false;
            }
            queue->resize(size_t(len));
        }
        return true;
    }
    // Dissemination floods (extension E20): Trickle-timed broadcast relay on the device.  setFlooding(&params) makes the table
    // (nullptr: releases it); floodSeed gives the data to the listed nodes at `time`; floodSources rolls the suppression and gives
    // the nodes due at `time` in node order (at most cap; *count: their true number); floodAdvance reads the LAST evaluated tick --
    // the tick mode's flush -- and moves the flood: without candidates every frame's own source transmitted, with them
    // candidates[k] is packet k's; floodTree gives every node's parent (nullptr: a seed or a node without the data) and hop (-1:
    // without the data).  The state is the device's: it survives apply(), and a node table of another size switches the feature
    // off.  false (or an empty list) and lastError on a refusal.
    static rm_flood_params floodingDefaults()
    {
        rm_flood_params p;
        rm_flood_defaults(&p);
        return p;
    }
    bool setFlooding(const rm_flood_params *params)
    {
        lastError.clear();
        if (params && !syncNodes()) return false; // the device mirrors the node table first: the table has its size
        if ((params ? rm_flood_enable(ctx_, params) : rm_flood_disable(ctx_)) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool getFlooding() const { return rm_flood_enabled(ctx_) != 0; }
    bool floodSeed(const std::vector<const Node *> &seeds, int64_t time)
    {
        lastError.clear();
        if (!syncNodes()) return false;
        std::vector<int32_t> idx;
        for (const Node *nd : seeds) idx.push_back(nd ? nd->index : -1);
        if (rm_flood_seed(ctx_, idx.empty() ? nullptr : idx.data(), int32_t(idx.size()), time) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    std::vector<Node *> floodSources(int64_t time, int32_t cap, int32_t *count = nullptr)
    {
        lastError.clear();
        std::vector<Node *> out;
        if (count) *count = 0;
        if (!simulator || !syncNodes()) return out;
        std::vector<int32_t> src(size_t(cap > 0 ? cap : 0) + 1);
        int32_t n = 0;
        if (rm_flood_sources(ctx_, time, cap, src.data(), &n) != RM_OK) {
            lastError = rm_last_error();
            return out;
        }
        const std::vector<Node *> &nodes = simulator->getNodes();
        for (int32_t k = 0; k < std::min(n, cap); ++k) out.push_back(nodes[size_t(src[size_t(k)])]);
        if (count) *count = n;
        return out;
    }
    bool floodAdvance(const std::vector<const Node *> *candidates = nullptr)
    {
        lastError.clear();
        std::vector<int32_t> cand;
        if (candidates)
            for (const Node *nd : *candidates) cand.push_back(nd ? nd->index : -1);
        cand.push_back(-1); // (never an empty array; not counted)
        if (rm_flood_advance(ctx_, 0, candidates ? cand.data() : nullptr, candidates ? int32_t(candidates->size()) : 0) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // the node's row; totals (may be nullptr)
    bool getFloodStatistics(const Node &node, rm_flood_node *out, rm_flood_totals *totals = nullptr)
    {
        lastError.clear();
        const int32_t i = node.index;
        if (!out || !syncNodes()) return false;
        if (rm_flood_read(ctx_, &i, 1, out, totals) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool floodTree(std::vector<Node *> *parents, std::vector<int32_t> *hops = nullptr)
    {
        lastError.clear();
        if (!parents || !simulator || !syncNodes()) return false;
        const std::vector<Node *> &nodes = simulator->getNodes();
        std::vector<rm_flood_node> rows(nodes.size() + 1);
        if (rm_flood_read(ctx_, nullptr, int32_t(nodes.size()), rows.data(), nullptr) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        parents->assign(nodes.size(), nullptr);
        if (hops) hops->assign(nodes.size(), -1);
        for (size_t j = 0; j < nodes.size(); ++j) {
            const int32_t par = rows[j].parent;
            if (par >= 0 && size_t(par) < nodes.size()) (*parents)[j] = nodes[size_t(par)];
            if (hops) (*hops)[j] = rows[j].hop;
        }
        return true;
    }
    // Neighbour tables (extension E22): the watched links' peer rows learnt from the frames heard.  setLinkWatch(K) comes first;
    // setNeighbourTable(&params) switches the rule on (nullptr: off; the watch tables stay); updateNeighbours reads the LAST
    // evaluated tick -- the tick mode's flush -- and admits at most one new peer per node, into an empty slot or in place of a
    // stale or poor one that is not pinned; expireNeighbours empties the stale slots that are not pinned.  pinned: empty, or one
    // entry per node of Simulator.getNodes() (nullptr: no pin), e.g. the parents of measuredRoutes.  The rows are the device's:
    // watchLinks still sets them, and what it set before is not restored over what was learnt.  false and lastError on a refusal.
    static rm_nbtable_params neighbourTableDefaults()
    {
        rm_nbtable_params p;
        rm_nbtable_defaults(&p);
        return p;
    }
    bool setNeighbourTable(const rm_nbtable_params *params)
    {
        lastError.clear();
        if (params && (!syncNodes() || !restoreLinkWatch())) return false;
        if ((params ? rm_nbtable_enable(ctx_, params) : rm_nbtable_disable(ctx_)) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool getNeighbourTable() const { return rm_nbtable_enabled(ctx_) != 0; }
    bool updateNeighbours(int64_t time, const std::vector<const Node *> &pinned = {})
    {
        lastError.clear();
        std::vector<int32_t> pin;
        if (!neighbourPins(pinned, pin)) return false;
        if (rm_nbtable_update(ctx_, 0, time, pinned.empty() ? nullptr : pin.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool expireNeighbours(int64_t time, const std::vector<const Node *> &pinned = {})
    {
        lastError.clear();
        std::vector<int32_t> pin;
        if (!neighbourPins(pinned, pin)) return false;
        if (rm_nbtable_expire(ctx_, time, pinned.empty() ? nullptr : pin.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // the node's counters; totals (may be nullptr); peers (may be nullptr): the node's K slots, nullptr for an empty one
    bool getNeighbourTableStatistics(const Node &node, rm_nbtable_node *out, rm_nbtable_totals *totals = nullptr, std::vector<Node *> *peers = nullptr)
    {
        lastError.clear();
        const int32_t i = node.index;
        if (!out || !simulator || !syncNodes()) return false;
        if (rm_nbtable_read(ctx_, &i, 1, out, totals) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        if (peers) {
            const int K = rm_linkstats_enabled(ctx_);
            std::vector<int32_t> row(size_t(K > 0 ? K : 0) + 1);
            if (K <= 0 || rm_linkstats_peers_get(ctx_, &i, 1, row.data()) != RM_OK) {
                lastError = K <= 0 ? "no watched-link statistics: setLinkWatch(K) comes first" : rm_last_error();
                return false;
            }
            const std::vector<Node *> &nodes = simulator->getNodes();
            peers->assign(size_t(K), nullptr);
            for (int k = 0; k < K; ++k)
                if (row[size_t(k)] >= 0 && size_t(row[size_t(k)]) < nodes.size() && row[size_t(k)] != i) (*peers)[size_t(k)] = nodes[size_t(row[size_t(k)])];
        }
        return true;
    }
    // Link estimator (extension E23): a smoothed ETX per watched neighbour, folded from windows of the watched links' counters and,
    // while the forwarding queues are on, of their acked / failed attempts toward the next hop.  setLinkWatch(K) comes first;
    // setLinkEstimator(&params) makes the tables for that K (nullptr: off; the watch tables stay); foldLinkEstimator() is one
    // fold over the medium's own tables as they stand; getLinkEstimates reads a node's K entries in slot order, and optionally its
    // data-step state, the totals and the peers the entries name (nullptr: an empty entry).  The estimate is also a watch table
    // of its own (linkEstimateTables, device pointers) for rm_etx_query_device.  false and lastError on a refusal.
    static rm_linkest_params linkEstimatorDefaults()
    {
        rm_linkest_params p;
        rm_linkest_defaults(&p);
        return p;
    }
    bool setLinkEstimator(const rm_linkest_params *params)
    {
        lastError.clear();
        if (!params) {
            if (rm_linkest_disable(ctx_) != RM_OK) {
                lastError = rm_last_error();
                return false;
            }
            return true;
        }
        if (!syncNodes() || !restoreLinkWatch()) return false;
        const int K = rm_linkstats_enabled(ctx_);
        if (K <= 0) {
            lastError = "setLinkEstimator: setLinkWatch(K) comes first";
            return false;
        }
        if (rm_linkest_enable(ctx_, int32_t(K), params) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    int getLinkEstimator() const { return rm_linkest_enabled(ctx_); } // K, or 0 while off
    bool foldLinkEstimator()
    {
        lastError.clear();
        if (!syncNodes()) return false;
        if (rm_linkest_fold(ctx_, nullptr) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool getLinkEstimates(const Node &node, std::vector<rm_linkest_entry> *entries, rm_linkest_node *state = nullptr, rm_linkest_totals *totals = nullptr,
                          std::vector<Node *> *peers = nullptr)
    {
        lastError.clear();
        if (!entries || !simulator || !syncNodes()) return false;
        const int K = rm_linkest_enabled(ctx_);
        entries->assign(size_t(K > 0 ? K : 0) + 1, rm_linkest_entry{}); // (one spare: never a NULL pointer)
        const int32_t i = node.index;
        rm_linkest_node st{};
        if (rm_linkest_read(ctx_, &i, 1, entries->data(), &st, totals) != RM_OK) {
            lastError = rm_last_error();
            entries->clear();
            return false;
        }
        entries->resize(size_t(K));
        if (state) *state = st;
        if (peers) {
            const std::vector<Node *> &nodes = simulator->getNodes();
            peers->assign(size_t(K), nullptr);
            for (int k = 0; k < K; ++k) {
                const int32_t q = (*entries)[size_t(k)].peer;
                if (q >= 0 && size_t(q) < nodes.size()) (*peers)[size_t(k)] = nodes[size_t(q)];
            }
        }
        return true;
    }
    bool linkEstimateTables(rm_etx_tables *out)
    {
        lastError.clear();
        if (rm_linkest_tables(ctx_, out) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // Did a frame reach the node it was addressed to (extension E12)?  One entry per packet of the LAST evaluated tick -- the tick
    // mode's flush, or transmitIfClear() -- in packet order: destinations[k] is packet k's intended receiver (nullptr: not asked).
    // status is RM_UC_*; link the index of the heard link in the tick's result (-1 without one); rssi and sinr as the result has
    // them (NaN without a link, sinr NaN on media without the SINR column).  Empty and lastError on a refusal.
    struct UnicastOutcome {
        int status;
        int link;
        double rssi, sinr;
    };
    std::vector<UnicastOutcome> unicastOutcomes(const std::vector<Node *> &destinations)
    {
        lastError.clear();
        const size_t n = destinations.size();
        std::vector<int32_t> want(n);
        for (size_t k = 0; k < n; ++k) want[k] = destinations[k] ? destinations[k]->index : -1;
        std::vector<uint8_t> status(n + 1);
        std::vector<int32_t> link(n + 1);
        std::vector<double> rssi(n + 1), sinr(n + 1);
        const rm_unicast_out out = {status.data(), link.data(), rssi.data(), sinr.data(), nullptr};
        const int32_t n_pkt = int32_t(n);
        if (rm_unicast_query(ctx_, 1, &n_pkt, want.data(), &out) != RM_OK) {
            lastError = rm_last_error();
            return {};
        }
        std::vector<UnicastOutcome> res(n);
        for (size_t k = 0; k < n; ++k) res[k] = UnicastOutcome{int(status[k]), int(link[k]), rssi[k], sinr[k]};
        return res;
    }
    std::string lastError;
    bool lastInterference = false;

protected:
    rm_model_params params_{};
    void apply()
    {
        if (rm_set_model(ctx_, &params_) != RM_OK) throw std::invalid_argument(rm_last_error());
        // (the traffic counters are the context's, not the medium's: a setting the medium made stays made)
        if (statistics_ && !rm_stats_enabled(ctx_) && rm_stats_enable(ctx_, 1) != RM_OK) {
            statistics_ = false;
            lastError = rm_last_error();
        }
        // (nor are the listening schedules: the engine keeps them over a change of the medium)
        restoreListenSchedules();
        // (nor are the watched links)
        restoreLinkWatch();
        // (nor are the traffic schedules)
        restoreTrafficSchedules();
    }
    // the traffic schedules the medium set, set again where the engine has dropped them (a node table of another size clears its
    // table), as far as their nodes still exist; false and lastError on a refusal
    bool restoreTrafficSchedules()
    {
        if (traffic_.empty() || rm_traffic_enabled(ctx_)) return true;
        std::vector<int32_t> idx;
        std::vector<rm_traffic_schedule> recs;
        const int32_t n = rm_node_count(ctx_);
        for (const auto &kv : traffic_)
            if (kv.first < n) {
                idx.push_back(kv.first);
                recs.push_back(kv.second);
            }
        if (!idx.empty() && rm_traffic_set(ctx_, idx.data(), int32_t(idx.size()), recs.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // K and the watch rows the medium set, set again where the engine has dropped them (a node table of another size switches the
    // feature off), as far as their nodes still exist; false and lastError on a refusal
    bool restoreLinkWatch()
    {
        if (linkWatchK_ <= 0 || rm_linkstats_enabled(ctx_) == linkWatchK_) return true;
        if (rm_linkstats_enable(ctx_, int32_t(linkWatchK_)) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        std::vector<int32_t> idx, rows;
        const int32_t n = rm_node_count(ctx_);
        for (const auto &kv : linkWatch_) {
            bool ok = kv.first < n;
            for (int32_t p : kv.second) ok = ok && p < n;
            if (!ok) continue;
            idx.push_back(kv.first);
            rows.insert(rows.end(), kv.second.begin(), kv.second.end());
        }
        if (!idx.empty() && rm_linkstats_watch(ctx_, idx.data(), int32_t(idx.size()), rows.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    // the pin array of updateNeighbours / expireNeighbours: empty, or one entry per node (nullptr: -1)
    bool neighbourPins(const std::vector<const Node *> &pinned, std::vector<int32_t> &pin)
    {
        if (!simulator || !syncNodes()) return false;
        if (!pinned.empty() && pinned.size() != simulator->getNodes().size()) {
            lastError = "neighbour tables: one pinned peer (or nullptr) per node, or none at all";
            return false;
        }
        for (const Node *nd : pinned) pin.push_back(nd ? nd->index : -1);
        return true;
    }
    // the schedules the medium set, set again where the engine has dropped them (a node table of another size clears its tables), as
    // far as their nodes still exist; false and lastError on a refusal
    bool restoreListenSchedules()
    {
        if (listen_.empty() || rm_listen_enabled(ctx_)) return true;
        std::vector<int32_t> idx;
        std::vector<rm_listen_schedule> recs;
        const int32_t n = rm_node_count(ctx_);
        for (const auto &kv : listen_)
            if (kv.first < n) {
                idx.push_back(kv.first);
                recs.push_back(kv.second);
            }
        if (!idx.empty() && rm_listen_set(ctx_, idx.data(), int32_t(idx.size()), recs.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        return true;
    }
    bool statistics_ = false; // what setStatistics set last, kept across apply()
    std::map<int32_t, rm_listen_schedule> listen_; // what setListenSchedule set, by node index, kept across apply()
    std::map<int32_t, rm_traffic_schedule> traffic_; // what setTrafficSchedule set, by node index, kept across apply()
    int linkWatchK_ = 0;                                // what setLinkWatch set last, kept across apply()
    std::map<int32_t, std::vector<int32_t>> linkWatch_; // what watchLinks set: K peers by node index, kept across apply()
    rm_context *ctx_ = nullptr;
    bool syncNodes() { return !simulator || sync(simulator, simulator->getNodes()); } // the device mirrors the node table first

private:
    bool sync(Simulator *sim, const std::vector<Node *> &nodes)
    {
        if (uploaded_ == sim->nodesVersion()) {
            for (int i : sim->takeChangedNodes()) { // the dirty list: only these nodes go to the device
                Node &nd = *nodes[size_t(i)];
                if (rm_node_update(ctx_, i, nd.getPosition().x, nd.getPosition().y, nd.getPosition().z,
                                   nd.getRadio().getTransmitPower(), nd.getRadio().getWirelessChannel(),
                                   nd.getRadio().isEnabled(), nd.getRadio().getRxProbability(),
                                   nd.getRadio().getTxProbability()) != RM_OK) {
                    lastError = rm_last_error();
                    uploaded_ = ~0ull; // the rest of the dirty list is gone with this call: a fresh snapshot next time
                    return false;
                }
            }
            return true;
        }
        (void)sim->takeChangedNodes(); // covered by the snapshot
        const size_t n = nodes.size();
        std::vector<double> x(n), y(n), z(n), tp(n), rp(n), xp(n);
        std::vector<int32_t> ch(n), id(n);
        std::vector<uint8_t> en(n);
        for (size_t i = 0; i < n; ++i) {
            Node &nd = *nodes[i];
            x[i] = nd.getPosition().x; y[i] = nd.getPosition().y; z[i] = nd.getPosition().z;
            tp[i] = nd.getRadio().getTransmitPower(); ch[i] = nd.getRadio().getWirelessChannel();
            en[i] = nd.getRadio().isEnabled(); rp[i] = nd.getRadio().getRxProbability();
            xp[i] = nd.getRadio().getTxProbability(); id[i] = nd.getIdAsInteger();
        }
        if (rm_nodes_upload(ctx_, int32_t(n), x.data(), y.data(), z.data(), tp.data(), ch.data(), en.data(), rp.data(),
                            xp.data(), id.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        dst_.resize(n + 1); verdict_.resize(n + 1); rssi_.resize(n + 1); sinr_.resize(n + 1);
        uploaded_ = sim->nodesVersion();
        return true;
    }
    std::vector<int32_t> chgNodes_, chgRecv_, chgChan_; // nodeInfoChanged: room for every node
    std::vector<double> chgRssi_;
    int kind_;
    bool tickMode_ = false, deviceEvents_ = false;
    std::vector<RadioPacket *> queue_;   // tick mode: transmit() calls since the last flush
    std::vector<RadioPacket *> inFlight_; // device events: packets with events still queued, by packet number (from inFlightHead_)
    std::vector<RadioPacket *> released_; // packets the medium has stopped referring to since the last takeReleased()
    size_t inFlightHead_ = 0;
    int64_t firstInFlight_ = 0;
    uint64_t uploaded_ = ~0ull;
    std::vector<int32_t> dst_;
    std::vector<uint8_t> verdict_;
    std::vector<double> rssi_, sinr_;
};

class NullRadioMedium : public GpuRadioMedium {
public:
    explicit NullRadioMedium(int device = 0) : GpuRadioMedium(RM_MODEL_NULL, device) {}
};

class UDGMRadioMedium : public GpuRadioMedium {
public:
    explicit UDGMRadioMedium(int device = 0) : GpuRadioMedium(RM_MODEL_UDGM, device) {}
    double getSuccessRatioTx() const { return params_.udgm_success_ratio_tx; }
    void setSuccessRatioTx(double v) { params_.udgm_success_ratio_tx = v; apply(); }
    double getSuccessRatioRx() const { return params_.udgm_success_ratio_rx; }
    void setSuccessRatioRx(double v) { params_.udgm_success_ratio_rx = v; apply(); }
    double getTransmissionRange() const { return params_.udgm_transmission_range; }
    void setTransmissionRange(double v) { params_.udgm_transmission_range = v; apply(); }
    double getInterferenceRange() const { return params_.udgm_interference_range; }
    void setInterferenceRange(double v) { params_.udgm_interference_range = v; apply(); }
};

class UDGMConstantLossRadioMedium : public GpuRadioMedium {
public:
    explicit UDGMConstantLossRadioMedium(int device = 0) : GpuRadioMedium(RM_MODEL_UDGM_CONST, device) {}
};

class N2NRadioMedium : public GpuRadioMedium {
public:
    explicit N2NRadioMedium(const std::vector<std::vector<double>> &m, int device = 0) : GpuRadioMedium(RM_MODEL_N2N, device)
    {
        setMatrix(m);
    }
    void setMatrix(const std::vector<std::vector<double>> &m)
    {
        // The reference bounds the source id by the number of rows and the destination id by THAT row's length
        // (N2NRadioMedium.java:28-37), anything outside gives probability 0 = unheard: a jagged matrix is the square
        // matrix of side max(rows, longest row) padded with zeros.
        size_t n = m.size();
        for (const auto &row : m) n = std::max(n, row.size());
        std::vector<double> flat(n * n, 0.0);
        for (size_t i = 0; i < m.size(); ++i)
            for (size_t j = 0; j < m[i].size(); ++j) flat[i * n + j] = m[i][j];
        if (rm_set_n2n_matrix(ctx_, int32_t(n), flat.data()) != RM_OK) throw std::invalid_argument(rm_last_error());
    }
};

// The build's extension medium behind the same contract (NOT a reference class): log-distance path
// loss, per-link log-normal shadowing, and with setSinr(true) co-channel SINR capture + half duplex over the frames on
// the air.  With SINR the verdicts of a tick's frames depend on each other: tick mode decides them against everything
// sent in the tick, the per-packet mode against what was sent before -- the reference media do not have this coupling.
class LogDistanceRadioMedium : public GpuRadioMedium {
public:
    explicit LogDistanceRadioMedium(int device = 0) : GpuRadioMedium(RM_MODEL_LOGDIST, device) {}
    rm_model_params &params() { return params_; } // change, then apply()
    void setSinr(bool on)
    {
        params_.flags = on ? (params_.flags | RM_LD_SINR) : (params_.flags & ~RM_LD_SINR);
        apply();
    }
    // (rm_set_model switches the frame error model off: a medium that has one sets it again after every change of its parameters --
    // and loses it, as the engine would refuse it, when the change takes the SINR extension away)
    void apply()
    {
        GpuRadioMedium::apply();
        if (errorModel_.kind != RM_EM_NONE && rm_set_error_model(ctx_, &errorModel_) != RM_OK) {
            errorModel_ = rm_error_model{};
            lastError = rm_last_error();
        }
    }
    // The neighbour query (extension E16): each listed node's K strongest potential links (1 <= K <= RM_NB_MAX_K), ranked by rssi,
    // ties by node index.  RM_NB_HEARD_BY: the receivers that hear the node best; RM_NB_HEARS: the transmitters it hears best, each
    // with its own txpower.  No list: all nodes in node order.  degree counts all potential links, not only the K listed.  Empty and
    // lastError on a refusal.
    struct NeighborRow {
        std::vector<Node *> peers; // at most K, strongest first
        std::vector<double> rssi;  // by the same index
        int degree;
    };
    std::vector<NeighborRow> neighbors(int direction, int K, const std::vector<const Node *> &nodes = {})
    {
        lastError.clear();
        if (!simulator || !syncNodes()) return {};
        const std::vector<Node *> &all = simulator->getNodes();
        std::vector<int32_t> idx;
        for (const Node *nd : nodes) idx.push_back(nd ? nd->index : -1);
        const size_t n = nodes.empty() ? all.size() : nodes.size();
        const size_t k = size_t(K > 0 ? K : 0);
        std::vector<int32_t> peer(n * k + 1), degree(n + 1);
        std::vector<double> rssi(n * k + 1);
        if (rm_neighbors_query(ctx_, int32_t(direction), int32_t(K), nodes.empty() ? nullptr : idx.data(), int32_t(n), peer.data(), rssi.data(),
                               degree.data()) != RM_OK) {
            lastError = rm_last_error();
            return {};
        }
        std::vector<NeighborRow> rows(n);
        for (size_t e = 0; e < n; ++e) {
            rows[e].degree = degree[e];
            for (size_t s = 0; s < k && peer[e * k + s] >= 0; ++s) {
                rows[e].peers.push_back(all[size_t(peer[e * k + s])]);
                rows[e].rssi.push_back(rssi[e * k + s]);
            }
        }
        return rows;
    }
    // The hop query (extension E17): hop count and best parent toward a set of roots over the potential links with rssi >= minRssi.
    // direction is the link between a node and its parent, seen from the node: RM_NB_HEARD_BY a collection tree, RM_NB_HEARS a
    // dissemination tree.  One row per node in node order; empty rows and lastError on a refusal.
    struct HopRow {
        int hop;      // -1: not reached
        Node *parent; // nullptr for a root and for a node that was not reached
        double rssi;  // the link to the parent, NaN without one
        int children;
    };
    struct HopTree {
        std::vector<HopRow> rows;
        rm_hops_totals totals;
    };
    HopTree hops(int direction, const std::vector<const Node *> &roots, double minRssi = -std::numeric_limits<double>::infinity())
    {
        lastError.clear();
        HopTree tree{{}, {0, -1, 0, 0}};
        if (!simulator || !syncNodes()) return tree;
        const std::vector<Node *> &all = simulator->getNodes();
        std::vector<int32_t> idx;
        for (const Node *nd : roots) idx.push_back(nd ? nd->index : -1);
        const size_t n = all.size();
        std::vector<int32_t> hop(n + 1), parent(n + 1), children(n + 1);
        std::vector<double> rssi(n + 1);
        const rm_hops_out out{hop.data(), parent.data(), rssi.data(), children.data()};
        if (rm_hops_query(ctx_, int32_t(direction), minRssi, idx.data(), int32_t(idx.size()), &out, &tree.totals) != RM_OK) {
            lastError = rm_last_error();
            tree.totals = {0, -1, 0, 0};
            return tree;
        }
        tree.rows.resize(n);
        for (size_t j = 0; j < n; ++j) tree.rows[j] = HopRow{hop[j], parent[j] >= 0 ? all[size_t(parent[j])] : nullptr, rssi[j], children[j]};
        return tree;
    }
    // The route query (extension E18): least path cost (ETX in units of 1/128) toward a set of roots over the potential links and
    // the parent on such a path.  params.direction is the link between a node and its parent, seen from the node.  One row per node
    // in node order; empty rows and lastError on a refusal.
    struct RouteRow {
        uint64_t cost; // RM_ROUTE_UNREACHED: not reached
        Node *parent;  // nullptr for a root and for a node that was not reached
        double rssi;   // the link to the parent, NaN without one
        uint32_t linkCost;
        int children;
    };
    struct RouteTree {
        std::vector<RouteRow> rows;
        rm_routes_totals totals;
    };
    static rm_routes_params routeParams(int direction, int kind = RM_EM_OQPSK_250K, double usPerBit = 4.0, int64_t airUs = 4064,
                                        double minRssi = -std::numeric_limits<double>::infinity(), uint32_t maxLinkCost = 1024)
    {
        return rm_routes_params{int32_t(direction), int32_t(kind), usPerBit, airUs, minRssi, maxLinkCost, 0};
    }
    RouteTree routes(const rm_routes_params &params, const std::vector<const Node *> &roots)
    {
        lastError.clear();
        RouteTree tree{{}, {0, 0, 0}};
        if (!simulator || !syncNodes()) return tree;
        const std::vector<Node *> &all = simulator->getNodes();
        std::vector<int32_t> idx;
        for (const Node *nd : roots) idx.push_back(nd ? nd->index : -1);
        const size_t n = all.size();
        std::vector<uint64_t> cost(n + 1);
        std::vector<int32_t> parent(n + 1), children(n + 1);
        std::vector<uint32_t> linkCost(n + 1);
        std::vector<double> rssi(n + 1);
        const rm_routes_out out{cost.data(), parent.data(), rssi.data(), linkCost.data(), children.data()};
        if (rm_routes_query(ctx_, &params, idx.data(), int32_t(idx.size()), &out, &tree.totals) != RM_OK) {
            lastError = rm_last_error();
            tree.totals = {0, 0, 0};
            return tree;
        }
        tree.rows.resize(n);
        for (size_t j = 0; j < n; ++j)
            tree.rows[j] = RouteRow{cost[j], parent[j] >= 0 ? all[size_t(parent[j])] : nullptr, rssi[j], linkCost[j], children[j]};
        return tree;
    }
    // Topology discovery into the watched links (E16 -> E14) without a link passing through the host: setLinkWatch(K) (K = 1, 2, 4
    // or 8), every node's RM_NB_HEARS row computed into the engine's staging block, taken as the watch rows on the device.  The
    // mirror then reads the rows back once, so that they survive apply() like rows set by watchLinks.  false and lastError on a refusal.
    bool watchStrongest(int K)
    {
        if (!simulator || !setLinkWatch(K)) return false;
        if (K <= 0) return true;
        const int32_t n = rm_node_count(ctx_);
        int32_t *rows = nullptr;
        if (rm_linkstats_stage_device(ctx_, &rows) != RM_OK || rm_neighbors_query_device(ctx_, RM_NB_HEARS, int32_t(K), nullptr, n, rows, nullptr, nullptr) != RM_OK ||
            rm_linkstats_watch_device(ctx_, nullptr, n, rows) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        std::vector<int32_t> host(size_t(n) * size_t(K));
        if (n > 0 && rm_linkstats_peers_get(ctx_, nullptr, n, host.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        linkWatch_.clear();
        for (int32_t i = 0; i < n; ++i) linkWatch_[i] = std::vector<int32_t>(host.begin() + size_t(i) * size_t(K), host.begin() + size_t(i + 1) * size_t(K));
        return true;
    }
    // The frame error model (extension E10; needs setSinr(true)): with RM_EM_OQPSK_250K a delivered link survives with the packet
    // success ratio of its SINR and its air time.  The verdicts come out of the engine, so transmit(), transmitIfClear(), the tick
    // mode and transmitCsmaBatch() deliver and interfere accordingly and their generateReceptionEvents calls carry the new verdict.
    // false and lastError on a refusal (the model the medium had stays).
    bool setErrorModel(int32_t kind, double us_per_bit = 4.0, uint64_t seed = 0)
    {
        rm_error_model e;
        rm_error_model_defaults(&e, kind);
        e.us_per_bit = us_per_bit;
        e.seed = seed;
        if (rm_set_error_model(ctx_, &e) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        errorModel_ = e;
        return true;
    }
    rm_error_model getErrorModel() const
    {
        rm_error_model e;
        if (rm_get_error_model(ctx_, &e) != RM_OK) rm_error_model_defaults(&e, RM_EM_NONE);
        return e;
    }
    // Clear-channel assessment / energy detection over the frames on the air (extension E5; needs setSinr(true)): the power in
    // dBm that `node` sees on its own channel at time_us -- the noise level when nothing counts; NaN and lastError on a refusal.
    // Transciever::getRSSI stays the reference's latched value.
    double getChannelEnergy(const Node &node, int64_t time_us)
    {
        double energy = std::nan("");
        const int32_t j = node.index;
        if (!syncNodes() || rm_channel_energy(ctx_, time_us, &j, 1, RM_CHANNEL_OWN, std::nan(""), &energy, nullptr) != RM_OK) {
            if (lastError.empty() || rm_last_error()[0]) lastError = rm_last_error();
            return std::nan("");
        }
        return energy;
    }
    // clear: the energy on the node's channel is below threshold_dbm (a refusal is not clear)
    bool isChannelClear(const Node &node, int64_t time_us, double threshold_dbm)
    {
        double energy = 0.0;
        uint8_t flags = 0;
        const int32_t j = node.index;
        if (!syncNodes() || rm_channel_energy(ctx_, time_us, &j, 1, RM_CHANNEL_OWN, threshold_dbm, &energy, &flags) != RM_OK) {
            if (lastError.empty() || rm_last_error()[0]) lastError = rm_last_error();
            return false;
        }
        return (flags & RM_ED_BUSY) == 0;
    }
    // Listen before talk for several nodes at once (extension E6; needs setSinr(true)): every listed node wants to send one packet
    // of hex_length characters starting at start_us; each senses its own channel at cca_time_us (<= start_us) on the device, and
    // only the ones that find it clear -- and are not on the air themselves -- transmit.  Returns the nodes' flags (0: sent,
    // else RM_ED_BUSY | RM_ED_TRANSMITTING: deferred); an empty vector and lastError on a refusal.  A sent packet generates its
    // events as transmit() does, a deferred one generates none.  The packets belong to the medium (sentIfClear()).  The medium's
    // own call order, not for the tick mode or the reception stage on the device.
    std::vector<uint8_t> transmitIfClear(const std::vector<Node *> &senders, int64_t start_us, int64_t hex_length, int64_t cca_time_us,
                                         double threshold_dbm)
    {
        lastError.clear();
        Simulator *sim = simulator;
        if (!sim) { lastError = "No simulator"; return {}; }
        if (!syncNodes()) return {};
        const std::vector<Node *> &nodes = sim->getNodes();
        rm_set_time(ctx_, sim->getTime());
        const int32_t n = int32_t(senders.size());
        std::vector<int32_t> src(senders.size());
        for (size_t i = 0; i < senders.size(); ++i) src[i] = senders[i] ? senders[i]->index : -1;
        std::vector<uint8_t> flags(senders.size(), 0);
        if (rm_tick_run_sources_cca(ctx_, cca_time_us, start_us, src.data(), n, start_us, rm_air_time_us(hex_length), cca_time_us,
                                    threshold_dbm, flags.data(), nullptr) != RM_OK) {
            lastError = rm_last_error();
            return {};
        }
        std::vector<uint32_t> off(senders.size() + 1, 0);
        uint32_t heard = 0;
        if (ccaDst_.empty()) { ccaDst_.resize(1024); ccaVerdict_.resize(1024); ccaRssi_.resize(1024); }
        for (int attempt = 0; attempt < 2; ++attempt) { // (the count comes back with the refusal of buffers that are too small)
            const int rc = rm_result_copy(ctx_, nullptr, ccaDst_.data(), ccaVerdict_.data(), ccaRssi_.data(), nullptr, uint32_t(ccaDst_.size()),
                                          &heard, nullptr, off.data());
            if (rc == RM_OK) break;
            if (attempt == 1 || heard <= ccaDst_.size()) { lastError = rm_last_error(); return {}; }
            ccaDst_.resize(heard); ccaVerdict_.resize(heard); ccaRssi_.resize(heard);
        }
        const std::string data(size_t(hex_length), '0');
        for (size_t i = 0; i < senders.size(); ++i) {
            if (src[i] < 0 || flags[i]) continue;
            ccaSent_.emplace_back(new RadioPacket(senders[i], start_us, data));
            RadioPacket &packet = *ccaSent_.back();
            sim->generateTransmissionEvents(packet);
            for (uint32_t k = off[i]; k < off[i + 1]; ++k)
                sim->generateReceptionEvents(packet, nodes[size_t(ccaDst_[k])], ccaRssi_[k], ccaVerdict_[k] == RM_DELIVERED);
        }
        return flags;
    }
    const std::vector<std::unique_ptr<RadioPacket>> &sentIfClear() const { return ccaSent_; }
    // The same across a batch of ticks (extension E7): tick b's senders want to start at start_us[b] and sense at cca_time_us[b]
    // (t_begin_us[b] <= cca_time_us[b] <= start_us[b]); a tick senses the window plus the KEPT frames of the ticks before it.
    // Returns the flags per tick (empty and lastError on a refusal); receptions are generated from the result slots.
    std::vector<std::vector<uint8_t>> transmitIfClearBatch(const std::vector<std::vector<Node *>> &senders, const std::vector<int64_t> &t_begin_us,
                                                           const std::vector<int64_t> &start_us, int64_t hex_length,
                                                           const std::vector<int64_t> &cca_time_us, double threshold_dbm)
    {
        lastError.clear();
        Simulator *sim = simulator;
        if (!sim) { lastError = "No simulator"; return {}; }
        const size_t nt = senders.size();
        if (nt == 0 || t_begin_us.size() != nt || start_us.size() != nt || cca_time_us.size() != nt) { lastError = "one entry per tick"; return {}; }
        if (!syncNodes()) return {};
        const std::vector<Node *> &nodes = sim->getNodes();
        rm_set_time(ctx_, sim->getTime());
        std::vector<std::vector<int32_t>> src(nt);
        std::vector<const int32_t *> lists(nt);
        std::vector<int32_t> n_src(nt);
        std::vector<int64_t> air(nt, rm_air_time_us(hex_length));
        size_t total = 0;
        for (size_t b = 0; b < nt; ++b) {
            src[b].resize(senders[b].size());
            for (size_t i = 0; i < senders[b].size(); ++i) src[b][i] = senders[b][i] ? senders[b][i]->index : -1;
            lists[b] = src[b].data();
            n_src[b] = int32_t(src[b].size());
            total += src[b].size();
        }
        std::vector<uint8_t> flat(std::max<size_t>(total, 1), 0);
        if (rm_batch_run_sources_cca(ctx_, int32_t(nt), t_begin_us.data(), start_us.data(), lists.data(), n_src.data(), start_us.data(), air.data(),
                                     cca_time_us.data(), threshold_dbm, flat.data(), nullptr) != RM_OK) {
            lastError = rm_last_error();
            return {};
        }
        std::vector<std::vector<uint8_t>> flags(nt);
        if (ccaDst_.empty()) { ccaDst_.resize(1024); ccaVerdict_.resize(1024); ccaRssi_.resize(1024); }
        const std::string data(size_t(hex_length), '0');
        size_t at = 0;
        for (size_t b = 0; b < nt; ++b) {
            flags[b].assign(flat.begin() + at, flat.begin() + at + src[b].size());
            at += src[b].size();
            std::vector<uint32_t> off(src[b].size() + 1, 0);
            uint32_t heard = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                const int rc = rm_batch_result_copy(ctx_, int32_t(b), nullptr, ccaDst_.data(), ccaVerdict_.data(), ccaRssi_.data(), nullptr,
                                                    uint32_t(ccaDst_.size()), &heard, nullptr, off.data());
                if (rc == RM_OK) break;
                if (attempt == 1 || heard <= ccaDst_.size()) { lastError = rm_last_error(); return {}; }
                ccaDst_.resize(heard); ccaVerdict_.resize(heard); ccaRssi_.resize(heard);
            }
            for (size_t i = 0; i < src[b].size(); ++i) {
                if (src[b][i] < 0 || flags[b][i]) continue;
                ccaSent_.emplace_back(new RadioPacket(senders[b][i], start_us[b], data));
                RadioPacket &packet = *ccaSent_.back();
                sim->generateTransmissionEvents(packet);
                for (uint32_t k = off[i]; k < off[i + 1]; ++k)
                    sim->generateReceptionEvents(packet, nodes[size_t(ccaDst_[k])], ccaRssi_[k], ccaVerdict_[k] == RM_DELIVERED);
            }
        }
        return flags;
    }
    // The CSMA-CA schedule of a batch (extension E8), on the host alone: the expanded lists' lengths, and per expanded slot in tick
    // order its packet (flat index over the ticks' own lists) and attempt number.  false and lastError on a refusal.
    struct CsmaSchedule {
        std::vector<int32_t> n_exp, origin;
        std::vector<uint8_t> attempt;
    };
    bool csmaSchedule(const rm_csma_params &p, const std::vector<int32_t> &n_src, const std::vector<int64_t> &cca_time_us, CsmaSchedule &out)
    {
        lastError.clear();
        if (n_src.empty() || n_src.size() != cca_time_us.size()) { lastError = "one entry per tick"; return false; }
        out.n_exp.assign(n_src.size(), 0);
        int64_t total = 0;
        if (rm_csma_schedule(&p, int32_t(n_src.size()), n_src.data(), cca_time_us.data(), out.n_exp.data(), nullptr, nullptr, 0, &total) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        out.origin.assign(size_t(total) + 1, 0);
        out.attempt.assign(size_t(total) + 1, 0);
        if (rm_csma_schedule(&p, int32_t(n_src.size()), n_src.data(), cca_time_us.data(), out.n_exp.data(), out.origin.data(), out.attempt.data(),
                             total, &total) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        out.origin.resize(size_t(total));
        out.attempt.resize(size_t(total));
        return true;
    }
    // Listen before talk with retries across a batch of ticks (extension E8): as transmitIfClearBatch, but a sender that defers
    // backs off and senses again in a later tick of the batch (rm_csma_params), up to max_backoffs times.  Returns one entry per
    // sender in tick order (empty and lastError on a refusal); a packet that was sent starts at the start_us of the tick it was
    // sent in, and generates its events there, in the order of that tick's expanded list.
    struct CsmaOutcome {
        uint8_t status, attempts, flags; // RM_CSMA_*, attempts made, RM_ED_* of the last one
        int32_t tick, pkt;               // sent: the tick and the position in its expanded list; pending: the tick of the next attempt
    };
    std::vector<CsmaOutcome> transmitCsmaBatch(const std::vector<std::vector<Node *>> &senders, const std::vector<int64_t> &t_begin_us,
                                               const std::vector<int64_t> &start_us, int64_t hex_length, const std::vector<int64_t> &cca_time_us,
                                               double threshold_dbm, const rm_csma_params &p)
    {
        std::vector<rm_csma_carry> none;
        return transmitCsmaBatch(senders, t_begin_us, start_us, hex_length, cca_time_us, threshold_dbm, p, {}, none);
    }
    // The same with a carry (extension E9): carry_in are the senders an earlier batch left pending (its carry_out), which go on
    // with their next attempt in this batch; carry_out receives the senders this batch leaves pending, for the next one, whose
    // tick 0 is the tick after this batch's last.  Consecutive batches chained this way make the calls of one batch over all
    // their ticks.  carried (may be NULL): one entry per carried sender, attempts counting those of the earlier batches.
    std::vector<CsmaOutcome> transmitCsmaBatch(const std::vector<std::vector<Node *>> &senders, const std::vector<int64_t> &t_begin_us,
                                               const std::vector<int64_t> &start_us, int64_t hex_length, const std::vector<int64_t> &cca_time_us,
                                               double threshold_dbm, const rm_csma_params &p, const std::vector<rm_csma_carry> &carry_in,
                                               std::vector<rm_csma_carry> &carry_out, std::vector<CsmaOutcome> *carried = nullptr)
    {
        lastError.clear();
        carry_out.clear();
        if (carried) carried->clear();
        Simulator *sim = simulator;
        if (!sim) { lastError = "No simulator"; return {}; }
        const size_t nt = senders.size();
        if (nt == 0 || t_begin_us.size() != nt || start_us.size() != nt || cca_time_us.size() != nt) { lastError = "one entry per tick"; return {}; }
        if (!syncNodes()) return {};
        const std::vector<Node *> &nodes = sim->getNodes();
        rm_set_time(ctx_, sim->getTime());
        std::vector<std::vector<int32_t>> src(nt);
        std::vector<const int32_t *> lists(nt);
        std::vector<int32_t> n_src(nt), n_exp(nt, 0);
        std::vector<int64_t> air(nt, rm_air_time_us(hex_length));
        std::vector<Node *> flat;
        for (size_t b = 0; b < nt; ++b) {
            src[b].resize(senders[b].size());
            for (size_t i = 0; i < senders[b].size(); ++i) src[b][i] = senders[b][i] ? senders[b][i]->index : -1;
            lists[b] = src[b].data();
            n_src[b] = int32_t(src[b].size());
            flat.insert(flat.end(), senders[b].begin(), senders[b].end());
        }
        // the carried senders are packets total .. of the same arrays
        const size_t total = flat.size(), nc = carry_in.size(), all = total + nc;
        for (const rm_csma_carry &c : carry_in) {
            if (c.node < 0 || size_t(c.node) >= nodes.size()) { lastError = "a carried sender is not a node"; return {}; }
            flat.push_back(nodes[size_t(c.node)]);
        }
        std::vector<uint8_t> status(all + 2, 0), attempts(all + 2, 0), flags(all + 2, 0);
        std::vector<int32_t> tick(all + 2, -1), pkt(all + 2, -1);
        const rm_csma_result res = {status.data(), attempts.data(), tick.data(), pkt.data(), flags.data(), nullptr};
        const size_t at = total + 1;
        const rm_csma_result res_c = {status.data() + at, attempts.data() + at, tick.data() + at, pkt.data() + at, flags.data() + at, nullptr};
        if (rm_batch_run_sources_csma_carry(ctx_, int32_t(nt), t_begin_us.data(), start_us.data(), lists.data(), n_src.data(), start_us.data(),
                                            air.data(), cca_time_us.data(), threshold_dbm, &p, &res, n_exp.data(), carry_in.data(), int32_t(nc),
                                            &res_c) != RM_OK) {
            lastError = rm_last_error();
            return {};
        }
        carry_out.resize(all + 1);
        int64_t n_out = 0;
        if (rm_csma_carry_collect(int32_t(nt), lists.data(), n_src.data(), cca_time_us.data(), carry_in.data(), int32_t(nc), &res, &res_c,
                                  carry_out.data(), int64_t(all), &n_out) != RM_OK) {
            lastError = rm_last_error();
            carry_out.clear();
            return {};
        }
        carry_out.resize(size_t(n_out));
        std::vector<CsmaOutcome> out(total);
        std::vector<std::vector<std::pair<int32_t, size_t>>> sent(nt); // per tick: (position in the expanded list, packet)
        for (size_t o = 0; o < all; ++o) {
            const size_t e = o < total ? o : o + 1;
            const CsmaOutcome one{status[e], attempts[e], flags[e], tick[e], pkt[e]};
            if (o < total) out[o] = one;
            else if (carried) carried->push_back(one);
            if (one.status == RM_CSMA_SENT) sent[size_t(one.tick)].emplace_back(one.pkt, o);
        }
        if (ccaDst_.empty()) { ccaDst_.resize(1024); ccaVerdict_.resize(1024); ccaRssi_.resize(1024); }
        const std::string data(size_t(hex_length), '0');
        for (size_t b = 0; b < nt; ++b) {
            std::sort(sent[b].begin(), sent[b].end());
            std::vector<uint32_t> off(size_t(n_exp[b]) + 1, 0);
            uint32_t heard = 0;
            for (int attempt = 0; attempt < 2; ++attempt) {
                const int rc = rm_batch_result_copy(ctx_, int32_t(b), nullptr, ccaDst_.data(), ccaVerdict_.data(), ccaRssi_.data(), nullptr,
                                                    uint32_t(ccaDst_.size()), &heard, nullptr, off.data());
                if (rc == RM_OK) break;
                if (attempt == 1 || heard <= ccaDst_.size()) { lastError = rm_last_error(); return {}; }
                ccaDst_.resize(heard); ccaVerdict_.resize(heard); ccaRssi_.resize(heard);
            }
            for (const std::pair<int32_t, size_t> &q : sent[b]) {
                ccaSent_.emplace_back(new RadioPacket(flat[q.second], start_us[b], data));
                RadioPacket &packet = *ccaSent_.back();
                sim->generateTransmissionEvents(packet);
                for (uint32_t k = off[size_t(q.first)]; k < off[size_t(q.first) + 1]; ++k)
                    sim->generateReceptionEvents(packet, nodes[size_t(ccaDst_[k])], ccaRssi_[k], ccaVerdict_[k] == RM_DELIVERED);
            }
        }
        return out;
    }

    // The same after transmitCsmaBatch() (extension E12): entry k asks for the packet of outcomes[k] -- the tick it was sent in and
    // its position there -- at destinations[k]; a packet that was not sent (failed, pending, padding) gives RM_UC_NONE.  Ask before
    // the next evaluating call of the medium.
    using GpuRadioMedium::unicastOutcomes;
    std::vector<UnicastOutcome> unicastOutcomes(const std::vector<CsmaOutcome> &outcomes, const std::vector<Node *> &destinations)
    {
        lastError.clear();
        const size_t n = outcomes.size();
        if (destinations.size() != n) { lastError = "one destination per outcome"; return {}; }
        std::vector<int32_t> slot(n + 1), pkt(n + 1), want(n + 1), link(n + 1);
        for (size_t k = 0; k < n; ++k) {
            const bool sent = outcomes[k].status == RM_CSMA_SENT;
            slot[k] = sent ? outcomes[k].tick : -1;
            pkt[k] = sent ? outcomes[k].pkt : -1;
            want[k] = destinations[k] ? destinations[k]->index : -1;
        }
        std::vector<uint8_t> status(n + 1);
        std::vector<double> rssi(n + 1), sinr(n + 1);
        const rm_unicast_out out = {status.data(), link.data(), rssi.data(), sinr.data(), nullptr};
        if (rm_unicast_query_at(ctx_, int64_t(n), slot.data(), pkt.data(), want.data(), &out) != RM_OK) {
            lastError = rm_last_error();
            return {};
        }
        std::vector<UnicastOutcome> res(n);
        for (size_t k = 0; k < n; ++k) res[k] = UnicastOutcome{int(status[k]), int(link[k]), rssi[k], sinr[k]};
        return res;
    }

private:
    rm_error_model errorModel_{}; // what setErrorModel set last (RM_EM_NONE: none), kept across apply()
    std::vector<std::unique_ptr<RadioPacket>> ccaSent_;
    std::vector<int32_t> ccaDst_;
    std::vector<uint8_t> ccaVerdict_;
    std::vector<double> ccaRssi_;
};

// The same contract over SEVERAL devices (or several partitions of one device): one rm_group behind one medium
// object, because the reference host is one process (Main.java:65-73).  The receivers are range-partitioned over the
// members; a packet is handed to every member, the members' heard links come back merged in node order, and the
// medium makes the calls of the single-device media.
class GroupRadioMedium : public AbstractRadioMedium {
public:
    GroupRadioMedium(int kind, const std::vector<int32_t> &devices) : kind_(kind)
    {
        if (rm_group_create(int32_t(devices.size()), devices.data(), &grp_) != RM_OK)
            throw std::runtime_error(std::string("no MI355X radio medium group: ") + rm_last_error());
        rm_model_defaults(&params_, kind);
        apply();
    }
    ~GroupRadioMedium() override { rm_group_destroy(grp_); }
    GroupRadioMedium(const GroupRadioMedium &) = delete;
    GroupRadioMedium &operator=(const GroupRadioMedium &) = delete;

    std::string getName() override { return rm_get_name(rm_group_context(grp_, 0)); }
    void setSimulator(Simulator *sim) override
    {
        simulator = sim;
        if (sim) rm_group_seed(grp_, sim->getRandomSeed());
        uploaded_ = ~0ull;
    }
    rm_model_params &params() { return params_; } // change, then apply()
    void apply()
    {
        if (rm_group_set_model(grp_, &params_) != RM_OK) throw std::invalid_argument(rm_last_error());
    }
    void setMatrix(const std::vector<std::vector<double>> &m) // N2NRadioMedium(double[][]): jagged rows as a zero-padded square
    {
        size_t side = m.size();
        for (const auto &row : m) side = std::max(side, row.size());
        std::vector<double> flat(side * side, 0.0);
        for (size_t i = 0; i < m.size(); ++i)
            for (size_t j = 0; j < m[i].size(); ++j) flat[i * side + j] = m[i][j];
        if (rm_group_set_n2n_matrix(grp_, int32_t(side), flat.data()) != RM_OK) throw std::invalid_argument(rm_last_error());
    }
    void transmit(RadioPacket &packet) override
    {
        lastError.clear();
        Simulator *sim = simulator;
        if (!sim) { lastError = "No simulator"; return; }
        const std::vector<Node *> &nodes = sim->getNodes();
        if (!sync(sim, nodes)) return;
        rm_group_set_time(grp_, sim->getTime());
        const double txp = packet.getTransmitPower();
        const int32_t ch = packet.getWirelessChannel();
        uint32_t heard = 0;
        uint8_t interference = 0;
        int rc = rm_group_tick_begin(grp_, packet.getStartTime(), packet.getStartTime());
        if (rc == RM_OK) rc = rm_group_enqueue_tx(grp_, packet.getSource()->index, packet.getStartTime(), packet.getPacketAirTime(), &txp, &ch);
        if (rc == RM_OK)
            rc = rm_group_tick_flush(grp_, nullptr, dst_.data(), verdict_.data(), rssi_.data(), nullptr, uint32_t(dst_.size()), &heard,
                                     &interference, nullptr);
        if (rc != RM_OK) { lastError = rm_last_error(); return; }
        if (kind_ != RM_MODEL_UDGM_CONST) sim->generateTransmissionEvents(packet);
        for (uint32_t i = 0; i < heard; ++i) {
            Node *node = nodes[size_t(dst_[i])];
            if (kind_ == RM_MODEL_UDGM_CONST) sim->deliverRadioPacket(packet, node, rssi_[i]);
            else sim->generateReceptionEvents(packet, node, rssi_[i], verdict_[i] == RM_DELIVERED);
        }
    }
    std::string lastError;

private:
    bool sync(Simulator *sim, const std::vector<Node *> &nodes)
    {
        if (uploaded_ == sim->nodesVersion()) {
            for (int i : sim->takeChangedNodes()) {
                Node &nd = *nodes[size_t(i)];
                if (rm_group_node_update(grp_, i, nd.getPosition().x, nd.getPosition().y, nd.getPosition().z, nd.getRadio().getTransmitPower(),
                                         nd.getRadio().getWirelessChannel(), nd.getRadio().isEnabled(), nd.getRadio().getRxProbability(),
                                         nd.getRadio().getTxProbability()) != RM_OK) {
                    lastError = rm_last_error();
                    return false;
                }
            }
            return true;
        }
        (void)sim->takeChangedNodes();
        const size_t n = nodes.size();
        std::vector<double> x(n), y(n), z(n), tp(n), rp(n), xp(n);
        std::vector<int32_t> ch(n), id(n);
        std::vector<uint8_t> en(n);
        for (size_t i = 0; i < n; ++i) {
            Node &nd = *nodes[i];
            x[i] = nd.getPosition().x; y[i] = nd.getPosition().y; z[i] = nd.getPosition().z;
            tp[i] = nd.getRadio().getTransmitPower(); ch[i] = nd.getRadio().getWirelessChannel();
            en[i] = nd.getRadio().isEnabled(); rp[i] = nd.getRadio().getRxProbability();
            xp[i] = nd.getRadio().getTxProbability(); id[i] = nd.getIdAsInteger();
        }
        if (rm_group_nodes_upload(grp_, int32_t(n), x.data(), y.data(), z.data(), tp.data(), ch.data(), en.data(), rp.data(), xp.data(),
                                  id.data()) != RM_OK) {
            lastError = rm_last_error();
            return false;
        }
        dst_.resize(n + 1); verdict_.resize(n + 1); rssi_.resize(n + 1);
        uploaded_ = sim->nodesVersion();
        return true;
    }
    int kind_;
    rm_group *grp_ = nullptr;
    rm_model_params params_{};
    uint64_t uploaded_ = ~0ull;
    std::vector<int32_t> dst_;
    std::vector<uint8_t> verdict_;
    std::vector<double> rssi_;
};


// ---- packet traces ----------------------------------------------------
// util/PcapExporter.java:47-91: classic pcap, every field written big-endian by DataOutputStream:
// magic 0xa1b2c3d4, version 2.4, thiszone 0, sigfigs 0, snaplen 4096, network 195
// (LINKTYPE_IEEE802_15_4); per packet ts_sec = time / 1e6, ts_usec = time % 1e6 (time in
// microseconds, truncated to int as in the reference), incl_len = orig_len = data length, the bytes.
class PcapExporter {
public:
    ~PcapExporter() { closePcap(); }
    void openPcap(const std::string &pcapFile)
    {
        closePcap();
        out_ = std::fopen(pcapFile.c_str(), "wb");
        if (!out_) throw std::runtime_error("cannot open " + pcapFile);
        writeInt(0xa1b2c3d4u);
        writeShort(0x0002);
        writeShort(0x0004);
        writeInt(0);
        writeInt(0);
        writeInt(4096);
        writeInt(195);
        std::fflush(out_);
    }
    void closePcap()
    {
        if (out_) std::fclose(out_);
        out_ = nullptr;
    }
    bool isOpen() const { return out_ != nullptr; }
    void exportPacketData(int64_t time, const std::vector<uint8_t> &data)
    {
        if (!out_) throw std::runtime_error("pcap file never set"); // the reference opens "radiolog-<millis>.pcap" here
        writeInt(uint32_t(int32_t(time / 1000000)));
        writeInt(uint32_t(int32_t(time % 1000000)));
        writeInt(uint32_t(data.size()));
        writeInt(uint32_t(data.size()));
        if (!data.empty()) std::fwrite(data.data(), 1, data.size(), out_);
        std::fflush(out_);
    }

private:
    void writeInt(uint32_t v)
    {
        const uint8_t b[4] = {uint8_t(v >> 24), uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)};
        std::fwrite(b, 1, 4, out_);
    }
    void writeShort(uint16_t v)
    {
        const uint8_t b[2] = {uint8_t(v >> 8), uint8_t(v)};
        std::fwrite(b, 1, 2, out_);
    }
    std::FILE *out_ = nullptr;
};

// util/PcapListener.java:40-58
class PcapListener : public RadioListener {
public:
    explicit PcapListener(const std::string &file) { exporter.openPcap(file); }
    void packetTransmission(RadioPacket &packet) override
    {
        exporter.exportPacketData(packet.getStartTime(), packet.getPacketDataAsBytes());
    }
    PcapExporter exporter;
};

// A pcap file does not say which node sent a frame, so it cannot be replayed.  The compact trace is
// what a replay needs and nothing else: a 16-byte header ("RMTRACE1", record count) and one
// little-endian 32-byte record per transmission, in call order:
//   int64 time_us | int32 source node index | int32 hex length | float64 rf-power | int32 channel | int32 0
// radio-sim_amd/trace.py reads it back and feeds whole ticks of it to rm_batch_run_device.
class TraceListener : public RadioListener {
public:
    explicit TraceListener(const std::string &file) : out_(std::fopen(file.c_str(), "wb"))
    {
        if (!out_) throw std::runtime_error("cannot open " + file);
        writeHeader();
    }
    ~TraceListener() { close(); }
    void packetTransmission(RadioPacket &p) override
    {
        struct Rec {
            int64_t time;
            int32_t src, hexLength;
            double power;
            int32_t channel, zero;
        } r = {p.getStartTime(), int32_t(p.getSource()->index), int32_t(p.getPacketDataAsHex().size()), p.getTransmitPower(),
               int32_t(p.getWirelessChannel()), 0};
        static_assert(sizeof(Rec) == 32, "trace record layout");
        std::fwrite(&r, sizeof(r), 1, out_);
        ++count_;
    }
    void close()
    {
        if (!out_) return;
        std::fseek(out_, 0, SEEK_SET);
        writeHeader();
        std::fclose(out_);
        out_ = nullptr;
    }

private:
    void writeHeader()
    {
        std::fwrite("RMTRACE1", 1, 8, out_);
        std::fwrite(&count_, sizeof(count_), 1, out_);
    }
    std::FILE *out_;
    uint64_t count_ = 0;
};

} // namespace emul8
