// rm_ncpool.hpp -- the heard-form source cache shared among a device's contexts: the 64-bit entry a node has
// in a pool, and the host's registry of pools -- key, attach, detach, the epoch rule.  Plain C++: no HIP call and no HIP type in
// here, so a stand-alone host program can drive it (tests/cpp/ncpool_host_san_test.cpp); what a pool owns on the device is the
// template's Payload (rm_host.hpp: NcPoolMem), and whatever has to happen on a stream happens in the caller's callbacks.
#pragma once

#include <stdint.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define RM_NC_HD __host__ __device__ inline
#else
#define RM_NC_HD inline
#endif

namespace rm {

// ---- the entry: ONE word per node says whether the node's list is valid AND where it lies, so that a reader on another stream
// can never pair one list's validity with another's place.  (epoch << 1 | valid) : 26, off : 27, len : 11.
constexpr int kNcWordBits = 26, kNcOffBits = 27, kNcLenBits = 11;
constexpr uint32_t kNcEpochMax = (1u << (kNcWordBits - 1)) - 1u;  // the last epoch a word can name; the host zeroes the entries before it wraps
constexpr uint64_t kNcArenaMax = uint64_t(1) << kNcOffBits;       // arena entries at most: every offset of a list with entries fits
static_assert(kNcWordBits + kNcOffBits + kNcLenBits == 64, "one 64-bit entry");

RM_NC_HD uint64_t nc_entry_pack(uint32_t word, uint32_t off, uint32_t len)
{
    return (uint64_t(word & ((1u << kNcWordBits) - 1u)) << (kNcOffBits + kNcLenBits)) | (uint64_t(off & ((1u << kNcOffBits) - 1u)) << kNcLenBits) |
           uint64_t(len & ((1u << kNcLenBits) - 1u));
}
RM_NC_HD uint32_t nc_entry_word(uint64_t e) { return uint32_t(e >> (kNcOffBits + kNcLenBits)); }
RM_NC_HD uint32_t nc_entry_off(uint64_t e) { return uint32_t(e >> kNcLenBits) & ((1u << kNcOffBits) - 1u); }
RM_NC_HD uint32_t nc_entry_len(uint64_t e) { return uint32_t(e) & ((1u << kNcLenBits) - 1u); }

} // namespace rm

namespace rmh {

// Everything a finished heard record depends on: the device the pool's memory lies on, the node table, the medium.  (The fill
// takes the ordered records directly behind the reorder stage, before the error model, the listening schedules, the statistics
// or the link statistics look at them: none of those is part of the key.)
struct NcPoolKey {
    int device = -1;
    int n = 0;
    uint64_t digest = 0;               // rm_table_digest: compared first
    std::vector<uint64_t> medium;      // kind, flags, every parameter's bits, the seed
    std::vector<unsigned char> table;  // the host's node columns, byte for byte: compared last
    bool operator==(const NcPoolKey &o) const
    {
        return device == o.device && n == o.n && digest == o.digest && medium == o.medium && table.size() == o.table.size() &&
               (table.empty() || std::memcmp(table.data(), o.table.data(), table.size()) == 0);
    }
};

template <class Payload> struct NcPool {
    NcPoolKey key;
    int refs = 0;            // attached contexts
    uint32_t epoch = 0;      // of the lists in `mem` (1 ..; rm::kNcEpochMax at most)
    uint64_t epochs = 0;     // begun since the pool was made (report)
    Payload mem;
};

// The process-wide registry.  Every function takes the one mutex for all it does, the callbacks included, so a context that
// joins a pool finds its memory allocated and the last epoch's resets issued (and recorded: Payload carries the event).
// Rules: a pool begins a new epoch only while exactly one context is attached, and it leaves the registry -- its memory is the
// caller's to free -- with its last context.  Nothing outlives the last context of a table.
template <class Payload> class NcRegistry {
public:
    using Pool = NcPool<Payload>;
    enum Change { kStay, kNewEpoch, kLeft };

    // Join a live pool whose key equals `key`, or make one.  A new pool: make(pool) allocates (false: nothing is kept, nullptr
    // comes back) and the first epoch begins: epoch(pool, true).  `joined`: the pool had other contexts attached.
    template <class Make, class Epoch> Pool *attach(NcPoolKey &&key, Make make, Epoch epoch, bool *joined)
    {
        std::lock_guard<std::mutex> g(mu_);
        for (auto &p : pools_)
            if (p->key == key) {
                p->refs++;
                if (joined) *joined = true;
                return p.get();
            }
        if (joined) *joined = false;
        std::unique_ptr<Pool> p(new Pool());
        p->key = std::move(key);
        if (!make(*p)) return nullptr;
        p->refs = 1;
        begin_epoch(*p, epoch, true);
        pools_.push_back(std::move(p));
        return pools_.back().get();
    }

    // The attached context's table, medium or engine order has changed; `key` is what it has now.
    //   alone in the pool: the pool takes the key and begins a new epoch (kNewEpoch), as a context's private cache did;
    //   sharing it, same key (the change was none the records depend on): nothing (kStay);
    //   sharing it, another key: the context leaves (kLeft; `key` is untouched: the caller attaches with it).
    template <class Epoch> Change changed(Pool *p, NcPoolKey &key, Epoch epoch)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (p->refs == 1) {
            p->key = std::move(key);
            begin_epoch(*p, epoch, false);
            return kNewEpoch;
        }
        if (p->key == key) return kStay;
        p->refs--;
        return kLeft;
    }

    // true: that was the pool's last context -- it has left the registry and is the caller's (free its memory, delete it)
    bool detach(Pool *p)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (--p->refs > 0) return false;
        for (size_t i = 0; i < pools_.size(); ++i)
            if (pools_[i].get() == p) {
                (void)pools_[i].release();
                pools_.erase(pools_.begin() + long(i));
                break;
            }
        return true;
    }

    // (reports and tests) a consistent look at a pool's counters
    void look(const Pool *p, int *refs, uint32_t *epoch, uint64_t *epochs)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (refs) *refs = p->refs;
        if (epoch) *epoch = p->epoch;
        if (epochs) *epochs = p->epochs;
    }
    size_t live()
    {
        std::lock_guard<std::mutex> g(mu_);
        return pools_.size();
    }

private:
    // epoch(pool, zero_entries): the caller's resets -- the bump counter, and every entry where the epoch's number starts over
    template <class Epoch> void begin_epoch(Pool &p, Epoch &epoch, bool fresh)
    {
        bool zero = fresh;
        if (p.epoch >= rm::kNcEpochMax) {
            p.epoch = 0;
            zero = true;
        }
        p.epoch++;
        p.epochs++;
        epoch(p, zero);
    }
    std::mutex mu_;
    std::vector<std::unique_ptr<Pool>> pools_;
};

} // namespace rmh
