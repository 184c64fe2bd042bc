// ncpool_host_san_test.cpp -- the host logic of the shared heard-form cache (rm_ncpool.hpp) in a stand-alone program under the
// host sanitizers: the 64-bit entry's pack and unpack at its field limits, and the registry's key, attach, detach and epoch rule
// driven from several host threads.  No device: a pool's payload here is a plain struct that the callbacks count in.
#include "rm_ncpool.hpp"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

namespace {

struct Mem {
    int made = 0;        // make() calls (1 for a live pool)
    int resets = 0;      // epoch callbacks
    int zeroed = 0;      // ... that zeroed the entries
    int refs_at_reset_max = 0;
};
using Registry = rmh::NcRegistry<Mem>;
using Pool = rmh::NcPool<Mem>;

std::atomic<long> g_made{0}, g_freed{0}, g_shared_epoch{0};

rmh::NcPoolKey key_of(int device, int n, uint64_t digest, uint64_t seed, unsigned char moved = 0)
{
    rmh::NcPoolKey k;
    k.device = device;
    k.n = n;
    k.digest = digest;
    k.medium = {3u, 0u, seed};
    k.table.assign(size_t(n) * 4, 7);
    if (n > 0) k.table[size_t(n)] ^= moved;
    return k;
}

bool make(Pool &p)
{
    p.mem.made++;
    g_made++;
    return true;
}
void on_epoch(Pool &p, bool zero)
{
    // (called under the registry's mutex: the pool's fields are stable)
    if (p.refs != 1) g_shared_epoch++;
    p.mem.resets++;
    if (zero) p.mem.zeroed++;
    if (p.refs > p.mem.refs_at_reset_max) p.mem.refs_at_reset_max = p.refs;
}
void leave(Registry &r, Pool *p)
{
    if (r.detach(p)) {
        g_freed++;
        delete p;
    }
}

void test_entry()
{
    using namespace rm;
    const uint32_t words[] = {0u, 1u, 2u, 3u, (kNcEpochMax << 1) | 1u, (kNcEpochMax << 1), (1u << kNcWordBits) - 1u};
    const uint32_t offs[] = {0u, 1u, (1u << kNcOffBits) - 1u, (1u << kNcOffBits) - 1024u, 12345678u};
    const uint32_t lens[] = {0u, 1u, 63u, 64u, 1023u, 1024u, (1u << kNcLenBits) - 1u};
    for (uint32_t w : words)
        for (uint32_t o : offs)
            for (uint32_t l : lens) {
                const uint64_t e = nc_entry_pack(w, o, l);
                CHECK(nc_entry_word(e) == w && nc_entry_off(e) == o && nc_entry_len(e) == l);
            }
    // a field never spills into its neighbour: bits beyond a field's width are dropped, not carried
    CHECK(nc_entry_pack(0u, 1u << kNcOffBits, 0u) == 0u);
    CHECK(nc_entry_pack(0u, 0u, 1u << kNcLenBits) == 0u);
    CHECK(nc_entry_pack(1u << kNcWordBits, 0u, 0u) == 0u);
    // the all-zero entry names epoch 0, which no pool ever runs in; "claimed" differs from "valid" in the lowest bit of the word alone
    CHECK(nc_entry_word(0u) == 0u);
    CHECK((nc_entry_word(nc_entry_pack(10u, 0u, 0u)) >> 1) == (nc_entry_word(nc_entry_pack(11u, 99u, 5u)) >> 1));
    CHECK(kNcArenaMax == (uint64_t(1) << 27));
    // the largest list at the arena's very end
    const uint64_t last = nc_entry_pack((kNcEpochMax << 1) | 1u, uint32_t(kNcArenaMax - 1024u), 1024u);
    CHECK(uint64_t(nc_entry_off(last)) + nc_entry_len(last) == kNcArenaMax);
}

void test_rules()
{
    Registry r;
    bool joined = true;
    Pool *a = r.attach(key_of(0, 100, 11, 5), make, on_epoch, &joined);
    CHECK(a && !joined && a->refs == 1 && a->epoch == 1 && a->mem.made == 1 && a->mem.resets == 1 && a->mem.zeroed == 1);
    Pool *b = r.attach(key_of(0, 100, 11, 5), make, on_epoch, &joined);
    CHECK(b == a && joined && a->refs == 2 && a->mem.resets == 1);
    // no sharing across a difference: device, size, digest, a parameter, a table byte under an equal digest
    for (rmh::NcPoolKey k : {key_of(1, 100, 11, 5), key_of(0, 101, 11, 5), key_of(0, 100, 12, 5), key_of(0, 100, 11, 6), key_of(0, 100, 11, 5, 1)}) {
        Pool *c = r.attach(std::move(k), make, on_epoch, &joined);
        CHECK(c && c != a && !joined && c->refs == 1);
        leave(r, c);
    }
    CHECK(r.live() == 1);
    // shared: a change that is none of the key's changes nothing; a change of the key makes the context leave; never an epoch
    rmh::NcPoolKey same = key_of(0, 100, 11, 5);
    CHECK(r.changed(a, same, on_epoch) == Registry::kStay && a->refs == 2 && a->epoch == 1);
    rmh::NcPoolKey other = key_of(0, 100, 13, 5, 2);
    CHECK(r.changed(a, other, on_epoch) == Registry::kLeft && a->refs == 1 && a->epoch == 1 && a->mem.resets == 1);
    CHECK(other.n == 100 && other.table.size() == 400); // (the key is still the caller's: it attaches with it)
    Pool *c = r.attach(std::move(other), make, on_epoch, &joined);
    CHECK(c && c != a && !joined && r.live() == 2);
    // alone: the pool is kept, takes the new key and begins an epoch -- an unchanged key too, as a private cache did
    rmh::NcPoolKey k2 = key_of(0, 100, 14, 5, 3);
    CHECK(r.changed(a, k2, on_epoch) == Registry::kNewEpoch && a->refs == 1 && a->epoch == 2 && a->mem.resets == 2 && a->mem.zeroed == 1);
    CHECK(a->key == key_of(0, 100, 14, 5, 3));
    rmh::NcPoolKey k3 = key_of(0, 100, 14, 5, 3);
    CHECK(r.changed(a, k3, on_epoch) == Registry::kNewEpoch && a->epoch == 3);
    // the epoch's number starts over before the entry's field would wrap, and the entries are zeroed then
    a->epoch = rm::kNcEpochMax - 1;
    rmh::NcPoolKey k4 = key_of(0, 100, 14, 5, 3);
    CHECK(r.changed(a, k4, on_epoch) == Registry::kNewEpoch && a->epoch == rm::kNcEpochMax && a->mem.zeroed == 1);
    rmh::NcPoolKey k5 = key_of(0, 100, 14, 5, 3);
    CHECK(r.changed(a, k5, on_epoch) == Registry::kNewEpoch && a->epoch == 1 && a->mem.zeroed == 2);
    CHECK(((a->epoch << 1) | 1u) < (1u << rm::kNcWordBits));
    // lifetime: the last context takes the pool out of the registry; the same key then makes a new one
    leave(r, c);
    leave(r, a);
    CHECK(r.live() == 0);
    Pool *d = r.attach(key_of(0, 100, 14, 5, 3), make, on_epoch, &joined);
    CHECK(d && !joined && d->epoch == 1 && d->mem.zeroed == 1);
    leave(r, d);
    CHECK(r.live() == 0 && g_made == g_freed);
    // a pool that cannot be made leaves nothing behind
    Pool *none = r.attach(key_of(0, 5, 1, 1), [](Pool &) { return false; }, on_epoch, &joined);
    CHECK(none == nullptr && r.live() == 0);
}

// several "contexts", one per thread, over a handful of tables: attach, look, change, leave, again and again
void test_threads()
{
    Registry r;
    const int kThreads = 8, kRounds = 4000;
    std::atomic<long> attached{0};
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; ++t)
        th.emplace_back([&, t] {
            uint32_t x = 12345u + 977u * uint32_t(t);
            auto rnd = [&] { return x = x * 1664525u + 1013904223u, x >> 8; };
            Pool *mine = nullptr;
            uint64_t table = 0;
            for (int i = 0; i < kRounds; ++i) {
                const uint32_t op = rnd() % 8u;
                if (!mine) {
                    table = rnd() % 3u;
                    bool joined = false;
                    mine = r.attach(key_of(0, 16, table, 1), make, on_epoch, &joined);
                    CHECK(mine != nullptr);
                    attached++;
                    int refs = 0;
                    uint32_t ep = 0;
                    r.look(mine, &refs, &ep, nullptr);
                    CHECK(refs >= 1 && ep >= 1 && ep <= rm::kNcEpochMax);
                } else if (op < 3u) { // the context's table changed
                    const uint64_t to = rnd() % 3u;
                    rmh::NcPoolKey k = key_of(0, 16, to, 1);
                    uint32_t before = 0, after = 0;
                    int refs_before = 0;
                    r.look(mine, &refs_before, &before, nullptr);
                    const auto what = r.changed(mine, k, on_epoch);
                    if (what == Registry::kLeft) {
                        CHECK(to != table);
                        bool joined = false;
                        mine = r.attach(std::move(k), make, on_epoch, &joined);
                        CHECK(mine != nullptr);
                    } else if (what == Registry::kStay) {
                        CHECK(to == table);
                    } else {
                        r.look(mine, nullptr, &after, nullptr);
                        (void)after;
                    }
                    table = to;
                } else if (op < 5u) {
                    leave(r, mine);
                    mine = nullptr;
                    attached--;
                } else { // a batch: the pool's epoch cannot move while anybody else is attached too
                    int refs = 0;
                    uint32_t e0 = 0;
                    r.look(mine, &refs, &e0, nullptr);
                    CHECK(refs >= 1);
                    CHECK(mine->key.digest == table); // (only its lone context rewrites a pool's key)
                }
            }
            if (mine) {
                leave(r, mine);
                attached--;
            }
        });
    for (auto &t : th) t.join();
    CHECK(attached == 0);
    CHECK(r.live() == 0);
    CHECK(g_made == g_freed);
    CHECK(g_shared_epoch == 0); // never a new epoch while shared
}

} // namespace

int main()
{
    test_entry();
    test_rules();
    test_threads();
    CHECK(g_shared_epoch == 0);
    std::printf("pools made %ld, freed %ld\nok\n", g_made.load(), g_freed.load());
    return 0;
}
