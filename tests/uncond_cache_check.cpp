// Stand-alone check of csrc/uncond_cache.h (the bookkeeping of the unconditional code-path cache): built and run by
// tests/test_host_uncond_cache.py with -fsanitize=address,undefined.  Slots are "busy" while they sit in a set.
#include "../detail_tts_amd/csrc/uncond_cache.h"

#include <cstdio>
#include <cstdlib>
#include <set>

using namespace dtts;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static UncondKey key(int len, int T = 400) {
    UncondKey k;
    k.bind_gen = 1;
    k.sched_id = 2;
    k.kind = 0;
    k.tmap = {0, 10, 20};
    k.n_pos = 3;
    k.len = len;
    k.T = T;
    return k;
}

int main() {
    std::set<int> busy_slots;
    const auto busy = [&](int s) { return busy_slots.count(s) != 0; };
    const size_t A = UncondCacheBook::ALIGN;

    // budget 0: nothing is ever stored, nothing is ever found
    {
        UncondCacheBook b;
        CHECK(b.insert(key(100), 1000, busy) == nullptr);
        CHECK(b.lookup(key(100)) == nullptr);
        b.set_budget(0);
        CHECK(b.insert(key(100), 1, busy) == nullptr);
        CHECK(b.stats().entries == 0 && b.stats().misses == 1 && b.stats().hits == 0);
    }
    // budget, offsets, LRU order
    {
        UncondCacheBook b;
        b.set_budget(3 * 1024);
        const UncondCacheBook::Entry* e0 = b.insert(key(1), 1000, busy);
        CHECK(e0 && e0->off == 0 && e0->bytes == 1000);
        const int s0 = e0->slot;
        const UncondCacheBook::Entry* e1 = b.insert(key(2), 1024, busy);
        CHECK(e1 && e1->off == 1024 && e1->slot != s0);
        const UncondCacheBook::Entry* e2 = b.insert(key(3), 1024, busy);
        CHECK(e2 && e2->off == 2048);
        CHECK(b.insert(key(2), 1024, busy) == nullptr);                 // stored already
        CHECK(b.stats().entries == 3 && b.stats().bytes == 1000 + 2048 && b.stats().evictions == 0);
        for (const auto& e : b.entries()) CHECK(e.off % A == 0 && e.off + e.bytes <= b.budget());
        CHECK(b.lookup(key(1)));                                        // key 1 is now the most recently used: key 2 is the oldest
        const UncondCacheBook::Entry* e3 = b.insert(key(4), 1024, busy);
        CHECK(e3 && e3->off == 1024 && b.stats().evictions == 1);
        CHECK(b.lookup(key(2)) == nullptr && b.lookup(key(1)) && b.lookup(key(3)) && b.lookup(key(4)));
        // an entry of two units: the two oldest neighbours go (1 was touched before 3 and 4 just now) - or more, until a gap opens
        const UncondCacheBook::Entry* e4 = b.insert(key(5), 2048, busy);
        CHECK(e4 && e4->bytes == 2048 && e4->off + 2048 <= b.budget());
        CHECK(b.lookup(key(5)) && b.lookup(key(1)) == nullptr);
        for (size_t i = 1; i < b.entries().size(); ++i) CHECK(b.entries()[i - 1].off + b.entries()[i - 1].bytes <= b.entries()[i].off);
        // oversize: not stored, nothing given up for it
        const unsigned long long ev = b.stats().evictions, n = b.stats().entries;
        CHECK(b.insert(key(6), 3 * 1024 + 1, busy) == nullptr);
        CHECK(b.stats().evictions == ev && b.stats().entries == n);
    }
    // every key field separates entries
    {
        UncondCacheBook b;
        b.set_budget(1 << 20);
        const UncondKey k0 = key(50);
        CHECK(b.insert(k0, 512, busy));
        UncondKey k = k0;
        CHECK(b.lookup(k));
        k = k0; k.bind_gen = 2; CHECK(!b.lookup(k));
        k = k0; k.sched_id = 3; CHECK(!b.lookup(k));
        k = k0; k.kind = 1; CHECK(!b.lookup(k));
        k = k0; k.tmap = {0, 10, 21}; CHECK(!b.lookup(k));
        k = k0; k.tmap = {0, 10}; CHECK(!b.lookup(k));
        k = k0; k.ftimes = {0.5f}; CHECK(!b.lookup(k));
        k = k0; k.n_pos = 2; CHECK(!b.lookup(k));
        k = k0; k.len = 51; CHECK(!b.lookup(k));
        k = k0; k.T = 401; CHECK(!b.lookup(k));
        CHECK(b.stats().hits == 1 && b.stats().misses == 9);
        CHECK(!(k0 == k));
    }
    // a busy slot is never reused and never waited for
    {
        UncondCacheBook b;
        b.set_budget(2 * 1024);
        const int s1 = b.insert(key(1), 1024, busy)->slot;
        const int s2 = b.insert(key(2), 1024, busy)->slot;
        busy_slots = {s1};                                              // the oldest entry is busy: the next oldest goes instead
        const UncondCacheBook::Entry* e = b.insert(key(3), 1024, busy);
        CHECK(e && e->off == 1024 && e->slot == s2);                    // (its slot number is handed on)
        CHECK(b.lookup(key(1)) && !b.lookup(key(2)));
        busy_slots = {s1, s2};                                          // both busy: not stored, both kept
        CHECK(b.insert(key(4), 1024, busy) == nullptr);
        CHECK(b.lookup(key(1)) && b.lookup(key(3)) && b.stats().entries == 2);
        busy_slots = {s2};                                              // two units need both slots; one is busy: the idle one is given up in vain, nothing stored
        CHECK(b.insert(key(5), 2048, busy) == nullptr);
        CHECK(b.lookup(key(3)) && b.stats().entries == 1);
        busy_slots.clear();
        CHECK(b.insert(key(5), 2048, busy));
    }
    // a rebind: nothing of the old generation is served; its bytes go first, but only once idle
    {
        UncondCacheBook b;
        b.set_budget(2 * 1024);
        const int s1 = b.insert(key(1), 1024, busy)->slot;
        CHECK(b.insert(key(2), 1024, busy));
        CHECK(b.lookup(key(2)));
        b.invalidate_all();
        CHECK(!b.lookup(key(1)) && !b.lookup(key(2)) && b.stats().entries == 0 && b.stats().bytes == 0);
        UncondKey k = key(1);
        k.bind_gen = 2;
        busy_slots = {s1};
        const UncondCacheBook::Entry* e = b.insert(k, 1024, busy);
        CHECK(e && e->off == 1024 && b.lookup(k));
        UncondKey k2 = key(2);
        k2.bind_gen = 2;
        CHECK(b.insert(k2, 1024, busy));                                // the dead entry is still read on the device: the live one makes room
        CHECK(b.lookup(k2) && !b.lookup(k) && b.entries().size() == 2);
        busy_slots.clear();
        CHECK(b.insert(k, 1024, busy) && b.lookup(k2) && b.lookup(k) && b.stats().entries == 2 && b.entries().size() == 2);
        b.count_bypass();
        CHECK(b.stats().bypasses == 1);
        b.set_budget(0);                                                // off: everything dropped, counters kept
        CHECK(b.stats().entries == 0 && !b.lookup(k) && b.stats().bypasses == 1);
    }
    std::puts("uncond_cache_check ok");
    return 0;
}
