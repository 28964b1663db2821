// Bookkeeping of the unconditional code-path cache (model_diffusion.hip): which (binding, schedule, length) slab lives
// where in ONE device block of `budget` bytes, in which order slabs are given up, and how often the cache served, missed, stood aside
// or evicted.  No HIP in here: the book deals in sizes, offsets and slot numbers; whether a slot's device work is still pending is the
// caller's to answer (a callback), so the whole of it compiles and runs on the CPU (tests/uncond_cache_check.cpp).
// Not thread safe: the owner holds its mutex around every call.
#pragma once
#include <cstddef>
#include <functional>
#include <vector>

namespace dtts {

// Everything that changes the bits of a slab.  (Option "trunk_fp16" is NOT in here: the integrator always takes three products,
// DESIGN.md 4.1b.  The launches' widths are not either: a slab is stored and served only where no launch of the pre-pass picks its
// summation order by its width, Model::integ_unsplit.)
struct UncondKey {
    unsigned long long bind_gen = 0;      // every (re)bind of the weights starts a new generation
    int sched_id = 0, kind = 0;           // the schedule's identity on the handle ...
    std::vector<int> tmap;                // ... and its timestep list (kind 0), so that an id handed out twice never aliases
    std::vector<float> ftimes;            // (kinds 1, 2)
    int n_pos = 0;                        // loop positions 0 .. n_pos - 1 of the descending loop are stored
    int len = 0, T = 0;                   // the row's length and the padded width it was evaluated under (GroupNorm sums in T's order)
    bool operator==(const UncondKey& o) const {
        return bind_gen == o.bind_gen && sched_id == o.sched_id && kind == o.kind && n_pos == o.n_pos && len == o.len && T == o.T &&
               tmap == o.tmap && ftimes == o.ftimes;
    }
};

struct UncondCacheStats {
    unsigned long long entries = 0, bytes = 0, hits = 0, misses = 0, bypasses = 0, evictions = 0;
};

class UncondCacheBook {
public:
    struct Entry {
        UncondKey key;
        size_t off = 0, bytes = 0;
        int slot = -1;                    // the caller's handle for this entry's device-side state (events); reused after an eviction
        unsigned long long tick = 0;      // last use; 0 = invalidated (never served again, first to go)
    };
    static constexpr size_t ALIGN = 256;

    size_t budget() const { return budget_; }
    // a new budget drops every entry at once: the caller has made sure nothing on the device still uses the old block
    void set_budget(size_t bytes) {
        budget_ = bytes;
        entries_.clear();
        free_slots_.clear();
        next_slot_ = 0;
    }
    // the entry of `key`, most recently used from now on, or null; counts a hit or a miss
    const Entry* lookup(const UncondKey& key) {
        for (Entry& e : entries_)
            if (e.tick && e.key == key) {
                e.tick = ++clock_;
                ++hits_;
                return &e;
            }
        ++misses_;
        return nullptr;
    }
    // Room for a new entry of `bytes` under `key`: a gap of the block, made if need be by giving up the least recently used entries
    // whose slot is not busy(slot) - a busy slot is never overwritten and never waited for.  Null (nothing changed but evictions
    // already made): the key is stored already, the entry is larger than the budget, or no such gap could be made.
    const Entry* insert(const UncondKey& key, size_t bytes, const std::function<bool(int)>& busy) {
        const size_t need = (bytes + ALIGN - 1) / ALIGN * ALIGN;
        if (bytes == 0 || need > budget_) return nullptr;
        for (const Entry& e : entries_)
            if (e.tick && e.key == key) return nullptr;
        std::vector<int> skipped;                      // busy slots met in this call: asked once each
        for (;;) {
            size_t off = 0;
            if (find_gap(need, &off)) {
                Entry e;
                e.key = key;
                e.off = off;
                e.bytes = bytes;
                e.tick = ++clock_;
                if (free_slots_.empty()) e.slot = next_slot_++;
                else { e.slot = free_slots_.back(); free_slots_.pop_back(); }
                size_t at = 0;
                while (at < entries_.size() && entries_[at].off < off) ++at;
                entries_.insert(entries_.begin() + (long)at, e);
                return &entries_[at];
            }
            int victim = -1;
            for (size_t i = 0; i < entries_.size(); ++i) {
                bool skip = false;
                for (int s : skipped) skip |= s == entries_[i].slot;
                if (!skip && (victim < 0 || entries_[i].tick < entries_[(size_t)victim].tick)) victim = (int)i;
            }
            if (victim < 0) return nullptr;
            if (busy && busy(entries_[(size_t)victim].slot)) {
                skipped.push_back(entries_[(size_t)victim].slot);
                continue;
            }
            free_slots_.push_back(entries_[(size_t)victim].slot);
            entries_.erase(entries_.begin() + victim);
            ++evictions_;
        }
    }
    // every entry stops being served (a rebind); its bytes are given up like any other's once its slot is idle
    void invalidate_all() {
        for (Entry& e : entries_) e.tick = 0;
    }
    void count_bypass() { ++bypasses_; }
    const std::vector<Entry>& entries() const { return entries_; }
    UncondCacheStats stats() const {
        UncondCacheStats s;
        for (const Entry& e : entries_)
            if (e.tick) { ++s.entries; s.bytes += e.bytes; }
        s.hits = hits_;
        s.misses = misses_;
        s.bypasses = bypasses_;
        s.evictions = evictions_;
        return s;
    }

private:
    bool find_gap(size_t need, size_t* off) const {     // first fit; entries_ is ordered by offset
        size_t at = 0;
        for (const Entry& e : entries_) {
            if (e.off >= at + need) break;
            at = (e.off + e.bytes + ALIGN - 1) / ALIGN * ALIGN;
        }
        if (at + need > budget_) return false;
        *off = at;
        return true;
    }
    size_t budget_ = 0;
    std::vector<Entry> entries_;
    std::vector<int> free_slots_;
    int next_slot_ = 0;
    unsigned long long clock_ = 0, hits_ = 0, misses_ = 0, bypasses_ = 0, evictions_ = 0;
};

}  // namespace dtts
