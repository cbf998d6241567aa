// record_index.h -- host bookkeeping of a keyed record store: one variable-length record per int64 key, a stable slot number and a
// sequence number per record, records that wait in a pending list until the owner's next flush, and an arena (owned by
// record_store.h) in which erased and replaced records leave holes until it is compacted.  A record is two parallel columns, kept
// here as bytes; lengths and offsets count elements.  Plain C++, nothing from HIP (tests/support/record_index_check.cpp runs it
// under sanitizers).  Not synchronised: the owner calls it under its mutex, except `stage`.
#pragma once
#include "record_types.h"
#include <cstddef>
#include <unordered_map>
#include <utility>
#include <vector>

struct RecordEntry {                        // one slot, host side
    int64_t key = 0, seq = -1;              // seq < 0: free slot
    int64_t off = -1;                       // place in the arena; -1 while the record waits in `pending`
    int32_t len = 0;
};

struct RecordPending { int32_t slot; std::vector<uint8_t> col[2]; };

struct RecordIndex {
    const size_t elem[2];                   // bytes per element of the two columns
    std::unordered_map<int64_t, int32_t> slot_of;
    std::vector<RecordEntry> entry;         // [slots]: its size is the high-water mark
    std::vector<int32_t> free_slots;        // the slot freed last is taken first
    std::vector<RecordPending> pending;     // inserted or replaced since the last flush, in that order
    int64_t next_seq = 0;
    bool table_dirty = false;               // the device's slot table is behind `entry`
    int64_t used = 0, live = 0;             // arena elements: tail, held by uploaded live records

    RecordIndex(size_t elem0, size_t elem1) : elem{ elem0, elem1 } {}

    // A record of n elements copied from the caller's columns: reads `elem` only, so the owner calls it outside its lock.
    RecordPending stage(int n, const void* col0, const void* col1) const
    {
        const uint8_t* src[2] = { static_cast<const uint8_t*>(col0), static_cast<const uint8_t*>(col1) };
        RecordPending p{ -1, {} };
        for (int k = 0; k < 2; k++)
            if (n > 0) p.col[k].assign(src[k], src[k] + (size_t)n * elem[k]);
        return p;
    }

    int32_t find(int64_t key) const { auto it = slot_of.find(key); return it == slot_of.end() ? -1 : it->second; }
    int size() const { return (int)slot_of.size(); }
    int slots() const { return (int)entry.size(); }
    void keys(int64_t* key, int64_t* seq) const                            // [slots] each; key -1 for a free slot; seq may be null
    {
        for (size_t s = 0; s < entry.size(); s++) { key[s] = entry[s].seq < 0 ? -1 : entry[s].key; if (seq) seq[s] = entry[s].seq; }
    }

    void insert(int64_t key, RecordPending&& p)                            // the key is not present
    {
        pending.reserve(pending.size() + 1);
        if (free_slots.empty()) { free_slots.reserve(1); entry.emplace_back(); free_slots.push_back((int32_t)entry.size() - 1); }
        slot_of.emplace(key, free_slots.back());                           // nothing below throws
        p.slot = free_slots.back(); free_slots.pop_back();
        RecordEntry& e = entry[p.slot];
        e.key = key; e.seq = next_seq++; e.off = -1; e.len = length(p);
        pending.push_back(std::move(p));
        table_dirty = true;
    }

    void replace(int32_t slot, RecordPending&& p)                          // slot = find(key) >= 0: slot and sequence number stay
    {
        pending.reserve(pending.size() + 1);                               // nothing below throws
        p.slot = slot;
        RecordEntry& e = entry[slot];
        const bool uploaded = e.off >= 0;
        if (uploaded) { live -= e.len; e.off = -1; }                       // its elements become a hole in the arena
        e.len = length(p);
        if (uploaded) pending.push_back(std::move(p));
        else for (RecordPending& q : pending) if (q.slot == slot) { q = std::move(p); break; }      // overwritten where it waits
        table_dirty = true;
    }

    void erase(int64_t key)                                                // an absent key: nothing to erase
    {
        auto it = slot_of.find(key);
        if (it == slot_of.end()) return;
        const int32_t s = it->second;
        free_slots.reserve(free_slots.size() + 1);                         // nothing below throws
        slot_of.erase(it);
        RecordEntry& e = entry[s];
        if (e.off < 0) {                                                   // never uploaded: drop it from the pending list
            for (size_t i = 0; i < pending.size(); i++)
                if (pending[i].slot == s) { pending.erase(pending.begin() + (long)i); break; }
        } else live -= e.len;                                              // its elements become a hole in the arena
        e = RecordEntry();
        free_slots.push_back(s);
        table_dirty = true;
    }

    void clear()
    {
        slot_of.clear(); entry.clear(); free_slots.clear(); pending.clear();
        used = live = 0;
        table_dirty = true;
    }

    int64_t pending_elements() const
    {
        int64_t n = 0;
        for (const RecordPending& p : pending) n += entry[p.slot].len;
        return n;
    }

    // Packs the uploaded live records at the front of a new arena: their new offsets, and the copies from the old arena in `jobs`.
    void plan_compaction(std::vector<RecordMoveJob>& jobs)
    {
        jobs.clear(); jobs.reserve(entry.size());                          // nothing below throws
        int64_t tail = 0;
        for (RecordEntry& e : entry) {
            if (e.seq < 0 || e.off < 0) continue;
            if (e.len > 0) jobs.push_back(RecordMoveJob{ e.off, tail, e.len, 0 });
            e.off = tail; tail += e.len;
        }
        used = live = tail; table_dirty = true;
    }

    // Places the pending records at the arena's tail in their order and empties the list.  upload[k]: their columns back to back,
    // for the arena from the returned element (the tail before the call) on.
    int64_t plan_flush(std::vector<uint8_t> upload[2])
    {
        const int64_t tail = used, add = pending_elements();
        if (pending.empty()) return tail;
        for (int k = 0; k < 2; k++) { upload[k].clear(); upload[k].reserve((size_t)add * elem[k]); }       // nothing below throws
        int64_t at = tail;
        for (const RecordPending& p : pending) {
            RecordEntry& e = entry[p.slot];
            e.off = at; at += e.len;
            for (int k = 0; k < 2; k++) upload[k].insert(upload[k].end(), p.col[k].begin(), p.col[k].end());
        }
        pending.clear();
        used += add; live += add; table_dirty = true;
        return tail;
    }

    void table(std::vector<RecordSlot>& t) const                           // the slot table as the device reads it
    {
        t.resize(entry.size());
        for (size_t s = 0; s < entry.size(); s++)
            t[s] = entry[s].seq < 0 ? RecordSlot{ 0, -1, 0 } : RecordSlot{ entry[s].off, entry[s].len, 0 };
    }

private:
    int32_t length(const RecordPending& p) const { return (int32_t)(p.col[0].size() / elem[0]); }
};
