// record_index_check.cpp -- stand-alone check of csrc/record_index.h on the host (tests/test_record_index_cpu.py builds it with
// -fsanitize=address,undefined and runs it as a child process).  A seeded random sequence of insert, replace (pending and uploaded),
// erase (pending and uploaded), clear, plan-flush and plan-compaction over 50 keys and record lengths 0 to 40, for the payload
// shapes of the KeyFrameDatabase (4 + 8 bytes an element) and of the covisibility index (4 + 1), each step compared with a std::map
// model; a host byte array per column stands for the arena, and the planned uploads and move jobs are applied to it.  Prints one
// line per shape (operations of each kind), then "ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>
#include "../../motioncheck_ccm_slam_amd/csrc/record_index.h"

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd(uint32_t n) { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (uint32_t)((g_state >> 20) % n); }

#define CHECK(cond) do { if (!(cond)) { std::printf("step %d, line %d: %s\n", step, __LINE__, #cond); return false; } } while (0)

struct ModelRecord { int32_t slot; int64_t seq; bool uploaded; std::vector<uint8_t> col[2]; };

struct Harness {
    RecordIndex ix;
    std::map<int64_t, ModelRecord> model;
    std::vector<int64_t> pending_keys;              // the order in which plan_flush must place them
    std::vector<int32_t> free_model;                // the slot freed last is taken first
    int64_t next_seq = 0, cap = 64;
    std::vector<uint8_t> arena[2];
    int step = 0;

    Harness(size_t e0, size_t e1) : ix(e0, e1) { for (int k = 0; k < 2; k++) arena[k].assign((size_t)cap * ix.elem[k], 0xee); }

    RecordPending payload(int n, std::vector<uint8_t> col[2])
    {
        for (int k = 0; k < 2; k++) { col[k].resize((size_t)n * ix.elem[k]); for (uint8_t& b : col[k]) b = (uint8_t)rnd(256); }
        return ix.stage(n, n ? col[0].data() : nullptr, n ? col[1].data() : nullptr);
    }

    bool insert(int64_t key)
    {
        ModelRecord m{ free_model.empty() ? ix.slots() : free_model.back(), next_seq++, false, {} };
        if (!free_model.empty()) free_model.pop_back();
        ix.table_dirty = false;
        ix.insert(key, payload((int)rnd(41), m.col));
        CHECK(ix.table_dirty && ix.find(key) == m.slot);                   // a freed slot is the next one taken
        model[key] = m; pending_keys.push_back(key);
        return true;
    }

    bool replace(int64_t key)
    {
        ModelRecord& m = model[key];
        ix.table_dirty = false;
        ix.replace(ix.find(key), payload((int)rnd(41), m.col));
        CHECK(ix.table_dirty);
        if (m.uploaded) { m.uploaded = false; pending_keys.push_back(key); }       // a pending one is overwritten in place
        return true;
    }

    bool erase(int64_t key)
    {
        ix.table_dirty = false;
        ix.erase(key);
        auto it = model.find(key);
        if (it == model.end()) { CHECK(!ix.table_dirty); return true; }
        CHECK(ix.table_dirty);
        free_model.push_back(it->second.slot);
        pending_keys.erase(std::remove(pending_keys.begin(), pending_keys.end(), key), pending_keys.end());
        model.erase(it);
        return true;
    }

    void clear() { ix.clear(); model.clear(); pending_keys.clear(); free_model.clear(); }

    // Applies a planned compaction into a fresh arena of new_cap elements.
    bool compact(int64_t new_cap)
    {
        std::vector<RecordMoveJob> jobs;
        const int64_t used_before = ix.used;
        ix.table_dirty = false;
        ix.plan_compaction(jobs);
        CHECK(ix.table_dirty && ix.used == ix.live && ix.used <= new_cap);
        std::vector<uint8_t> fresh[2];
        for (int k = 0; k < 2; k++) fresh[k].assign((size_t)new_cap * ix.elem[k], 0xee);
        std::vector<uint8_t> written((size_t)new_cap, 0);
        for (const RecordMoveJob& j : jobs) {
            CHECK(j.len > 0 && j.src >= 0 && j.src + j.len <= used_before && j.dst >= 0 && j.dst + j.len <= ix.used);
            for (int64_t i = j.dst; i < j.dst + j.len; i++) { CHECK(!written[(size_t)i]); written[(size_t)i] = 1; }   // destinations never overlap
            for (int k = 0; k < 2; k++)
                std::memcpy(fresh[k].data() + (size_t)j.dst * ix.elem[k], arena[k].data() + (size_t)j.src * ix.elem[k], (size_t)j.len * ix.elem[k]);
        }
        for (int k = 0; k < 2; k++) arena[k].swap(fresh[k]);
        cap = new_cap;
        return true;
    }

    bool flush()
    {
        const int64_t add = ix.pending_elements();
        if (ix.used + add > cap && !compact(std::max(2 * cap, ix.live + add))) return false;
        std::vector<uint8_t> upload[2];
        const int64_t used_before = ix.used, live_before = ix.live;
        const bool had_pending = !ix.pending.empty();
        ix.table_dirty = false;
        const int64_t tail = ix.plan_flush(upload);
        CHECK(tail == used_before && ix.used == used_before + add && ix.live == live_before + add && ix.used <= cap);
        CHECK(ix.pending.empty() && ix.table_dirty == had_pending);
        int64_t at = tail;
        for (int64_t key : pending_keys) {                                 // tail offsets in the order of the pending list
            ModelRecord& m = model[key];
            const RecordEntry& e = ix.entry[(size_t)m.slot];
            CHECK(e.off == at);
            at += e.len; m.uploaded = true;
        }
        pending_keys.clear();
        for (int k = 0; k < 2; k++) {
            CHECK(upload[k].size() == (size_t)add * ix.elem[k]);
            if (add) std::memcpy(arena[k].data() + (size_t)tail * ix.elem[k], upload[k].data(), upload[k].size());
        }
        return true;
    }

    bool verify()
    {
        const int n_slots = ix.slots();
        CHECK(ix.size() == (int)model.size() && ix.next_seq == next_seq);
        CHECK(n_slots == (int)(model.size() + free_model.size()) && ix.free_slots == free_model);
        std::vector<int64_t> keys((size_t)n_slots + 1, -7), seq((size_t)n_slots + 1, -7);
        ix.keys(keys.data(), seq.data());
        CHECK(keys[(size_t)n_slots] == -7 && seq[(size_t)n_slots] == -7);
        std::vector<RecordSlot> table;
        ix.table(table);
        CHECK((int)table.size() == n_slots);
        int held = 0;
        for (int s = 0; s < n_slots; s++) {
            if (seq[(size_t)s] < 0) { CHECK(keys[(size_t)s] == -1 && table[(size_t)s].len == -1); continue; }
            held++;
            CHECK(model.count(keys[(size_t)s]) && model[keys[(size_t)s]].slot == s);
        }
        CHECK(held == (int)model.size());
        int64_t live = 0;
        size_t n_pending = 0;
        std::vector<std::pair<int64_t, int64_t>> spans;
        for (const auto& kv : model) {
            const ModelRecord& m = kv.second;
            const RecordEntry& e = ix.entry[(size_t)m.slot];
            const int32_t len = (int32_t)(m.col[0].size() / ix.elem[0]);
            CHECK(ix.find(kv.first) == m.slot && e.key == kv.first && e.seq == m.seq && seq[(size_t)m.slot] == m.seq && e.len == len);
            CHECK(table[(size_t)m.slot].off == e.off && table[(size_t)m.slot].len == len);
            if (!m.uploaded) { CHECK(e.off == -1); n_pending++; continue; }
            CHECK(e.off >= 0 && e.off + len <= ix.used);
            live += len;
            if (len) spans.push_back({ e.off, e.off + len });
            for (int k = 0; k < 2; k++)                                    // the payload survived every flush and compaction
                CHECK(len == 0 || std::memcmp(arena[k].data() + (size_t)e.off * ix.elem[k], m.col[k].data(), m.col[k].size()) == 0);
        }
        CHECK(ix.live == live && ix.used >= ix.live && ix.used <= cap);
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); i++) CHECK(spans[i - 1].second <= spans[i].first);           // live records are disjoint
        CHECK(ix.pending.size() == n_pending && pending_keys.size() == n_pending);
        for (size_t i = 0; i < n_pending; i++) {
            const ModelRecord& m = model[pending_keys[i]];
            CHECK(ix.pending[i].slot == m.slot && ix.pending[i].col[0] == m.col[0] && ix.pending[i].col[1] == m.col[1]);
        }
        CHECK(ix.find(1000) == -1);
        return true;
    }
};

static bool run(const char* name, size_t e0, size_t e1, int n_steps)
{
    Harness h(e0, e1);
    int count[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };      // insert, replace pending / uploaded, erase pending / uploaded / absent, clear, compaction
    int flushes = 0;
    for (h.step = 0; h.step < n_steps; h.step++) {
        const uint32_t op = rnd(100);
        const int64_t key = (int64_t)rnd(50) * 1000003 - 17;
        const auto it = h.model.find(key);
        const bool present = it != h.model.end(), uploaded = present && it->second.uploaded;
        bool ok = true;
        if (op < 50) {
            if (!present) { ok = h.insert(key); count[0]++; }
            else { ok = h.replace(key); count[uploaded ? 2 : 1]++; }
        } else if (op < 72) { ok = h.erase(key); count[!present ? 5 : uploaded ? 4 : 3]++; }
        else if (op < 90) { ok = h.flush(); flushes++; }
        else if (op < 99) { ok = h.compact(h.cap); count[7]++; }
        else { h.clear(); count[6]++; }
        if (!ok || !h.verify()) { std::printf("%s failed\n", name); return false; }
    }
    std::printf("%s insert %d replace %d+%d erase %d+%d+%d clear %d flush %d compaction %d cap %lld\n", name, count[0], count[1], count[2],
                count[3], count[4], count[5], count[6], flushes, count[7], (long long)h.cap);
    for (int i = 0; i < 8; i++) if (count[i] < 10) { std::printf("%s: operation %d ran %d times\n", name, i, count[i]); return false; }
    return flushes >= 10;
}

int main()
{
    if (!run("kfdb", 4, 8, 4000) || !run("covis", 4, 1, 4000)) return 1;
    std::printf("ok\n");
    return 0;
}
