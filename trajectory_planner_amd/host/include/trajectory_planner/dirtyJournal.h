/*
 * dirtyJournal.h — which boxes of a voxel map changed with which version of it: a ring of the last 16 entries, kept by the
 * map's owner side (the in-tree dense map's markChanged(), the adapter's generation table for a live map) and read by
 * mapAdapter::uploadSnapshot, which then sends only those boxes to the device (vigo_update_grid_region_host).
 *
 * A version the owner bumped WITHOUT an entry (a bare ++version, refreshMap() without a box) is a hole: changesSince()
 * is false across it and the snapshot is replaced whole, as before.  No dependencies; the rule for threads is the one of
 * the version counter itself: the owner changes the map between planning calls.
 */
#ifndef TRAJECTORY_PLANNER_DIRTY_JOURNAL_H
#define TRAJECTORY_PLANNER_DIRTY_JOURNAL_H
#include <cstdint>
#include <vector>

namespace trajPlanner {

struct DirtyBox {
    uint64_t version;   // the map's version AFTER this change
    int lo[3], n[3];    // first voxel and extent, on the lattice the journal's owner documents
};

class DirtyJournal {
public:
    static const int kEntries = 16;
    void record(uint64_t versionAfter, const int lo[3], const int n[3]) {
        DirtyBox& e = ring_[next_ % kEntries];
        e.version = versionAfter;
        for (int a = 0; a < 3; ++a) { e.lo[a] = lo[a]; e.n[a] = n[a]; }
        ++next_;
    }
    /* true: `out` holds, oldest first, one entry for EVERY version in (since, now].  false — and the caller takes the full
     * route — when since == 0 (nothing uploaded yet), since > now, a version of the range has no entry (a bare bump), or
     * the range is longer than the ring. */
    bool changesSince(uint64_t since, uint64_t now, std::vector<DirtyBox>& out) const {
        out.clear();
        if (since == 0 || since > now || now - since > (uint64_t)kEntries) return false;
        const uint64_t held = next_ < (uint64_t)kEntries ? next_ : (uint64_t)kEntries;
        for (uint64_t v = since + 1; v <= now; ++v) {
            bool found = false;
            for (uint64_t k = 0; k < held && !found; ++k) {
                const DirtyBox& e = ring_[(next_ - 1 - k) % kEntries];   // newest first: a version recorded twice reads its last entry
                if (e.version == v) { out.push_back(e); found = true; }
            }
            if (!found) { out.clear(); return false; }
        }
        return true;
    }

private:
    DirtyBox ring_[kEntries] = {};
    uint64_t next_ = 0;   // entries ever recorded
};

}  // namespace trajPlanner
#endif
