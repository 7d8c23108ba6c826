/*
 * mapAdapter.h — the ONE place where the planner facades go beyond the four map methods the reference calls
 * (getRes, isInflatedOccupied, isInflatedOccupiedLine, isUnknown).
 *
 * The device works on a dense snapshot of the voxel map (include/vigo.h, "voxel map").  An arbitrary
 * mapManager::occMap offers no bulk access, so the adapter RASTERISES it: every voxel centre of a caller-given box
 * is asked isInflatedOccupied / isUnknown and the answers become the byte grid vigo_set_grid_host() uploads
 * (bit0 inflated-occupied, bit1 unknown, bit2 := bit0 — the un-inflated occupancy is not observable through the four
 * methods; only polyTrajOctomap's octree-style checks read bit2).  The box comes from setMapRegion() of the planner
 * classes; a live map is re-rasterised when the owner calls refreshMap() (the reference's planners see map updates
 * through the shared pointer, a device snapshot cannot).
 *
 * Builds without map_manager (this tree's dense stand-in, standin/dense_occmap.h) take a fast path: the stand-in's
 * own bytes are uploaded as they are and its `version` counter tells when they changed — no region, no refresh call.
 *
 * When the map's owner says WHICH box changed (the dense map's markChanged(lo, n); refreshMap(boxMin, boxMax) /
 * updateMap(boxMin, boxMax) on a live map), a handle whose snapshot is only such changes behind gets the boxes alone,
 * through vigo_update_grid_region_host: the dense map's bytes of the box as they are, a live map rasterised over the box
 * only.  Anything else — a first upload, a bare ++version, refreshMap() without a box, more than 16 changes behind, boxes
 * that together hold no fewer voxels than the grid — replaces the snapshot whole as before.
 */
#ifndef TRAJECTORY_PLANNER_MAP_ADAPTER_H
#define TRAJECTORY_PLANNER_MAP_ADAPTER_H
#include <trajectory_planner/compat.h>
#include <trajectory_planner/dirtyJournal.h>

#include <cstdint>
#include <memory>
#include <vector>

struct vigo_context;
struct vigo_params_s;

namespace trajPlanner {

struct mapRegion {
    bool set = false;
    Eigen::Vector3d boxMin, boxMax;   // metric box the planner works in
};
// two planners may share one device snapshot only when they would rasterise the same box
inline bool sameRegion(const mapRegion& a, const mapRegion& b) {
    if (a.set != b.set) return false;
    if (!a.set) return true;
    for (int k = 0; k < 3; ++k)
        if (a.boxMin(k) != b.boxMin(k) || a.boxMax(k) != b.boxMax(k)) return false;
    return true;
}

class mapAdapter {
public:
    /* Make `dev` hold a current snapshot of `map`.  `stamp` is the caller's memo of what it last uploaded (0 = nothing
     * yet / refresh requested); it is updated.  false: no region for a map that needs one, or a device failure. */
    static bool uploadSnapshot(vigo_context* dev, const std::shared_ptr<mapManager::occMap>& map, const mapRegion& region,
                               uint64_t& stamp);
    /* A live map (one the adapter can only rasterise) changed: EVERY handle that snapshotted it is stale, whichever
     * planner's refreshMap() / updateMap() said so — the generation is per map object, process-wide, and a planner's
     * `stamp` records the generation its own handle holds (so a batch whose lead never asked for the refresh itself
     * still re-rasterises).  Generations start at 1; a stamp of 0 never matches. */
    static uint64_t generation(const mapManager::occMap* map);
    static void bumpGeneration(const mapManager::occMap* map);
    /* ... and the same with the metric box outside which the map did not change: the generation moves AND the map's
     * journal (one per map object, next to its generation) gets the box, in voxels of the lattice of whole multiples of
     * res from zero that every region's snapshot lies on: lo = floor(boxMin / res), n = ceil(boxMax / res) - lo.  A box
     * that is not finite or is empty counts as a bump without a box. */
    static void bumpGeneration(mapManager::occMap* map, const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);
    /* the boxes of every generation in (since, now] of a live map: DirtyJournal::changesSince on the map's journal */
    static bool changesSince(const mapManager::occMap* map, uint64_t since, uint64_t now, std::vector<DirtyBox>& out);
    /* process-wide counts of what uploadSnapshot sent, behind the generation table's lock: snapshots replaced whole,
     * boxes sent by the region route, and the voxels in those boxes */
    struct SnapshotTotals {
        long long fullSnapshots = 0, regionUpdates = 0, regionVoxels = 0;
    };
    static SnapshotTotals snapshotTotals();
    /* octomap-style node lookup for polyTrajOctomap::checkCollisionPoint (PO.cpp:571-589): kOutside beyond the metric
     * bounds, else bit1 = no node (unknown), bit2 = occupied */
    enum : unsigned { kUnknown = 2u, kOccupied = 4u, kOutside = 0x80u };
    static unsigned nodeBits(const std::shared_ptr<mapManager::occMap>& map, const mapRegion& region, float x, float y, float z);
    /* rasterisation of any occMap through its four public methods over `region` (what uploadSnapshot uploads for a
     * map it cannot read in bulk); dims and origin of the grid are returned */
    static bool rasterise(mapManager::occMap& map, const mapRegion& region, std::vector<uint8_t>& voxels, int dims[3], double origin[3]);
    /* the same over the sub-box [subMin, subMax] only, on the lattice rasterise() uses for `region` (origin
     * floor(boxMin / res) * res): the voxels the sub-box touches, clipped to the region's grid, come back as
     * bytes[n[0]][n[1]][n[2]] with their first voxel lo — the arguments of vigo_update_grid_region_host.  An empty clip is
     * a no-op: true with n = {0, 0, 0}.  false: no region, or a resolution or box rasterise() refuses. */
    static bool rasteriseBox(mapManager::occMap& map, const mapRegion& region, const Eigen::Vector3d& subMin, const Eigen::Vector3d& subMax,
                             std::vector<uint8_t>& bytes, int lo[3], int n[3]);
    /* ... and over a box given in voxels of the zero-based lattice (a journal entry of a live map) */
    static bool rasteriseKeys(mapManager::occMap& map, const mapRegion& region, const int keyLo[3], const int keyN[3],
                              std::vector<uint8_t>& bytes, int lo[3], int n[3]);
};

/* The link between ONE planner and its device handle, held by all three facades (bsplineTraj, polyTrajOctomap,
 * polyTrajOccMap): the map and the box of it to snapshot, the memo of the snapshot the handle holds, the HIP device
 * ordinal, and the handle itself, which it creates on demand and destroys.  It prints nothing: sync() says why it failed
 * and each facade keeps its own console lines. */
class DeviceLink {
public:
    enum Sync { kSynced = 0, kNoMap, kNoDevice, kNoHandle, kFailed };
    DeviceLink() = default;
    ~DeviceLink();
    DeviceLink(const DeviceLink&) = delete;
    DeviceLink& operator=(const DeviceLink&) = delete;

    void setMap(const std::shared_ptr<mapManager::occMap>& map);                    // forces a new snapshot
    void setRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);   // forces a new snapshot
    /* the map changed: every handle that holds a snapshot of it is stale, not only this one (generation, above) */
    void refresh();
    /* ... and only inside this metric box: handles that were current before get the box alone (mapAdapter.h, top).  On the
     * in-tree dense map this is markChanged() of the voxels the box touches. */
    void refresh(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax);
    /* One process per GPU is the deployment the back-end is built for (HIP_VISIBLE_DEVICES picks the card); a process
     * that drives several cards gives each planner its ordinal before the planner's first device call.  The current
     * ordinal: nothing happens.  Another: the link lets go of its handle; the next sync() creates one there and uploads
     * the map again. */
    void setDevice(int ordinal);
    /* In this order: the ordinal's GPU made current on the calling thread (its stream and staging buffers are per
     * thread and device), the handle created on demand, its launches and copies bound to the calling thread's stream
     * (two host threads planning two batches then overlap on the device), `params` pushed when given, the map
     * snapshotted again if it changed.  Without a map: kNoMap before anything else when `needMap`, else no snapshot. */
    Sync sync(bool needMap, const vigo_params_s* params = nullptr);

    vigo_context* handle() const { return dev_; }
    const std::shared_ptr<mapManager::occMap>& map() const { return map_; }
    const mapRegion& region() const { return region_; }
    int ordinal() const { return ordinal_; }
    /* two planners may share one handle's state: same device, same map object, same box of it */
    bool sameTarget(const DeviceLink& o) const { return ordinal_ == o.ordinal_ && map_ == o.map_ && sameRegion(region_, o.region_); }

private:
    std::shared_ptr<mapManager::occMap> map_;
    mapRegion region_;
    uint64_t stamp_ = 0;   // uploadSnapshot's memo of the snapshot the handle holds (0 = none)
    int ordinal_ = 0;
    vigo_context* dev_ = nullptr;
};

}  // namespace trajPlanner
#endif
