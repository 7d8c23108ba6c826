// mapAdapter.cpp — see mapAdapter.h.  The generic path uses getRes / isInflatedOccupied / isUnknown only; the dense
// fast path exists only in builds with this tree's stand-in map (no VIGO_WITH_ROS).
#include <trajectory_planner/mapAdapter.h>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <iostream>
#include <map>
#include <mutex>
#include <vector>

#include "../../../include/vigo.h"
#include "devbuf.h"

// The one device entry point this file names beyond those of the whole route.  Weak: a program that links the planner
// sources against scripted stand-ins of the device entry points (tests/poly_batch_check.cpp lists them) has none, and
// there every change takes the whole route; libtrajectory_planner_vigo.so links libvigo_hip.so, which defines it.
#pragma weak vigo_update_grid_region_host

namespace trajPlanner {

namespace {
// the grid rasterise() makes of a region: aligned to multiples of res (the corridor checker's octomap keys need that);
// key0: its first voxel on the lattice of whole multiples of res from zero
bool regionLattice(double res, const mapRegion& region, int key0[3], int dims[3], double origin[3]) {
    if (!region.set || !(res > 0)) return false;
    for (int a = 0; a < 3; ++a) {
        const double lo = std::floor(region.boxMin(a) / res), hi = std::ceil(region.boxMax(a) / res);
        if (!(hi > lo) || hi - lo > 4096 || !(std::fabs(lo) < 1e9)) return false;
        origin[a] = lo * res;
        key0[a] = (int)lo;
        dims[a] = (int)(hi - lo);
    }
    return true;
}
// the byte of voxel (ix, iy, iz) of that grid, through the map's public methods
uint8_t voxelByte(mapManager::occMap& map, const double origin[3], double res, int ix, int iy, int iz) {
    const Eigen::Vector3d c(origin[0] + (ix + 0.5) * res, origin[1] + (iy + 0.5) * res, origin[2] + (iz + 0.5) * res);
    uint8_t v = 0;
    if (map.isInflatedOccupied(c)) v |= 1u | 4u;
    if (map.isUnknown(c)) v |= 2u;
    return v;
}
// voxels [lo, lo + n) of that grid
void rasteriseVoxels(mapManager::occMap& map, const double origin[3], double res, const int lo[3], const int n[3], std::vector<uint8_t>& bytes) {
    bytes.assign((size_t)n[0] * n[1] * n[2], 0);
    for (int ix = 0; ix < n[0]; ++ix)
        for (int iy = 0; iy < n[1]; ++iy)
            for (int iz = 0; iz < n[2]; ++iz)
                bytes[((size_t)ix * n[1] + iy) * n[2] + iz] = voxelByte(map, origin, res, lo[0] + ix, lo[1] + iy, lo[2] + iz);
}
// [a, b) of doubles already floored / ceiled, clipped to [key0, key0 + dim) and moved there; false: nothing left
bool clipToGrid(double a, double b, int key0, int dim, int& lo, int& n) {
    const double from = std::max(a, (double)key0), to = std::min(b, (double)key0 + dim);
    if (!(to > from)) return false;
    lo = (int)(from - key0);
    n = (int)(to - from);
    return true;
}
}  // namespace

bool mapAdapter::rasterise(mapManager::occMap& map, const mapRegion& region, std::vector<uint8_t>& voxels, int dims[3], double origin[3]) {
    const double res = map.getRes();
    int key0[3];
    if (!regionLattice(res, region, key0, dims, origin)) return false;
    const int zero[3] = {0, 0, 0};
    rasteriseVoxels(map, origin, res, zero, dims, voxels);
    return true;
}

namespace {
// the voxels of [from, to) (zero-based lattice, already floored / ceiled) that lie in the region's grid
bool rasteriseClipped(mapManager::occMap& map, const mapRegion& region, const double from[3], const double to[3], std::vector<uint8_t>& bytes,
                      int lo[3], int n[3]) {
    const double res = map.getRes();
    int key0[3], dims[3];
    double origin[3];
    if (!regionLattice(res, region, key0, dims, origin)) return false;
    bool any = true;
    for (int a = 0; a < 3; ++a) any = clipToGrid(from[a], to[a], key0[a], dims[a], lo[a], n[a]) && any;   // (a NaN fails every comparison: empty)
    bytes.clear();
    if (any) rasteriseVoxels(map, origin, res, lo, n, bytes);
    else
        for (int a = 0; a < 3; ++a) lo[a] = n[a] = 0;
    return true;
}
}  // namespace

bool mapAdapter::rasteriseKeys(mapManager::occMap& map, const mapRegion& region, const int keyLo[3], const int keyN[3],
                               std::vector<uint8_t>& bytes, int lo[3], int n[3]) {
    const double from[3] = {(double)keyLo[0], (double)keyLo[1], (double)keyLo[2]};
    const double to[3] = {from[0] + keyN[0], from[1] + keyN[1], from[2] + keyN[2]};
    return rasteriseClipped(map, region, from, to, bytes, lo, n);
}

bool mapAdapter::rasteriseBox(mapManager::occMap& map, const mapRegion& region, const Eigen::Vector3d& subMin, const Eigen::Vector3d& subMax,
                              std::vector<uint8_t>& bytes, int lo[3], int n[3]) {
    const double res = map.getRes();
    if (!(res > 0)) return false;
    const double from[3] = {std::floor(subMin(0) / res), std::floor(subMin(1) / res), std::floor(subMin(2) / res)};
    const double to[3] = {std::ceil(subMax(0) / res), std::ceil(subMax(1) / res), std::ceil(subMax(2) / res)};
    return rasteriseClipped(map, region, from, to, bytes, lo, n);
}

namespace {
std::mutex g_genMutex;
struct MapRecord {
    uint64_t generation = 1;
    DirtyJournal journal;     // boxes in voxels of the zero-based lattice of the map's res
};
std::map<const mapManager::occMap*, MapRecord> g_generation;
mapAdapter::SnapshotTotals g_totals;

void countSnapshot(bool full, long long boxes, long long voxels) {
    std::lock_guard<std::mutex> lk(g_genMutex);
    if (full) ++g_totals.fullSnapshots;
    g_totals.regionUpdates += boxes;
    g_totals.regionVoxels += voxels;
}
}  // namespace

uint64_t mapAdapter::generation(const mapManager::occMap* map) {
    std::lock_guard<std::mutex> lk(g_genMutex);
    auto it = g_generation.find(map);
    return it == g_generation.end() ? 1 : it->second.generation;
}

void mapAdapter::bumpGeneration(const mapManager::occMap* map) {
    if (!map) return;
    std::lock_guard<std::mutex> lk(g_genMutex);
    ++g_generation[map].generation;       // (a new record starts at 1: the first bump gives 2)
}

void mapAdapter::bumpGeneration(mapManager::occMap* map, const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) {
    if (!map) return;
    const double res = map->getRes();
    int lo[3], n[3];
    bool box = res > 0;
    for (int a = 0; a < 3 && box; ++a) {
        const double from = std::floor(boxMin(a) / res), to = std::ceil(boxMax(a) / res);
        box = std::fabs(from) < 1e9 && std::fabs(to) < 1e9 && to > from;
        if (box) { lo[a] = (int)from; n[a] = (int)(to - from); }
    }
    std::lock_guard<std::mutex> lk(g_genMutex);
    MapRecord& r = g_generation[map];
    ++r.generation;
    if (box) r.journal.record(r.generation, lo, n);
}

bool mapAdapter::changesSince(const mapManager::occMap* map, uint64_t since, uint64_t now, std::vector<DirtyBox>& out) {
    std::lock_guard<std::mutex> lk(g_genMutex);
    auto it = g_generation.find(map);
    out.clear();
    return it != g_generation.end() && it->second.journal.changesSince(since, now, out);
}

mapAdapter::SnapshotTotals mapAdapter::snapshotTotals() {
    std::lock_guard<std::mutex> lk(g_genMutex);
    return g_totals;
}

bool mapAdapter::uploadSnapshot(vigo_context* dev, const std::shared_ptr<mapManager::occMap>& map, const mapRegion& region,
                                uint64_t& stamp) {
    if (!dev || !map) return false;
    std::vector<DirtyBox> boxes;
    std::vector<uint8_t> bytes;
#ifndef VIGO_WITH_ROS
    (void)region;
    if (stamp == map->version) return true;
    const int dims[3] = {map->nx(), map->ny(), map->nz()};
    // the region route: every change since `stamp` has its box, the boxes lie in the grid and hold fewer voxels than it
    bool byBoxes = vigo_update_grid_region_host != nullptr && map->journal().changesSince(stamp, map->version, boxes);
    long long voxels = 0;
    for (const DirtyBox& b : boxes)
        for (int a = 0; a < 3; ++a) byBoxes = byBoxes && b.lo[a] >= 0 && b.n[a] >= 0 && (long long)b.lo[a] + b.n[a] <= dims[a];
    for (size_t k = 0; k < boxes.size() && byBoxes; ++k) voxels += (long long)boxes[k].n[0] * boxes[k].n[1] * boxes[k].n[2];
    if (byBoxes && voxels < (long long)dims[0] * dims[1] * dims[2]) {
        for (const DirtyBox& b : boxes) {
            if (b.n[0] == 0 || b.n[1] == 0 || b.n[2] == 0) continue;
            bytes.resize((size_t)b.n[0] * b.n[1] * b.n[2]);
            for (int ix = 0; ix < b.n[0]; ++ix)       // the map's bytes of the box (they carry bit 0 already: raw mode)
                for (int iy = 0; iy < b.n[1]; ++iy)
                    std::copy_n(&map->voxels()[((size_t)(b.lo[0] + ix) * dims[1] + b.lo[1] + iy) * dims[2] + b.lo[2]], b.n[2],
                                &bytes[((size_t)ix * b.n[1] + iy) * b.n[2]]);
            if (vigo_update_grid_region_host(dev, b.lo, b.n, bytes.data(), nullptr) != VIGO_OK) return false;
        }
        countSnapshot(false, (long long)boxes.size(), voxels);
        stamp = map->version;
        return true;
    }
    const double o[3] = {map->origin()(0), map->origin()(1), map->origin()(2)};
    if (vigo_set_grid_host(dev, map->nx(), map->ny(), map->nz(), o, map->getRes(), map->voxels().data()) != VIGO_OK) return false;
    countSnapshot(true, 0, 0);
    stamp = map->version;
    return true;
#else
    const uint64_t gen = generation(map.get());
    if (stamp == gen) return true;        // current until an owner of this map asks for a refresh
    int dims[3], key0[3], lo[3], n[3];
    double origin[3];
    // the region route: every generation since `stamp` came with its box (refresh(boxMin, boxMax)); fewer voxels than the grid
    if (vigo_update_grid_region_host != nullptr && changesSince(map.get(), stamp, gen, boxes) && regionLattice(map->getRes(), region, key0, dims, origin)) {
        long long voxels = 0;
        for (const DirtyBox& b : boxes) {         // what of each box lies in this planner's grid
            long long inGrid = 1;
            for (int a = 0, l, m; a < 3; ++a) inGrid *= clipToGrid((double)b.lo[a], (double)b.lo[a] + b.n[a], key0[a], dims[a], l, m) ? m : 0;
            voxels += inGrid;
        }
        if (voxels < (long long)dims[0] * dims[1] * dims[2]) {
            voxels = 0;
            for (const DirtyBox& b : boxes) {
                if (!rasteriseKeys(*map, region, b.lo, b.n, bytes, lo, n)) return false;
                if (bytes.empty()) continue;      // the box misses this planner's region
                if (vigo_update_grid_region_host(dev, lo, n, bytes.data(), nullptr) != VIGO_OK) return false;
                voxels += (long long)bytes.size();
            }
            countSnapshot(false, (long long)boxes.size(), voxels);
            stamp = gen;
            return true;
        }
    }
    if (!rasterise(*map, region, bytes, dims, origin)) {
        std::cout << "[mapAdapter]: setMapRegion() must give the box to snapshot before planning on this map type." << std::endl;
        return false;
    }
    if (vigo_set_grid_host(dev, dims[0], dims[1], dims[2], origin, map->getRes(), bytes.data()) != VIGO_OK) return false;
    countSnapshot(true, 0, 0);
    stamp = gen;
    return true;
#endif
}

unsigned mapAdapter::nodeBits(const std::shared_ptr<mapManager::occMap>& map, const mapRegion& region, float x, float y, float z) {
    if (!map) return kOutside;
#ifndef VIGO_WITH_ROS
    (void)region;
    const double res = map->getRes();
    const Eigen::Vector3d o = map->origin();
    // octomap getMetricMin/Max (PO.cpp:572-577), then coordToKey: floor(coord * resolution_factor)
    if (x < o(0) || x > o(0) + map->nx() * res || y < o(1) || y > o(1) + map->ny() * res || z < o(2) || z > o(2) + map->nz() * res) return kOutside;
    const double rf = 1.0 / res;
    const int kx = (int)std::floor(rf * (double)x) - (int)std::floor(o(0) / res + 0.5);
    const int ky = (int)std::floor(rf * (double)y) - (int)std::floor(o(1) / res + 0.5);
    const int kz = (int)std::floor(rf * (double)z) - (int)std::floor(o(2) / res + 0.5);
    if (kx < 0 || ky < 0 || kz < 0 || kx >= map->nx() || ky >= map->ny() || kz >= map->nz()) return kUnknown;
    const unsigned v = map->voxels()[((size_t)kx * map->ny() + ky) * map->nz() + kz];
    return v & (kUnknown | kOccupied);
#else
    if (!region.set) return kOutside;
    if (x < region.boxMin(0) || x > region.boxMax(0) || y < region.boxMin(1) || y > region.boxMax(1) || z < region.boxMin(2) || z > region.boxMax(2))
        return kOutside;
    const Eigen::Vector3d p((double)x, (double)y, (double)z);
    unsigned v = 0;
    if (map->isUnknown(p)) v |= kUnknown;
    if (map->isInflatedOccupied(p)) v |= kOccupied;
    return v;
#endif
}

DeviceLink::~DeviceLink() {
    if (dev_) vigo_destroy(dev_);
}

void DeviceLink::setMap(const std::shared_ptr<mapManager::occMap>& map) {
    map_ = map;
    stamp_ = 0;
}

void DeviceLink::setRegion(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) {
    region_.set = true;
    region_.boxMin = boxMin;
    region_.boxMax = boxMax;
    stamp_ = 0;
}

void DeviceLink::refresh() {
    mapAdapter::bumpGeneration(map_.get());
    stamp_ = 0;
}

void DeviceLink::refresh(const Eigen::Vector3d& boxMin, const Eigen::Vector3d& boxMax) {
    if (!map_) return;
#ifndef VIGO_WITH_ROS
    // the dense map keeps its own journal, on its own lattice: the voxels the box touches, clipped to the map
    const double res = map_->getRes();
    const int dims[3] = {map_->nx(), map_->ny(), map_->nz()};
    int lo[3], n[3];
    for (int a = 0; a < 3; ++a) {
        const double from = std::max(std::floor((boxMin(a) - map_->origin()(a)) / res), 0.0);
        const double to = std::min(std::ceil((boxMax(a) - map_->origin()(a)) / res), (double)dims[a]);
        if (!(to > from)) { lo[a] = 0; n[a] = 0; }
        else { lo[a] = (int)from; n[a] = (int)(to - from); }
    }
    map_->markChanged(lo, n);
#else
    mapAdapter::bumpGeneration(map_.get(), boxMin, boxMax);   // stamp_ stays: it names the generation this handle holds
#endif
}

void DeviceLink::setDevice(int ordinal) {
    if (ordinal == ordinal_) return;
    if (dev_) { vigo_destroy(dev_); dev_ = nullptr; }
    stamp_ = 0;
    ordinal_ = ordinal;
}

DeviceLink::Sync DeviceLink::sync(bool needMap, const vigo_params_s* params) {
    if (needMap && !map_) return kNoMap;
    if (hipSetDevice(ordinal_) != hipSuccess) return kNoDevice;
    if (!dev_ && vigo_create(&dev_, ordinal_) != VIGO_OK) {
        dev_ = nullptr;
        return kNoHandle;
    }
    if (vigo_set_stream(dev_, vigo_host::threadStream()) != VIGO_OK) return kFailed;
    if (params && vigo_set_params(dev_, params) != VIGO_OK) return kFailed;
    if (map_ && !mapAdapter::uploadSnapshot(dev_, map_, region_, stamp_)) return kFailed;
    return kSynced;
}

}  // namespace trajPlanner
