// ref_shim/map_manager/occupancyMap.h — TEST INFRASTRUCTURE ONLY.
//
// mapManager::occMap is an EXTERNAL dependency of the reference (package map_manager, not vendored by it).  This class is
// NOT that package: it is this build's own dense voxel contract (include/vigo.h "voxel map"; the same arithmetic as
// host/include/.../standin/dense_occmap.h and oracle/vigo_oracle.c's grid) behind the four methods the reference calls.
// What the compiled reference sources compute is therefore the reference's code over THIS map definition.
// (dense_occmap.h itself cannot be included here: it brings the facades' mini_eigen.h, a second namespace Eigen.)
#ifndef REF_SHIM_MAP_MANAGER_OCCUPANCY_MAP_H
#define REF_SHIM_MAP_MANAGER_OCCUPANCY_MAP_H
#include <Eigen/Eigen>
#include <ros/ros.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <queue>
#include <set>
#include <vector>

namespace mapManager {
// byte per voxel: bit0 inflated-occupied, bit1 unknown, bit2 occupied; index = floor((p - origin) / res);
// a point outside the box is occupied and unknown
class occMap {
public:
    occMap(int nx, int ny, int nz, const double origin[3], double res, const uint8_t* vox)
        : nx_(nx), ny_(ny), nz_(nz), res_(res), vox_(vox, vox + static_cast<size_t>(nx) * ny * nz) {
        for (int a = 0; a < 3; ++a) origin_[a] = origin[a];
    }
    double getRes() { return res_; }
    unsigned byteAt(const Eigen::Vector3d& p) const {
        const int ix = static_cast<int>(std::floor((p(0) - origin_[0]) / res_));
        const int iy = static_cast<int>(std::floor((p(1) - origin_[1]) / res_));
        const int iz = static_cast<int>(std::floor((p(2) - origin_[2]) / res_));
        if (ix < 0 || iy < 0 || iz < 0 || ix >= nx_ || iy >= ny_ || iz >= nz_) return 0xFFu;
        return vox_[(static_cast<size_t>(ix) * ny_ + iy) * nz_ + iz];
    }
    bool isInflatedOccupied(const Eigen::Vector3d& p) { return byteAt(p) & 1u; }
    bool isUnknown(const Eigen::Vector3d& p) { return (byteAt(p) >> 1) & 1u; }
    // both ends, then int(dist / res) - 1 probes spaced res along the line; the length sums (dx² + dy²) + dz² whatever the
    // Eigen shim's reduction switch says: this is the map's arithmetic, not the reference's
    bool isInflatedOccupiedLine(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2) {
        if (isInflatedOccupied(p1) || isInflatedOccupied(p2)) return true;
        const double d[3] = {p2(0) - p1(0), p2(1) - p1(1), p2(2) - p1(2)};
        const double dist = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        const double inc[3] = {d[0] / dist * res_, d[1] / dist * res_, d[2] / dist * res_};
        const int steps = static_cast<int>(dist / res_);
        for (int i = 1; i < steps; ++i) {
            if (isInflatedOccupied(Eigen::Vector3d(p1(0) + i * inc[0], p1(1) + i * inc[1], p1(2) + i * inc[2]))) return true;
        }
        return false;
    }

private:
    int nx_, ny_, nz_;
    double origin_[3];
    double res_;
    std::vector<uint8_t> vox_;
};
}  // namespace mapManager
#endif
