// seedBlock.h — internal to the host facades: the two blocks bsplineTraj::seedOnDevice moves per group, every input of
// vigo_seed_paths in one upload and every output in one download.  No HIP, Eigen or ROS in here:
// tests/seed_block_check.cpp runs both layouts on host memory under the address sanitizer.
//
// A layout is ONE function, run on a null base to measure (its return value, whole 8-byte words, sizes the block) and on
// a real base to hand out the fields (as csrc/vigo_ws_layout.hpp does for the C-ABI layer's workspaces) — the host fills
// and reads the fields carved on its copy of a block, the call gets the ones carved on the device's, and the offsets
// cannot disagree.  The extents are the ones include/vigo.h gives for vigo_seed_paths' arguments.
#ifndef VIGO_HOST_SEED_BLOCK_H
#define VIGO_HOST_SEED_BLOCK_H
#include <cstddef>
#include <cstdint>

namespace vigo_host {

// a cursor over `base` (8-byte aligned): every field starts on a multiple of its element size, with no other padding
class BlockCarver {
public:
    explicit BlockCarver(void* base) : base_(static_cast<char*>(base)) {}
    template <class T>
    T* take(size_t count) {
        off_ = (off_ + sizeof(T) - 1) & ~(sizeof(T) - 1);
        T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return (off_ + 7) & ~(size_t)7; }

private:
    char* base_;
    size_t off_ = 0;
};

// T trajectories with S polynomial segments of degree deg in all
struct SeedIn {
    double *duration, *dt0, *controlPointDistance, *maxPathLength, *prevSeed, *prevFit;   // [T] each
    double* knots;      // [S + T]
    double* coeffs;     // [S][3][deg + 1]
    int32_t* segOff;    // [T + 1]
};
inline size_t seedInBlock(void* base, size_t T, size_t S, size_t deg, SeedIn& f) {
    BlockCarver c(base);
    f.duration = c.take<double>(T); f.dt0 = c.take<double>(T); f.controlPointDistance = c.take<double>(T);
    f.maxPathLength = c.take<double>(T); f.prevSeed = c.take<double>(T); f.prevFit = c.take<double>(T);
    f.knots = c.take<double>(S + T);
    f.coeffs = c.take<double>(S * 3 * (deg + 1));
    f.segOff = c.take<int32_t>(T + 1);
    return c.bytes();
}

// ... followed by the start / end conditions of the fit, [T][4][3], when the launch's fit points stay on the device
// for vigo_bspline_fit_mixed (bsplineTraj::setMixedFit): the same block, one upload
inline size_t seedInBlockWithConds(void* base, size_t T, size_t S, size_t deg, SeedIn& f, double*& conds) {
    const size_t head = seedInBlock(base, T, S, deg, f);        // whole 8-byte words
    conds = base ? reinterpret_cast<double*>(static_cast<char*>(base) + head) : nullptr;
    return head + T * 12 * sizeof(double);
}

// cap: rows of the seed / fit points per trajectory
struct SeedOut {
    int32_t *status, *tries, *seedN, *fitN;           // [T] each
    double *dt, *finalTime, *prevSeed, *prevFit;      // [T] each
    double *seed, *fit;                               // [T][cap][3] each
};
inline size_t seedOutBlock(void* base, size_t T, size_t cap, SeedOut& f) {
    BlockCarver c(base);
    f.status = c.take<int32_t>(T); f.tries = c.take<int32_t>(T); f.seedN = c.take<int32_t>(T); f.fitN = c.take<int32_t>(T);
    f.dt = c.take<double>(T); f.finalTime = c.take<double>(T); f.prevSeed = c.take<double>(T); f.prevFit = c.take<double>(T);
    f.seed = c.take<double>(T * cap * 3);
    f.fit = c.take<double>(T * cap * 3);
    return c.bytes();
}

}  // namespace vigo_host
#endif  /* VIGO_HOST_SEED_BLOCK_H */
