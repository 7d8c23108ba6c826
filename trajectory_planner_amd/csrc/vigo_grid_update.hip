// vigo_grid_update.hip — vigo_update_grid_region: a box of voxels written into the handle's three bit planes in place, and,
// in inflate mode, plane 0 re-inflated around it.  Each kernel is one word function of vigo_grid_update_core.hpp (the rule,
// the windows and the masks are stated there) or of vigo_dilate_bits.hpp per thread.  One launch in raw mode, six in inflate
// mode (write, gather, dilate z, y, x, write back), all on the handle's stream, each a plain pass over words: the work is
// that of the box grown by 2r, not of the grid.  No atomics: a thread owns the words it writes.
#include "vigo_dilate_bits.hpp"
#include "vigo_grid_update_core.hpp"
#include "vigo_internal.hpp"

namespace vigo {
namespace {

__global__ void k_region_write(RegionPlan p, size_t n_words, const uint8_t* __restrict__ vox, uint32_t* __restrict__ planes, size_t plane_words) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_words) region_write_word(p, t, vox, planes, plane_words);
}
__global__ void k_region_gather(RegionPlan p, size_t n_words, const uint32_t* __restrict__ occupied, uint32_t* __restrict__ compact) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_words) region_gather_word(p, t, occupied, compact);
}
__global__ void k_region_back(RegionPlan p, size_t n_words, const uint32_t* __restrict__ compact, uint32_t* __restrict__ inflated) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_words) region_back_word(p, t, compact, inflated);
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int launch_grid_region(hipStream_t s, const RegionPlan& p, const uint8_t* vox, uint32_t* planes, size_t plane_words,
                       uint32_t* planeA, uint32_t* planeB) {
    const size_t nb = region_box_words(p);
    hipLaunchKernelGGL(k_region_write, dim3(blocks_of(nb)), dim3(256), 0, s, p, nb, vox, planes, plane_words);
    if (p.inflate) {
        const size_t nw = region_window_words(p), n1 = region_back_words(p);
        const unsigned gw = blocks_of(nw);
        hipLaunchKernelGGL(k_region_gather, dim3(gw), dim3(256), 0, s, p, nw, planes + 2 * plane_words, planeA);
        hipLaunchKernelGGL(k_dilate_bits_z, dim3(gw), dim3(256), 0, s, p.cnz, p.cw, nw, p.r[2], planeA, planeB);
        hipLaunchKernelGGL(k_dilate_bits_rows, dim3(gw), dim3(256), 0, s, nw, (size_t)p.cw, p.cy, p.r[1], planeB, planeA);
        hipLaunchKernelGGL(k_dilate_bits_rows, dim3(gw), dim3(256), 0, s, nw, (size_t)p.cy * p.cw, p.cx, p.r[0], planeA, planeB);
        hipLaunchKernelGGL(k_region_back, dim3(blocks_of(n1)), dim3(256), 0, s, p, n1, planeB, planes);
    }
    return (int)hipGetLastError();
}

}  // namespace vigo
