// vigo_grid_update_core.hpp — the index arithmetic of vigo_update_grid_region (include/vigo.h, "voxel map"), once: the
// kernels of vigo_grid_update.hip are one call of a *_word function per thread, tests/grid_update_check.cpp walks the same
// functions thread index by thread index on the CPU, and grid_region_apply below is the host twin
// (vigo_grid_region_apply_host) on the byte grid.
//
// The snapshot: three bit planes of nx * ny * nzw words, nzw = ceil(nz / 32); voxel (x, y, z) is bit z % 32 of word
// (x * ny + y) * nzw + z / 32; the bits of a z-row's last word beyond nz are padding and stay clear.
//
// The box [lo, lo + n) touches the z-words bw0 .. bw0 + bnw - 1 of each of its n[0] * n[1] rows.  ONE thread owns ONE such
// word in all three planes: new = (old & ~mask) | bits, mask = the bits of [lo_z, lo_z + n_z) that fall into the word —
// so the padding is never written, and no two threads write one word.
//
// Inflate mode (r given): plane 0 becomes, on the box grown by r (clipped to the grid: window 1), the box dilation of
// plane 2.  A voxel of window 1 sees occupied voxels at most r away, all of them inside the box grown by 2r (window 2,
// clipped) or outside the grid, where there is nothing.  Window 2's part of plane 2 is gathered — whole z-words, word
// aligned with the snapshot, so the gather is a copy — into a compact plane of cx * cy * cw words, dilated there along
// z, y, x by vigo_dilate_bits.hpp (bits that the window's words hold beyond window 2 are further than r from window 1, as
// is everything the compact plane leaves out), and window 1 is written back to plane 0 under the same kind of z mask.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#ifndef VIGO_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_HD __host__ __device__ __forceinline__
#else
#define VIGO_HD inline
#endif
#endif

namespace vigo {

enum RegionCheck { kRegionOk = 0, kRegionEmpty, kRegionInvalid, kRegionUnsupported };
constexpr int kRegionMaxRz = 31;   // vigo_inflate_grid's limit: the z dilation reads one neighbour word each side

// what the entry points refuse, in their order (pointers: the caller's business); r == nullptr: raw mode
inline RegionCheck region_check(int nx, int ny, int nz, const int32_t lo[3], const int32_t n[3], const int32_t* r) {
    const int dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        if (lo[a] < 0 || n[a] < 0 || (r && r[a] < 0)) return kRegionInvalid;
        if ((int64_t)lo[a] + n[a] > dims[a]) return kRegionInvalid;
    }
    if (r && r[2] > kRegionMaxRz) return kRegionUnsupported;
    for (int a = 0; a < 3; ++a)
        if (n[a] == 0) return kRegionEmpty;
    return kRegionOk;
}

struct RegionPlan {
    int nx, ny, nz, nzw;
    int lo[3], n[3];
    int inflate;          // 0: raw mode, the windows below are unset
    int r[3];             // min(r, dim) per axis
    int bw0, bnw;         // the box' z-words: first, count
    int a1[3], e1[3];     // window 1 = box grown by r, clipped: [a1, e1)
    int w1_0, w1_n;       //   its z-words
    int a2[3], e2[3];     // window 2 = box grown by 2r, clipped
    int w2_0;             //   its first z-word
    int cx, cy, cw;       // the compact plane: rows and words per row
    int cnz;              // nz seen from the compact plane's first word (the z dilation's padding mask)
};

VIGO_HD int region_clip(int64_t v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// a checked (kRegionOk) box
inline RegionPlan region_plan(int nx, int ny, int nz, const int32_t lo[3], const int32_t n[3], const int32_t* r) {
    RegionPlan p{};
    p.nx = nx; p.ny = ny; p.nz = nz; p.nzw = (nz + 31) / 32;
    const int dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) { p.lo[a] = lo[a]; p.n[a] = n[a]; }
    p.bw0 = lo[2] / 32;
    p.bnw = (lo[2] + n[2] - 1) / 32 - p.bw0 + 1;
    p.inflate = r != nullptr;
    if (!r) return p;
    for (int a = 0; a < 3; ++a) {
        p.r[a] = r[a] < dims[a] ? r[a] : dims[a];   // a larger radius reaches no further: keeps c + r an int
        p.a1[a] = region_clip((int64_t)lo[a] - r[a], dims[a]);
        p.e1[a] = region_clip((int64_t)lo[a] + n[a] + r[a], dims[a]);
        p.a2[a] = region_clip((int64_t)lo[a] - 2 * (int64_t)r[a], dims[a]);
        p.e2[a] = region_clip((int64_t)lo[a] + n[a] + 2 * (int64_t)r[a], dims[a]);
    }
    p.w1_0 = p.a1[2] / 32;
    p.w1_n = (p.e1[2] - 1) / 32 - p.w1_0 + 1;
    p.w2_0 = p.a2[2] / 32;
    p.cw = (p.e2[2] - 1) / 32 - p.w2_0 + 1;
    p.cx = p.e2[0] - p.a2[0];
    p.cy = p.e2[1] - p.a2[1];
    p.cnz = nz - 32 * p.w2_0;
    return p;
}

// threads of the three steps (one word each), and the compact plane's words
VIGO_HD size_t region_box_words(const RegionPlan& p) { return (size_t)p.n[0] * p.n[1] * p.bnw; }
VIGO_HD size_t region_window_words(const RegionPlan& p) { return p.inflate ? (size_t)p.cx * p.cy * p.cw : 0; }
VIGO_HD size_t region_back_words(const RegionPlan& p) { return p.inflate ? (size_t)(p.e1[0] - p.a1[0]) * (p.e1[1] - p.a1[1]) * p.w1_n : 0; }

// the bits of z-word w that [za, zb) covers; *first: the lowest of them (32 and a zero mask when there is none)
VIGO_HD uint32_t region_word_mask(int za, int zb, int w, int* first, int* count) {
    const int b0 = za - 32 * w < 0 ? 0 : za - 32 * w, b1 = zb - 32 * w > 32 ? 32 : zb - 32 * w;
    const int cnt = b1 - b0;
    *first = b0;
    *count = cnt > 0 ? cnt : 0;
    if (cnt <= 0) return 0u;
    return cnt >= 32 ? 0xffffffffu : ((1u << cnt) - 1u) << b0;
}

// one destination word per plane from cnt bytes of a row, the first of them landing on bit `shift` (shift + cnt <= 32);
// a whole word from a 16-byte aligned row goes by two 16-byte loads as in k_pack_grid, the rest byte by byte
VIGO_HD void region_build_word(const uint8_t* src, int cnt, int shift, uint32_t b[3]) {
    b[0] = b[1] = b[2] = 0;
    if (cnt == 32 && ((reinterpret_cast<uintptr_t>(src) & 15) == 0)) {
        uint32_t wds[8];
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        const uint4 q0 = s4[0], q1 = s4[1];
        wds[0] = q0.x; wds[1] = q0.y; wds[2] = q0.z; wds[3] = q0.w;
        wds[4] = q1.x; wds[5] = q1.y; wds[6] = q1.z; wds[7] = q1.w;
#else
        memcpy(wds, src, 32);
#endif
        for (int i = 0; i < 8; ++i) {
            for (int j = 0; j < 4; ++j) {
                const uint32_t v = (wds[i] >> (8 * j)) & 0xFFu;
                const int bit = 4 * i + j;
                b[0] |= (v & 1u) << bit;
                b[1] |= ((v >> 1) & 1u) << bit;
                b[2] |= ((v >> 2) & 1u) << bit;
            }
        }
    } else {
        for (int i = 0; i < cnt; ++i) {
            const uint32_t v = src[i];
            b[0] |= (v & 1u) << (shift + i);
            b[1] |= ((v >> 1) & 1u) << (shift + i);
            b[2] |= ((v >> 2) & 1u) << (shift + i);
        }
    }
}

// step 1, thread t < region_box_words: the box' bytes vox[n0][n1][n2] into word (row, bw0 + t % bnw) of the planes (plane 0
// is left alone in inflate mode)
VIGO_HD void region_write_word(const RegionPlan& p, size_t t, const uint8_t* vox, uint32_t* planes, size_t plane_words) {
    const int k = (int)(t % p.bnw);
    const size_t row = t / p.bnw;
    const int j = (int)(row % p.n[1]), i = (int)(row / p.n[1]);
    const int w = p.bw0 + k;
    int first, cnt;
    const uint32_t mask = region_word_mask(p.lo[2], p.lo[2] + p.n[2], w, &first, &cnt);
    const uint8_t* src = vox + row * p.n[2] + (size_t)(32 * w + first - p.lo[2]);
    uint32_t b[3];
    region_build_word(src, cnt, first, b);
    const size_t wi = ((size_t)(p.lo[0] + i) * p.ny + (p.lo[1] + j)) * p.nzw + w;
    for (int pl = p.inflate ? 1 : 0; pl < 3; ++pl) {
        uint32_t* dst = planes + pl * plane_words + wi;
        *dst = (*dst & ~mask) | (b[pl] & mask);
    }
}

// step 2, thread t < region_window_words: window 2's word of the occupied plane into the compact plane
VIGO_HD void region_gather_word(const RegionPlan& p, size_t t, const uint32_t* occupied, uint32_t* compact) {
    const int k = (int)(t % p.cw);
    const size_t row = t / p.cw;
    const int j = (int)(row % p.cy), i = (int)(row / p.cy);
    compact[t] = occupied[((size_t)(p.a2[0] + i) * p.ny + (p.a2[1] + j)) * p.nzw + p.w2_0 + k];
}

// step 4 (3 is the dilation), thread t < region_back_words: window 1's word of the dilated compact plane into plane 0
VIGO_HD void region_back_word(const RegionPlan& p, size_t t, const uint32_t* compact, uint32_t* inflated) {
    const int k = (int)(t % p.w1_n);
    const size_t row = t / p.w1_n;
    const int ny1 = p.e1[1] - p.a1[1];
    const int y = p.a1[1] + (int)(row % ny1), x = p.a1[0] + (int)(row / ny1);
    const int w = p.w1_0 + k;
    int first, cnt;
    const uint32_t mask = region_word_mask(p.a1[2], p.e1[2], w, &first, &cnt);
    const uint32_t bits = compact[((size_t)(x - p.a2[0]) * p.cy + (y - p.a2[1])) * p.cw + (w - p.w2_0)];
    uint32_t* dst = inflated + ((size_t)x * p.ny + y) * p.nzw + w;
    *dst = (*dst & ~mask) | (bits & mask);
}

// The host twin on the byte grid vox[nx][ny][nz]: the box' bytes are assigned (inflate mode: all but bit 0), then bit 0 of
// window 1 := OR of bit 2 over |d| <= r per axis, one axis at a time on a byte copy of window 2.  Returns a RegionCheck;
// nothing is written unless it is kRegionOk.
inline RegionCheck grid_region_apply(int nx, int ny, int nz, uint8_t* vox, const int32_t lo[3], const int32_t n[3],
                                     const uint8_t* box, const int32_t* r) {
    const RegionCheck rc = region_check(nx, ny, nz, lo, n, r);
    if (rc != kRegionOk) return rc;
    const RegionPlan p = region_plan(nx, ny, nz, lo, n, r);
    for (int i = 0; i < n[0]; ++i)
        for (int j = 0; j < n[1]; ++j) {
            uint8_t* dst = vox + ((size_t)(lo[0] + i) * ny + (lo[1] + j)) * nz + lo[2];
            const uint8_t* src = box + ((size_t)i * n[1] + j) * n[2];
            for (int k = 0; k < n[2]; ++k) dst[k] = r ? (uint8_t)((src[k] & ~1u) | (dst[k] & 1u)) : src[k];
        }
    if (!r) return kRegionOk;
    const int d[3] = {p.e2[0] - p.a2[0], p.e2[1] - p.a2[1], p.e2[2] - p.a2[2]};
    const size_t stride[3] = {(size_t)d[1] * d[2], (size_t)d[2], 1};
    std::vector<uint8_t> cur((size_t)d[0] * d[1] * d[2]), nxt(cur.size());
    for (int x = 0; x < d[0]; ++x)
        for (int y = 0; y < d[1]; ++y)
            for (int z = 0; z < d[2]; ++z)
                cur[x * stride[0] + y * stride[1] + z] = (vox[((size_t)(p.a2[0] + x) * ny + (p.a2[1] + y)) * nz + p.a2[2] + z] >> 2) & 1u;
    for (int axis = 2; axis >= 0; --axis) {
        for (int x = 0; x < d[0]; ++x)
            for (int y = 0; y < d[1]; ++y)
                for (int z = 0; z < d[2]; ++z) {
                    const int c[3] = {x, y, z};
                    const size_t at = x * stride[0] + y * stride[1] + z;
                    const int from = c[axis] - p.r[axis] < 0 ? -c[axis] : -p.r[axis];
                    const int to = c[axis] + p.r[axis] >= d[axis] ? d[axis] - 1 - c[axis] : p.r[axis];
                    uint8_t acc = 0;
                    for (int e = from; e <= to; ++e) acc |= cur[(ptrdiff_t)at + e * (ptrdiff_t)stride[axis]];
                    nxt[at] = acc;
                }
        cur.swap(nxt);
    }
    for (int x = p.a1[0]; x < p.e1[0]; ++x)
        for (int y = p.a1[1]; y < p.e1[1]; ++y)
            for (int z = p.a1[2]; z < p.e1[2]; ++z) {
                uint8_t& v = vox[((size_t)x * ny + y) * nz + z];
                v = (uint8_t)((v & ~1u) | cur[(x - p.a2[0]) * stride[0] + (y - p.a2[1]) * stride[1] + (z - p.a2[2])]);
            }
    return kRegionOk;
}

}  // namespace vigo
