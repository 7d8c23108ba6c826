// vigo_esdf_core.hpp — the rule of the ESDF build (vigo_build_esdf, vigo_esdf_from_voxels_host): the EXACT Euclidean
// distance transform of the voxel snapshot in integer voxel units, as the kernels of vigo_esdf_build.hip run it and
// the host compiles too (esdf_from_voxels below is the host twin, the same functions in plain loops;
// tests/test_esdf_build_core.py pins it against the all-pairs definition and scipy's EDT).
//
// Definitions (include/vigo.h, vigo_build_esdf):
//   sites      the voxels whose bit is set in the chosen plane (0 inflated-occupied, 2 occupied), OR the unknown
//              plane when unknown_is_site; bits of a z-row's last word beyond nz are PADDING: in neither set
//   d2_site    min dx^2 + dy^2 + dz^2 to a site (0 on a site); d2_free the same to a non-site voxel of the lattice
//   empty set  its squared distance is E = nx^2 + ny^2 + nz^2 everywhere (finite, above anything attainable inside)
//   value      (float)((sqrt((double)d2_site) - sqrt((double)d2_free)) * res), every operation rounded once
//
// One signed integer per voxel carries both fields: a voxel is a site or it is not, so exactly one of d2_site, d2_free
// is 0 there — and that holds after every pass, because the 1-D distance of a set's own member is 0 already.  A
// non-site voxel stores +d2_site (> 0), a site voxel stores -d2_free (< 0); a reader that looks for the nearest site
// takes max(v, 0) of what it reads, one that looks for the nearest non-site max(-v, 0).  Half the memory and the work
// of two transforms.
//
// The transform is separable: first the 1-D squared distance along z, straight from the packed words (count leading /
// trailing zeros; no byte grid), then out[i] = min_j (in[j] + (i - j)^2) along y and along x.  esdf_line_value finds
// that minimum by an outward scan from j = i that stops at the first radius r with r^2 >= best: every in[j] is >= 0, so
// no j further out can lower the minimum — the integer result is exact, not approximate.
//
// Sentinel and overflow: a z-row without a member of the wanted set gets E itself as its squared 1-D distance (it is
// stored squared; nothing is squared later).  The entry points refuse lattices with E > 2^30.  Every stored magnitude is
// then <= E: the z pass writes d^2 <= (nz - 1)^2 < E or E, and a line pass returns at most its own in[i].  The scan adds
// r^2 only while r^2 < best <= E, so every sum in[j] + r^2 is <= E + (E - 1) <= 2^31 - 1: it fits an int32.
// E + anything >= E exceeds every attainable distance ((nx-1)^2 + (ny-1)^2 + (nz-1)^2 < E), so a sentinel never wins
// against a real member, and where the set is empty the minimum is E (the j = i term) — the empty-set rule.
//
// Integer logic; the output value is two fp64 square roots, one subtraction, one product, one conversion.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <new>
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

constexpr int64_t kEsdfMaxEmptyD2 = (int64_t)1 << 30;
constexpr int64_t kEsdfMaxVoxels = (int64_t)1 << 33;            // vigo_set_esdf's cap on a lattice

// E = nx^2 + ny^2 + nz^2 (the squared distance to an empty set), or 0 when the lattice is refused: an axis < 2, E
// beyond kEsdfMaxEmptyD2 (see the header: int32 sums), or more than kEsdfMaxVoxels voxels — one test for both entries
VIGO_HD int32_t esdf_empty_d2(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return 0;
    const int64_t e = (int64_t)nx * nx + (int64_t)ny * ny + (int64_t)nz * nz;
    if (e > kEsdfMaxEmptyD2) return 0;                          // every axis <= 2^15 from here on: the product fits
    return (int64_t)nx * ny * nz <= kEsdfMaxVoxels ? (int32_t)e : 0;
}

// word w of a z-row of the wanted set: the sites' word, or its complement; the padding bits are in neither
VIGO_HD uint32_t esdf_set_word(uint32_t sites, int w, int nz, bool complement) {
    const int valid = nz - 32 * w;
    const uint32_t mask = valid >= 32 ? 0xffffffffu : (1u << valid) - 1u;
    return (complement ? ~sites : sites) & mask;
}

// distance along z from voxel z to the nearest set bit of a row of nzw words (word(w) -> uint32), -1: none
template <typename Word>
VIGO_HD int esdf_nearest_bit(const Word& word, int nzw, int z) {
    const int w0 = z >> 5, b = z & 31;
    const uint32_t m = word(w0);
    int down = -1, up = -1;
    const uint32_t lo = m & (0xffffffffu >> (31 - b));          // bits 0 .. b
    if (lo) down = b - (31 - __builtin_clz(lo));
    else
        for (int w = w0 - 1; w >= 0; --w) {
            const uint32_t v = word(w);
            if (v) { down = z - (32 * w + 31 - __builtin_clz(v)); break; }
        }
    const uint32_t hi = m & (0xffffffffu << b);                 // bits b .. 31
    if (hi) up = __builtin_ctz(hi) - b;
    else
        for (int w = w0 + 1; w < nzw; ++w) {
            const uint32_t v = word(w);
            if (v) { up = 32 * w + __builtin_ctz(v) - z; break; }
        }
    if (down < 0) return up;
    if (up < 0) return down;
    return down < up ? down : up;
}

// first pass: the signed squared 1-D distance of voxel z of a row (sites(w) -> the row's site word w)
template <typename Sites>
VIGO_HD int32_t esdf_z_value(const Sites& sites, int nz, int nzw, int z, int32_t E) {
    const bool site = ((sites(z >> 5) >> (z & 31)) & 1u) != 0;
    const int d = esdf_nearest_bit([&](int w) { return esdf_set_word(sites(w), w, nz, site); }, nzw, z);
    const int32_t a = d < 0 ? E : d * d;                        // d <= nz - 1 < 2^15
    return site ? -a : a;
}

// y and x passes: the signed value of element i of a line of n (in(j) -> the signed value of element j)
template <typename In>
VIGO_HD int32_t esdf_line_value(const In& in, int n, int i) {
    const int32_t s = in(i);
    const bool site = s < 0;
    int32_t best = site ? -s : s;
    for (int r = 1; r < n; ++r) {
        const int32_t rr = r * r;
        if (rr >= best) break;
        const int lo = i - r, hi = i + r;
        if (lo < 0 && hi >= n) break;
        if (lo >= 0) {
            int32_t v = in(lo);
            v = site ? -v : v;
            v = (v > 0 ? v : 0) + rr;
            best = v < best ? v : best;
        }
        if (hi < n) {
            int32_t v = in(hi);
            v = site ? -v : v;
            v = (v > 0 ? v : 0) + rr;
            best = v < best ? v : best;
        }
    }
    return site ? -best : best;
}

// the output value from the signed squared distance
VIGO_HD float esdf_compose(int32_t s, double res) {
    const int32_t d2_site = s > 0 ? s : 0, d2_free = s < 0 ? -s : 0;
    return (float)((sqrt((double)d2_site) - sqrt((double)d2_free)) * res);
}

// The host twin (vigo_esdf_from_voxels_host): the byte grid's plane bit — OR the unknown bit — packed like the
// snapshot (bit k of word w = voxel z = 32 w + k), then the three passes above in plain loops.  0, or -1 for a bad
// argument, -6 for a lattice beyond kEsdfMaxEmptyD2 or kEsdfMaxVoxels, or one whose working memory (8 bytes per voxel
// and the packed words) the host cannot allocate (VIGO_ERR_INVALID_ARG / VIGO_ERR_UNSUPPORTED); nothing is written
// then, and no exception leaves the function: its caller is extern "C".
inline int esdf_from_voxels(int nx, int ny, int nz, const uint8_t* vox, int plane, int unknown_is_site, double res, float* out) {
    if (!vox || !out || (plane != 0 && plane != 2) || nx < 2 || ny < 2 || nz < 2 || !(res > 0.0) || !(res < INFINITY)) return -1;
    const int32_t E = esdf_empty_d2(nx, ny, nz);
    if (E == 0) return -6;
    const int nzw = (nz + 31) / 32;
    const size_t rows = (size_t)nx * ny, total = rows * nz;
    const unsigned pick = (1u << plane) | (unknown_is_site ? 2u : 0u);
    std::vector<uint32_t> words;
    std::vector<int32_t> a, b;
    try {
        words.assign(rows * nzw, 0u);
        a.resize(total);
        b.resize(total);
    } catch (const std::bad_alloc&) {
        return -6;
    }
    for (size_t row = 0; row < rows; ++row)
        for (int z = 0; z < nz; ++z)
            if (vox[row * nz + z] & pick) words[row * nzw + (z >> 5)] |= 1u << (z & 31);
    for (size_t row = 0; row < rows; ++row) {
        const uint32_t* rw = &words[row * nzw];
        for (int z = 0; z < nz; ++z) a[row * nz + z] = esdf_z_value([rw](int w) { return rw[w]; }, nz, nzw, z, E);
    }
    for (int x = 0; x < nx; ++x)
        for (int y = 0; y < ny; ++y)
            for (int z = 0; z < nz; ++z) {
                const int32_t* line = &a[(size_t)x * ny * nz + z];
                b[((size_t)x * ny + y) * nz + z] = esdf_line_value([line, nz](int j) { return line[(size_t)j * nz]; }, ny, y);
            }
    const size_t sx = (size_t)ny * nz;
    for (int x = 0; x < nx; ++x)
        for (size_t r = 0; r < sx; ++r) {
            const int32_t* line = &b[r];
            out[(size_t)x * sx + r] = esdf_compose(esdf_line_value([line, sx](int j) { return line[(size_t)j * sx]; }, nx, x), res);
        }
    return 0;
}

}  // namespace vigo
