// vigo_esdf_core.hpp — the rule of the ESDF build (vigo_build_esdf, vigo_esdf_from_voxels_host): the EXACT Euclidean
// distance transform of the voxel snapshot in integer voxel units, as the kernels of vigo_esdf_build.hip run it and
// the host compiles too (esdf_from_voxels below is the host twin, the same functions in plain loops;
// tests/test_esdf_build_core.py pins it against the all-pairs definition and scipy's EDT).  The region update
// (vigo_update_esdf, vigo_esdf_update_host) is further down: the same three value functions on the lines a changed box
// reaches.
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

// ---- Region update (vigo_update_esdf, vigo_esdf_update_host) ---------------------------------------------------------
// The three passes keep their results: A (z pass), B (y pass), L (the lattice).  A y-pass line (x, ., z) depends on its
// own A line and nothing else, an x-pass line (., y, z) on its own B line — so after the sites of a box changed, a line
// whose input did not change needs no work, and what is recomputed equals a whole rebuild bit for bit.  Flags carry
// "the pass before changed a value on this line": fy[(x - lo_x) * nz + z] for the y lines of the box' slab, fx[y * nz + z]
// for the x lines.  A flag is set if and only if such a value changed; every writer stores 1.  No pass scans the array
// it writes (z: words -> A, y: A -> B, x: B -> L; the compare reads the old value at the address it stores to), so
// threads of a pass never race.  One function per thread and pass: the kernels of vigo_esdf_build.hip are one call each,
// over esdf_region_grid() blocks of kEsdfRegionBlock (the surplus threads of the last block leave at the first line),
// esdf_update below is the same calls in plain loops, tests/esdf_update_check.cpp walks them thread index by thread index.
struct EsdfRegion {
    int nx, ny, nz, nzw;
    int lo[3], n[3];      // the box [lo, lo + n) inside the lattice, every n > 0
    int32_t E;
};
// what a tracked build keeps for the updates (carved by ws_esdf_track of vigo_ws_layout.hpp): 12 bytes per voxel, then
// the two line counts and the flags — one run of clear_bytes from `counters` on, cleared ahead of the passes
struct EsdfTrackWs {
    int32_t *a, *b;                  // nx * ny * nz each
    float* lattice;                  // nx * ny * nz, row-major
    unsigned long long* counters;    // y_lines, x_lines of the last update that was asked for them
    uint8_t *fy, *fx;                // nx * nz (a box uses its first n[0] * nz), ny * nz
    size_t clear_bytes;
};
constexpr int kEsdfRegionBlock = 256;
VIGO_HD size_t esdf_region_grid(size_t threads) { return (threads + kEsdfRegionBlock - 1) / kEsdfRegionBlock; }
// threads of the passes: the box' columns x nz; its slab of x x ny x nz; the whole lattice
VIGO_HD size_t esdf_region_z_threads(const EsdfRegion& r) { return (size_t)r.n[0] * r.n[1] * r.nz; }
VIGO_HD size_t esdf_region_y_threads(const EsdfRegion& r) { return (size_t)r.n[0] * r.ny * r.nz; }
VIGO_HD size_t esdf_region_x_threads(const EsdfRegion& r) { return (size_t)r.nx * r.ny * r.nz; }

inline EsdfRegion esdf_region(int nx, int ny, int nz, const int32_t lo[3], const int32_t n[3]) {
    EsdfRegion r{};
    r.nx = nx; r.ny = ny; r.nz = nz; r.nzw = (nz + 31) / 32;
    for (int a = 0; a < 3; ++a) { r.lo[a] = lo[a]; r.n[a] = n[a]; }
    r.E = esdf_empty_d2(nx, ny, nz);
    return r;
}

// z pass, thread t: voxel z of column (x, y) of the box' footprint — every z, not only the box' own — from the current
// packed words (unk_plane: ORed in, or nullptr)
VIGO_HD void esdf_region_z(const EsdfRegion& r, size_t t, const uint32_t* site_plane, const uint32_t* unk_plane, int32_t* a, uint8_t* fy) {
    if (t >= esdf_region_z_threads(r)) return;
    const int z = (int)(t % (size_t)r.nz);
    const size_t col = t / (size_t)r.nz;
    const int xi = (int)(col / r.n[1]), y = r.lo[1] + (int)(col % r.n[1]);
    const size_t row = (size_t)(r.lo[0] + xi) * r.ny + y;
    const uint32_t* sp = site_plane + row * r.nzw;
    const uint32_t* up = unk_plane ? unk_plane + row * r.nzw : nullptr;
    const int32_t v = esdf_z_value([sp, up](int w) { return up ? (sp[w] | up[w]) : sp[w]; }, r.nz, r.nzw, z, r.E);
    int32_t* at = a + row * r.nz + z;
    if (*at != v) {
        *at = v;
        fy[(size_t)xi * r.nz + z] = 1;
    }
}

// y pass, thread t: element y of line (x, ., z) of the box' slab, if the z pass flagged the line
VIGO_HD void esdf_region_y(const EsdfRegion& r, size_t t, const int32_t* a, int32_t* b, const uint8_t* fy, uint8_t* fx) {
    if (t >= esdf_region_y_threads(r)) return;
    const int z = (int)(t % (size_t)r.nz);
    const size_t q = t / (size_t)r.nz;
    const int y = (int)(q % r.ny), xi = (int)(q / r.ny);
    if (!fy[(size_t)xi * r.nz + z]) return;
    const size_t nz = (size_t)r.nz, first = (size_t)(r.lo[0] + xi) * r.ny * nz + z;
    const int32_t* line = a + first;
    const int32_t v = esdf_line_value([line, nz](int j) { return line[(size_t)j * nz]; }, r.ny, y);
    int32_t* at = b + first + (size_t)y * nz;
    if (*at != v) {
        *at = v;
        fx[(size_t)y * nz + z] = 1;
    }
}

// x pass, thread t = voxel t of the lattice: element x of line (., y, z), if the y pass flagged the line
VIGO_HD void esdf_region_x(const EsdfRegion& r, size_t t, const int32_t* b, float* lattice, const uint8_t* fx, double res) {
    if (t >= esdf_region_x_threads(r)) return;
    const size_t sx = (size_t)r.ny * r.nz, q = t % sx;
    if (!fx[q]) return;
    const int32_t* line = b + q;
    lattice[t] = esdf_compose(esdf_line_value([line, sx](int j) { return line[(size_t)j * sx]; }, r.nx, (int)(t / sx)), res);
}

// re-tile, thread i = float i of the bricked field (EsdfView, vigo_internal.hpp: line (x, by, bz) of nby x nbz lines per x
// holds [x, x + 1] x [3 by, 3 by + 3] x [3 bz, 3 bz + 3], z fastest): rewritten if its source lies on a flagged x line
VIGO_HD void esdf_region_brick(const EsdfRegion& r, size_t i, int nby, int nbz, const uint8_t* fx, const float* lattice, float* bricked) {
    if (i >= (size_t)(r.nx - 1) * nby * nbz * 32) return;
    const size_t line = i >> 5;
    const int k = (int)(i & 31);
    const int bz = (int)(line % nbz), by = (int)((line / nbz) % nby);
    const int x = (int)(line / ((size_t)nbz * nby)) + (k >> 4), y = by * 3 + ((k >> 2) & 3), z = bz * 3 + (k & 3);
    if (x < r.nx && y < r.ny && z < r.nz && fx[(size_t)y * r.nz + z]) bricked[i] = lattice[((size_t)x * r.ny + y) * r.nz + z];
}

// the byte grid's plane bit — OR the unknown bit — packed like the snapshot (bit k of word w = voxel z = 32 w + k)
inline void esdf_pack_sites(const uint8_t* vox, size_t rows, int nz, int nzw, unsigned pick, uint32_t* words) {
    for (size_t row = 0; row < rows; ++row)
        for (int z = 0; z < nz; ++z)
            if (vox[row * nz + z] & pick) words[row * nzw + (z >> 5)] |= 1u << (z & 31);
}

// the three passes in plain loops on a checked lattice; a, b: nx * ny * nz each.  0, or -6 when the packed words cannot
// be allocated
inline int esdf_passes(int nx, int ny, int nz, const uint8_t* vox, int plane, int unknown_is_site, double res, int32_t E,
                       int32_t* a, int32_t* b, float* out) {
    const int nzw = (nz + 31) / 32;
    const size_t rows = (size_t)nx * ny;
    const unsigned pick = (1u << plane) | (unknown_is_site ? 2u : 0u);
    std::vector<uint32_t> words;
    try {
        words.assign(rows * nzw, 0u);
    } catch (const std::bad_alloc&) {
        return -6;
    }
    esdf_pack_sites(vox, rows, nz, nzw, pick, words.data());
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

// what the host twins refuse before they look at the lattice's size
inline bool esdf_host_args_ok(int nx, int ny, int nz, int plane, double res) {
    return (plane == 0 || plane == 2) && nx >= 2 && ny >= 2 && nz >= 2 && res > 0.0 && res < INFINITY;
}

// The host twin (vigo_esdf_from_voxels_host): the three passes above in plain loops.  0, or -1 for a bad argument, -6 for
// a lattice beyond kEsdfMaxEmptyD2 or kEsdfMaxVoxels, or one whose working memory (8 bytes per voxel and the packed
// words) the host cannot allocate (VIGO_ERR_INVALID_ARG / VIGO_ERR_UNSUPPORTED); nothing is written then, and no
// exception leaves the function: its caller is extern "C".
inline int esdf_from_voxels(int nx, int ny, int nz, const uint8_t* vox, int plane, int unknown_is_site, double res, float* out) {
    if (!vox || !out || !esdf_host_args_ok(nx, ny, nz, plane, res)) return -1;
    const int32_t E = esdf_empty_d2(nx, ny, nz);
    if (E == 0) return -6;
    std::vector<int32_t> a, b;
    try {
        a.resize((size_t)nx * ny * nz);
        b.resize(a.size());
    } catch (const std::bad_alloc&) {
        return -6;
    }
    return esdf_passes(nx, ny, nz, vox, plane, unknown_is_site, res, E, a.data(), b.data(), out);
}

// vigo_esdf_from_voxels_host_tracked: the same, and the caller keeps A and B (what esdf_update works on)
inline int esdf_from_voxels_tracked(int nx, int ny, int nz, const uint8_t* vox, int plane, int unknown_is_site, double res,
                                    int32_t* a, int32_t* b, float* out) {
    if (!vox || !a || !b || !out || !esdf_host_args_ok(nx, ny, nz, plane, res)) return -1;
    const int32_t E = esdf_empty_d2(nx, ny, nz);
    return E == 0 ? -6 : esdf_passes(nx, ny, nz, vox, plane, unknown_is_site, res, E, a, b, out);
}

// vigo_esdf_update_host: A, B and the lattice of the grid before the box [lo, lo + n) changed become those of `vox`, the
// whole grid after it, by the region functions in plain loops; *y_lines, *x_lines: the flagged lines.  An n of 0 changes
// nothing.  -1 also for a box that is negative or leaves the lattice.
inline int esdf_update(int nx, int ny, int nz, const uint8_t* vox, int plane, int unknown_is_site, double res, const int32_t lo[3],
                       const int32_t n[3], int32_t* a, int32_t* b, float* lattice, int64_t* y_lines, int64_t* x_lines) {
    if (!vox || !lo || !n || !a || !b || !lattice || !esdf_host_args_ok(nx, ny, nz, plane, res)) return -1;
    const int dims[3] = {nx, ny, nz};
    for (int k = 0; k < 3; ++k)
        if (lo[k] < 0 || n[k] < 0 || (int64_t)lo[k] + n[k] > dims[k]) return -1;
    if (esdf_empty_d2(nx, ny, nz) == 0) return -6;
    *y_lines = *x_lines = 0;
    if (n[0] == 0 || n[1] == 0 || n[2] == 0) return 0;
    const EsdfRegion r = esdf_region(nx, ny, nz, lo, n);
    std::vector<uint32_t> words;
    std::vector<uint8_t> fy, fx;
    try {
        words.assign((size_t)nx * ny * r.nzw, 0u);
        fy.assign((size_t)n[0] * nz, 0);
        fx.assign((size_t)ny * nz, 0);
    } catch (const std::bad_alloc&) {
        return -6;
    }
    esdf_pack_sites(vox, (size_t)nx * ny, nz, r.nzw, (1u << plane) | (unknown_is_site ? 2u : 0u), words.data());
    for (size_t t = 0; t < esdf_region_z_threads(r); ++t) esdf_region_z(r, t, words.data(), nullptr, a, fy.data());
    for (size_t t = 0; t < esdf_region_y_threads(r); ++t) esdf_region_y(r, t, a, b, fy.data(), fx.data());
    for (size_t t = 0; t < esdf_region_x_threads(r); ++t) esdf_region_x(r, t, b, lattice, fx.data(), res);
    for (uint8_t f : fy) *y_lines += f;
    for (uint8_t f : fx) *x_lines += f;
    return 0;
}

}  // namespace vigo
