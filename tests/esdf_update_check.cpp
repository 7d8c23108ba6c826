// esdf_update_check.cpp — the kernels of vigo_update_esdf (csrc/vigo_esdf_build.hip) on a machine without a GPU: every
// launch is walked thread index by thread index through the region functions the kernels call (csrc/vigo_esdf_core.hpp),
// over the launches' own grids — esdf_region_grid() blocks of kEsdfRegionBlock, the surplus indices of the last block
// included — on a packed snapshot, with the tracking workspace carved by ws_esdf_track into a heap block of exactly its
// size and the bricked field in one of exactly its size.  tests/test_esdf_update_core.py builds this with the address
// and undefined-behaviour sanitizers, so an index beyond the box, a line, a flag array or the field is a failure.
//
// After every refresh the walked A, B, lattice and line counts are compared with the loops (esdf_update on a copy) and
// with a whole rebuild (esdf_from_voxels_tracked) of the new grid, the bricked field with a whole re-tiling of the rebuilt
// lattice; a difference ends the program with a message and status 2.
//
// stdin, binary: int32 nx ny nz plane unknown_is_site R, double res, the start grid's nx * ny * nz bytes, then R refreshes
//   int32 lo[3] n[3], the whole new grid's bytes
// stdout, binary, per refresh: int64 y_lines x_lines, then A, B (int32) and the lattice (float) of nx * ny * nz each.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vigo_esdf_core.hpp"
#include "vigo_ws_layout.hpp"

static bool get(void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, stdin) == bytes; }
static int bad(const char* what, int refresh) {
    fprintf(stderr, "esdf_update_check: refresh %d: %s\n", refresh, what);
    return 2;
}

// the snapshot's three bit planes of a byte grid (include/vigo.h: bit p of a byte -> plane p)
static std::vector<uint32_t> pack(const std::vector<uint8_t>& vox, size_t rows, int nz, int nzw) {
    std::vector<uint32_t> planes(3 * rows * nzw, 0u);
    for (int p = 0; p < 3; ++p)
        for (size_t row = 0; row < rows; ++row)
            for (int z = 0; z < nz; ++z)
                if ((vox[row * nz + z] >> p) & 1u) planes[(p * rows + row) * nzw + (z >> 5)] |= 1u << (z & 31);
    return planes;
}

// k_esdf_brick's rule, restated: float i of line (x, by, bz)
static void brick(int nx, int ny, int nz, const float* src, std::vector<float>& dst) {
    const int nby = (ny + 1) / 3, nbz = (nz + 1) / 3;
    for (size_t i = 0; i < dst.size(); ++i) {
        const size_t line = i >> 5;
        const int k = (int)(i & 31);
        const int x = (int)(line / ((size_t)nby * nbz)) + (k >> 4), y = (int)((line / nbz) % nby) * 3 + ((k >> 2) & 3), z = (int)(line % nbz) * 3 + (k & 3);
        dst[i] = (x < nx && y < ny && z < nz) ? src[((size_t)x * ny + y) * nz + z] : 0.0f;
    }
}

int main() {
    int32_t head[6];
    double res;
    if (!get(head, sizeof head) || !get(&res, sizeof res)) return 1;
    const int nx = head[0], ny = head[1], nz = head[2], plane = head[3], unk = head[4], R = head[5];
    const int nzw = (nz + 31) / 32, nby = (ny + 1) / 3, nbz = (nz + 1) / 3;
    const size_t rows = (size_t)nx * ny, voxels = rows * nz, pw = rows * nzw;
    std::vector<uint8_t> vox(voxels);
    if (!get(vox.data(), voxels)) return 1;

    vigo::EsdfTrackWs w{};
    const size_t need = vigo::ws_esdf_track(nullptr, voxels, (size_t)nx * nz, (size_t)ny * nz, w);
    char* block = static_cast<char*>(aligned_alloc(256, (need + 255) / 256 * 256 + 256));   // 256: hipMalloc's alignment
    // the block ends where the layout ends: shift the base so that ASan's red zone starts right behind it
    char* base = block + ((need + 255) / 256 * 256 + 256 - need) / 16 * 16;
    vigo::ws_esdf_track(base, voxels, (size_t)nx * nz, (size_t)ny * nz, w);
    if (vigo::esdf_from_voxels_tracked(nx, ny, nz, vox.data(), plane, unk, res, w.a, w.b, w.lattice) != 0) return 1;
    std::vector<float> field((size_t)(nx - 1) * nby * nbz * 32), field_want(field.size());
    brick(nx, ny, nz, w.lattice, field);
    std::vector<int32_t> a2(w.a, w.a + voxels), b2(w.b, w.b + voxels), a3(voxels), b3(voxels);
    std::vector<float> l2(w.lattice, w.lattice + voxels), l3(voxels);

    for (int k = 0; k < R; ++k) {
        int32_t box[6];
        if (!get(box, sizeof box) || !get(vox.data(), voxels)) return 1;
        const int32_t *lo = box, *n = box + 3;
        int64_t y_lines = 0, x_lines = 0, y2 = 0, x2 = 0;
        if (n[0] != 0 && n[1] != 0 && n[2] != 0) {
            const std::vector<uint32_t> planes = pack(vox, rows, nz, nzw);
            const uint32_t* sites = planes.data() + (size_t)plane * pw;
            const uint32_t* unknown = unk ? planes.data() + pw : nullptr;
            const vigo::EsdfRegion r = vigo::esdf_region(nx, ny, nz, lo, n);
            const auto launch = [](size_t threads) { return vigo::esdf_region_grid(threads) * vigo::kEsdfRegionBlock; };
            memset(w.counters, 0, w.clear_bytes);
            for (size_t t = 0; t < launch(vigo::esdf_region_z_threads(r)); ++t) vigo::esdf_region_z(r, t, sites, unknown, w.a, w.fy);
            for (size_t t = 0; t < launch(vigo::esdf_region_y_threads(r)); ++t) vigo::esdf_region_y(r, t, w.a, w.b, w.fy, w.fx);
            for (size_t t = 0; t < launch(vigo::esdf_region_x_threads(r)); ++t) vigo::esdf_region_x(r, t, w.b, w.lattice, w.fx, res);
            for (size_t t = 0; t < launch(field.size()); ++t) vigo::esdf_region_brick(r, t, nby, nbz, w.fx, w.lattice, field.data());
            for (size_t t = 0; t < (size_t)n[0] * nz; ++t) y_lines += w.fy[t] != 0;
            for (size_t t = 0; t < (size_t)ny * nz; ++t) x_lines += w.fx[t] != 0;
            for (size_t t = 0; t < (size_t)(nx + ny) * nz; ++t)
                if (w.fy[t] > 1) return bad("a flag that is neither 0 nor 1", k);
        }
        if (vigo::esdf_update(nx, ny, nz, vox.data(), plane, unk, res, lo, n, a2.data(), b2.data(), l2.data(), &y2, &x2) != 0) return bad("esdf_update refused", k);
        if (vigo::esdf_from_voxels_tracked(nx, ny, nz, vox.data(), plane, unk, res, a3.data(), b3.data(), l3.data()) != 0) return bad("rebuild refused", k);
        brick(nx, ny, nz, l3.data(), field_want);
        if (y_lines != y2 || x_lines != x2) return bad("line counts differ from the loops'", k);
        if (memcmp(w.a, a2.data(), voxels * 4) || memcmp(w.b, b2.data(), voxels * 4) || memcmp(w.lattice, l2.data(), voxels * 4)) return bad("walk differs from the loops", k);
        if (memcmp(w.a, a3.data(), voxels * 4) || memcmp(w.b, b3.data(), voxels * 4) || memcmp(w.lattice, l3.data(), voxels * 4)) return bad("walk differs from a rebuild", k);
        if (memcmp(field.data(), field_want.data(), field.size() * 4)) return bad("bricked field differs from a whole re-tiling", k);
        fwrite(&y_lines, 8, 1, stdout);
        fwrite(&x_lines, 8, 1, stdout);
        fwrite(w.a, 4, voxels, stdout);
        fwrite(w.b, 4, voxels, stdout);
        fwrite(w.lattice, 4, voxels, stdout);
    }
    free(block);
    return 0;
}
