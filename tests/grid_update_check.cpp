// grid_update_check.cpp — the kernels of vigo_update_grid_region (csrc/vigo_grid_update.hip) on a machine without a GPU:
// every launch is walked thread index by thread index through the word functions the kernels call
// (csrc/vigo_grid_update_core.hpp, csrc/vigo_dilate_bits.hpp), on a packed snapshot, with the workspace carved by
// ws_grid_update into a heap block of exactly its size.  tests/test_grid_update_core.py builds this with the address and
// undefined-behaviour sanitizers, so an index beyond a box, a plane or a window is a failure, not a wrong word.
//
// stdin, binary, int32 unless said: nx ny nz U, the snapshot's 3 * nx * ny * nzw words, then U updates
//   lo[3] n[3] has_r r[3], n0 * n1 * n2 bytes
// stdout, binary: after every update one int32 (the RegionCheck) and the whole snapshot again.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vigo_dilate_bits.hpp"
#include "vigo_grid_update_core.hpp"
#include "vigo_ws_layout.hpp"

static bool get(void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, stdin) == bytes; }

int main() {
    int32_t head[4];
    if (!get(head, sizeof head)) return 1;
    const int nx = head[0], ny = head[1], nz = head[2], U = head[3];
    const int nzw = (nz + 31) / 32;
    const size_t pw = (size_t)nx * ny * nzw;
    std::vector<uint32_t> planes(3 * pw);
    if (!get(planes.data(), planes.size() * 4)) return 1;
    for (int u = 0; u < U; ++u) {
        int32_t a[10];
        if (!get(a, sizeof a)) return 1;
        const int32_t *lo = a, *n = a + 3, *r = a[6] ? a + 7 : nullptr;
        const bool sane = n[0] >= 0 && n[1] >= 0 && n[2] >= 0;
        std::vector<uint8_t> box(sane ? (size_t)n[0] * n[1] * n[2] : 0);
        if (!get(box.data(), box.size())) return 1;
        const int32_t rc = vigo::region_check(nx, ny, nz, lo, n, r);
        if (rc == vigo::kRegionOk) {
            const vigo::RegionPlan p = vigo::region_plan(nx, ny, nz, lo, n, r);
            uint8_t* staged;
            uint32_t *A, *B;
            const size_t need = vigo::ws_grid_update(nullptr, box.size(), vigo::region_window_words(p), staged, A, B);
            char* ws = static_cast<char*>(aligned_alloc(256, (need + 255) / 256 * 256 + 256));   // 256: hipMalloc's alignment
            // the block ends where the layout ends: shift the base so that ASan's red zone starts right behind it
            char* base = ws + ((need + 255) / 256 * 256 + 256 - need) / 16 * 16;
            vigo::ws_grid_update(base, box.size(), vigo::region_window_words(p), staged, A, B);
            for (size_t i = 0; i < box.size(); ++i) staged[i] = box[i];
            for (size_t t = 0; t < vigo::region_box_words(p); ++t) vigo::region_write_word(p, t, staged, planes.data(), pw);
            if (p.inflate) {
                const size_t nw = vigo::region_window_words(p);
                for (size_t t = 0; t < nw; ++t) vigo::region_gather_word(p, t, planes.data() + 2 * pw, A);
                for (size_t t = 0; t < nw; ++t) B[t] = vigo::dilate_bits_z_word(p.cnz, p.cw, p.r[2], A, t);
                for (size_t t = 0; t < nw; ++t) A[t] = vigo::dilate_bits_rows_word((size_t)p.cw, p.cy, p.r[1], B, t);
                for (size_t t = 0; t < nw; ++t) B[t] = vigo::dilate_bits_rows_word((size_t)p.cy * p.cw, p.cx, p.r[0], A, t);
                for (size_t t = 0; t < vigo::region_back_words(p); ++t) vigo::region_back_word(p, t, B, planes.data());
            }
            free(ws);
        }
        fwrite(&rc, 4, 1, stdout);
        fwrite(planes.data(), 4, planes.size(), stdout);
    }
    return 0;
}
