// seed_block_check.cpp — the two blocks of bsplineTraj::seedOnDevice (host/src/seedBlock.h) on host memory
// (tests/test_seed_block.py builds this with the address and undefined-behaviour sanitizers and runs it).  Per shape
// (T, S, deg, cap): size each block on a null base, allocate exactly that, carve a host view and a device view on the
// same base, and check that every field starts at a multiple of its element size, that the fields are disjoint, in order
// and tile the block (the only padding is the one before a field of wider elements and the block's tail up to a whole
// 8-byte word), that the extents are the ones include/vigo.h gives vigo_seed_paths' arguments, and that a distinct pattern
// written through the host view reads back unchanged through the device view.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "seedBlock.h"

namespace {

struct Field { const char* name; void* host; void* dev; size_t count, elem; };
long g_blocks = 0;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (%s, field %s, T %zu S %zu deg %zu cap %zu)\n", __FILE__, __LINE__, #c, what, fname, gT, gS, gDeg, gCap); exit(1); } } while (0)
size_t gT, gS, gDeg, gCap;

template <class T>
Field field(const char* name, T* host, T* dev, size_t count) { return Field{name, host, dev, count, sizeof(T)}; }

// closedBytes: the size the facade computed by hand before the layout existed
void check(const char* what, char* base, size_t total, size_t closedBytes, const std::vector<Field>& fields) {
    const char* fname = "-";
    REQUIRE(total == closedBytes && total % 8 == 0);
    size_t end = 0;                                            // of the previous field, from the base
    unsigned char tag = 1;
    for (const Field& f : fields) {
        fname = f.name;
        REQUIRE(f.host != nullptr && f.host == f.dev);         // two carvings of one base agree
        const size_t off = (size_t)(static_cast<char*>(f.host) - base);
        REQUIRE(off % f.elem == 0);
        REQUIRE(off == ((end + f.elem - 1) & ~(f.elem - 1)));  // in order, disjoint, no hole but the alignment's
        end = off + f.count * f.elem;
        REQUIRE(end <= total);
        memset(f.host, tag++, f.count * f.elem);               // past the allocation: the sanitizer stops here
    }
    fname = "tail";
    REQUIRE(total == ((end + 7) & ~(size_t)7));
    tag = 1;
    for (const Field& f : fields) {                            // the pattern of each field through the other view
        fname = f.name;
        const unsigned char* q = static_cast<const unsigned char*>(f.dev);
        for (size_t i = 0; i < f.count * f.elem; ++i) REQUIRE(q[i] == tag);
        ++tag;
    }
    ++g_blocks;
}

void shape(size_t T, size_t S, size_t deg, size_t cap) {
    gT = T; gS = S; gDeg = deg; gCap = cap;
    const char* what = "seedInBlock";
    const char* fname = "-";
    {
        vigo_host::SeedIn h{}, d{};
        const size_t total = vigo_host::seedInBlock(nullptr, T, S, deg, h);
        REQUIRE(!h.duration && !h.segOff);
        char* base = static_cast<char*>(malloc(total));
        REQUIRE(vigo_host::seedInBlock(base, T, S, deg, h) == total && vigo_host::seedInBlock(base, T, S, deg, d) == total);
        // vigo.h: duration .. prev_in_fit double[T]; knots "as vigo_traj_point_check" double[S + T]; coeffs [S][3][deg + 1];
        // seg_off int32[T + 1]
        check(what, base, total, (6 * T + S + T + S * 3 * (deg + 1)) * 8 + ((T + 2) / 2) * 8,
              {field("duration", h.duration, d.duration, T), field("dt0", h.dt0, d.dt0, T),
               field("control_point_distance", h.controlPointDistance, d.controlPointDistance, T),
               field("max_path_length", h.maxPathLength, d.maxPathLength, T), field("prev_in_seed", h.prevSeed, d.prevSeed, T),
               field("prev_in_fit", h.prevFit, d.prevFit, T), field("knots", h.knots, d.knots, S + T),
               field("coeffs", h.coeffs, d.coeffs, S * 3 * (deg + 1)), field("seg_off", h.segOff, d.segOff, T + 1)});
        free(base);
    }
    what = "seedOutBlock";
    {
        vigo_host::SeedOut h{}, d{};
        const size_t total = vigo_host::seedOutBlock(nullptr, T, cap, h);
        REQUIRE(!h.status && !h.fit);
        char* base = static_cast<char*>(malloc(total));
        REQUIRE(vigo_host::seedOutBlock(base, T, cap, h) == total && vigo_host::seedOutBlock(base, T, cap, d) == total);
        // vigo.h: out_status, out_tries, out_seed_n, out_fit_n int32[T]; out_dt, out_final_time, out_prev_seed, out_prev_fit
        // double[T]; out_seed, out_fit [T][point_cap][3]
        check(what, base, total, 16 * T + 32 * T + 2 * T * cap * 24,
              {field("out_status", h.status, d.status, T), field("out_tries", h.tries, d.tries, T), field("out_seed_n", h.seedN, d.seedN, T),
               field("out_fit_n", h.fitN, d.fitN, T), field("out_dt", h.dt, d.dt, T), field("out_final_time", h.finalTime, d.finalTime, T),
               field("out_prev_seed", h.prevSeed, d.prevSeed, T), field("out_prev_fit", h.prevFit, d.prevFit, T),
               field("out_seed", h.seed, d.seed, T * cap * 3), field("out_fit", h.fit, d.fit, T * cap * 3)});
        free(base);
    }
}

}  // namespace

int main() {
    // T = 1 against 2: the int32 tail seg_off [T + 1] ends on a whole word or leaves half of one
    for (size_t T : {(size_t)1, (size_t)2, (size_t)3})
        for (size_t S : {(size_t)0, (size_t)1, (size_t)5})
            for (size_t deg : {(size_t)0, (size_t)7, (size_t)15})
                for (size_t cap : {(size_t)0, (size_t)1, (size_t)128}) shape(T, S, deg, cap);
    printf("seed_block_check: %ld blocks carved, written and read back\n", g_blocks);
    return 0;
}
