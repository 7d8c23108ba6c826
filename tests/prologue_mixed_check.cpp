// prologue_mixed_check.cpp — the index arithmetic of the mixed prologue entries (csrc/vigo_rows_core.hpp: row_count,
// row_offsets, row_slot_owner) as k_guide_offsets, k_guide_merge_offsets and k_guide_merge use it, walked on the host over
// rows like the crafted ones of tests/prologue_mixed_cases.py: counts 7 .. 120 interleaved in rows of 120, an odd batch,
// bad counts in the middle.  Every array is a heap block of its exact size (the address sanitizer sees one element past
// it) between guard words that are checked at the end.  A program of its own: tests/test_prologue_mixed_core.py builds it
// with -fsanitize=address,undefined and runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vigo_guide_core.hpp"
#include "vigo_rows_core.hpp"

namespace {

constexpr int32_t kGuard = 0x5AFE5AFE;
constexpr int kGuardWords = 16;

// n int32 between two runs of guard words
struct Guarded {
    int32_t* block;
    int32_t* p;
    size_t n;
    explicit Guarded(size_t n_, int32_t fill) : n(n_) {
        block = (int32_t*)malloc((n + 2 * kGuardWords) * sizeof(int32_t));
        for (int i = 0; i < kGuardWords; ++i) block[i] = block[kGuardWords + n + i] = kGuard;
        p = block + kGuardWords;
        for (size_t i = 0; i < n; ++i) p[i] = fill;
    }
    bool intact() const {
        for (int i = 0; i < kGuardWords; ++i)
            if (block[i] != kGuard || block[kGuardWords + n + i] != kGuard) return false;
        return true;
    }
    ~Guarded() { free(block); }
};

int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED line %d: %s\n", __LINE__, #cond);               \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Seg {
    int first, second;
};

// the segments of a row of n control points: an interior run, a segment without interior points near the start (its
// pushes are clipped to [3, n - 4]), the (start, n - 1) segment and its duplicate
std::vector<Seg> segments_of(int n, int variant) {
    std::vector<Seg> s;
    if (variant % 3 == 0) return s;
    if (n >= 12) s.push_back({n / 3, n / 3 + 4});
    s.push_back({2, 3});
    if (variant % 3 == 2) {
        s.push_back({n - 4, n - 1});
        s.push_back({n - 4, n - 3});
    }
    return s;
}

void walk(int Ns, const std::vector<int>& counts) {
    const int B = (int)counts.size();
    Guarded n_pts((size_t)B, 0), off((size_t)B * Ns + 1, -7), status((size_t)B, -7);
    for (int b = 0; b < B; ++b) n_pts.p[b] = counts[b];
    // k_guide_offsets, pass 2: the offsets of every row, a bad count deferred
    long long at = 0, want_total = 0;
    for (int b = 0; b < B; ++b) {
        const int N = vigo::row_count(n_pts.p, b, Ns);
        CHECK(N == -1 || (N >= 7 && N <= Ns && N == counts[b]));
        const bool deferred = N < 0;
        status.p[b] = deferred ? 1 : 0;
        const std::vector<Seg> segs = deferred ? std::vector<Seg>() : segments_of(N, b);
        for (const Seg& s : segs) {
            CHECK(vigo::guide_segment_ok(N, s.first, s.second, 2));
            want_total += vigo::guide_pushes_total(N, s.first, s.second);
        }
        at = vigo::row_offsets(Ns, deferred ? 0 : N, at, off.p + (size_t)b * Ns, [&](int i) {
            int k = 0;
            for (const Seg& s : segs) k += vigo::guide_pushes(N, s.first, s.second, i);
            return k;
        });
    }
    off.p[(size_t)B * Ns] = (int32_t)at;
    CHECK(at == want_total);
    // a valid CSR over all B * Ns + 1 entries; the padding and the bad counts own empty ranges
    CHECK(off.p[0] == 0);
    for (size_t q = 0; q < (size_t)B * Ns; ++q) CHECK(off.p[q + 1] >= off.p[q]);
    for (int b = 0; b < B; ++b) {
        const int N = vigo::row_count(n_pts.p, b, Ns);
        for (int i = N < 0 ? 0 : N; i < Ns; ++i) CHECK(off.p[(size_t)b * Ns + i + 1] == off.p[(size_t)b * Ns + i]);
    }
    // k_guide_merge: the owner of every slot, searched over the row
    Guarded seen((size_t)(at > 0 ? at : 1), 0);
    for (int b = 0; b < B; ++b) {
        const int32_t* row = off.p + (size_t)b * Ns;
        const int N = vigo::row_count(n_pts.p, b, Ns);
        for (int q = row[0]; q < row[Ns]; ++q) {
            const int i = vigo::row_slot_owner(row, Ns, q);
            CHECK(i >= 0 && i < Ns && N > 0 && i < N);
            CHECK(row[i] <= q && q < row[i + 1]);
            seen.p[q] += 1;
        }
    }
    for (long long q = 0; q < at; ++q) CHECK(seen.p[q] == 1);
    // k_guide_merge_offsets: old pairs on EVERY control point of every row (copied whatever the count) plus the new ones
    Guarded merged((size_t)B * Ns + 1, -7);
    long long m_at = 0, m_want = 0;
    for (int b = 0; b < B; ++b)
        m_at = vigo::row_offsets(Ns, Ns, m_at, merged.p + (size_t)b * Ns, [&](int i) {
            const size_t q = (size_t)b * Ns + i;
            const int k = (i % 5 == 0 ? 1 : 0) + (off.p[q + 1] - off.p[q]);
            m_want += k;
            return k;
        });
    merged.p[(size_t)B * Ns] = (int32_t)m_at;
    CHECK(m_at == m_want);
    for (int b = 0; b < B; ++b) {
        const int32_t* row = merged.p + (size_t)b * Ns;
        for (int q = row[0]; q < row[Ns]; ++q) {
            const int i = vigo::row_slot_owner(row, Ns, q);
            CHECK(i >= 0 && i < Ns && row[i] <= q && q < row[i + 1]);
        }
    }
    CHECK(n_pts.intact() && off.intact() && status.intact() && seen.intact() && merged.intact());
}

}  // namespace

int main() {
    // no counts: the uniform entries
    CHECK(vigo::row_count(nullptr, 5, 32) == 32);
    const int good[] = {7, 8, 12, 31, 32, 33, 40, 64, 65, 120};
    std::vector<int> counts;
    for (int r = 0; r < 5; ++r)
        for (int n : good) counts.push_back(n);
    counts.push_back(7);                                   // an odd batch
    walk(120, counts);
    // bad counts in the middle of a good batch: 6, 0, -1, Ns + 1, INT32_MAX
    const int bad[] = {6, 0, -1, 121, 2147483647};
    for (int k = 0; k < 5; ++k) counts[10 + 7 * k] = bad[k];
    walk(120, counts);
    // a single row of its own count, the smallest and the largest stride
    walk(7, {7});
    walk(120, {120});
    walk(33, {33, 7, 33});
    if (failures) return 1;
    printf("rows ok\n");
    return 0;
}
