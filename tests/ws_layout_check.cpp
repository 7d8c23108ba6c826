// ws_layout_check.cpp — every workspace layout of csrc/vigo_ws_layout.hpp on host memory (tests/test_ws_layout.py builds
// this with the address and undefined-behaviour sanitizers and runs it).  Per layout and argument set: size it on a null
// base, malloc exactly that, carve, write every array over the extent the kernels index (vigo_internal.hpp gives it next
// to each member), and check 8-byte alignment, pairwise disjointness and the byte count against the closed form the
// C-ABI layer used before the layouts existed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vigo_ws_layout.hpp"

namespace {

// stand-ins with the members the layouts fill (the real structs need the HIP runtime's header)
struct Args {
    long long* result;
    int32_t *in_off, *n_in, *pre, *tstatus, *n_out, *oseg_off, *opt_off, *tcounts;
    const uint8_t *pt, *ln;
    double* out_path;
    int32_t *out_seg, *out_path_off;
};
struct Work {
    int32_t *seg, *mseg, *pick, *retry_of, *status1, *len1, *status2, *len2;
    double *start1, *end1, *start2, *end2, *path1, *path2;
};
struct Reguide {
    long long* result;
    int32_t *kind, *n_list, *list, *n_new, *new_seg, *outcome;
};

struct Span { const void* p; size_t bytes; size_t align; };
long g_layouts = 0;

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #c, what); exit(1); } } while (0)

template <class T>
Span span(const T* p, size_t count, size_t align = 8) { return Span{p, count * sizeof(T), align}; }

void check(const char* what, void* base, size_t total, size_t parent_bytes, const std::vector<Span>& spans) {
    REQUIRE(total <= parent_bytes);
    const char* lo = static_cast<const char*>(base);
    for (size_t i = 0; i < spans.size(); ++i) {
        const char* p = static_cast<const char*>(spans[i].p);
        REQUIRE(p != nullptr);
        REQUIRE((reinterpret_cast<uintptr_t>(p) & (spans[i].align - 1)) == 0);
        REQUIRE(p >= lo && p + spans[i].bytes <= lo + total);
        memset(const_cast<char*>(p), 0xA5, spans[i].bytes);             // past the allocation: the sanitizer stops here
        for (size_t j = 0; j < i; ++j) {
            const char* q = static_cast<const char*>(spans[j].p);
            REQUIRE(p + spans[i].bytes <= q || q + spans[j].bytes <= p);
        }
    }
    ++g_layouts;
}

size_t even(size_t n) { return (n + 1) & ~(size_t)1; }   // (B + 2) & ~1 of the earlier code is even(B + 1)

void path_search_scratch(size_t B, size_t N, bool flags) {
    Args a{};
    const size_t total = vigo::ws_path_search_scratch(nullptr, B, N, flags, a);
    void* base = malloc(total);
    const char* what = "ws_path_search_scratch";
    REQUIRE(vigo::ws_path_search_scratch(base, B, N, flags, a) == total);
    std::vector<Span> s = {span(a.result, 8), span(a.in_off, B + 1), span(a.n_in, B), span(a.pre, B), span(a.tstatus, B), span(a.n_out, B),
                           span(a.oseg_off, B), span(a.opt_off, B), span(a.tcounts, 2 * B)};
    if (flags) { s.push_back(span(a.pt, B * N)); s.push_back(span(a.ln, B * N)); }
    else REQUIRE(!a.pt && !a.ln);
    const size_t words = (B + 2) & ~(size_t)1, flag_bytes = flags ? ((B * N + 7) & ~(size_t)7) : 0;
    check(what, base, total, 64 + 9 * words * 4 + 2 * flag_bytes, s);
    free(base);
}

void reguide(size_t B, size_t N) {
    const size_t kSegs = 48;                                              // VIGO_MAX_COLLISION_SEGS
    Reguide r{};
    vigo::ReguideStage st{};
    const size_t total = vigo::ws_reguide(nullptr, B, N, kSegs, r, st);
    void* base = malloc(total);
    const char* what = "ws_reguide";
    REQUIRE(vigo::ws_reguide(base, B, N, kSegs, r, st) == total);
    const size_t words = (B + 2) & ~(size_t)1, gwords = (B * N + 2) & ~(size_t)1;
    check(what, base, total, 64 + 4 * (9 * words + 4 * kSegs * B + gwords),
          {span(r.result, 8), span(r.kind, B), span(r.n_list, B), span(r.n_new, B), span(r.outcome, B), span(st.ps_status, B), span(st.ps_seg_off, B + 1),
           span(st.g_status, B), span(st.ps_counts, 2 * B), span(r.list, 2 * kSegs * B), span(r.new_seg, 2 * kSegs * B), span(st.g_off, B * N + 1)});
    free(base);
}

void searches(size_t S, size_t Q2, size_t cap) {
    Work w{};
    const char* what = "ws_first_searches";
    size_t total = vigo::ws_first_searches(nullptr, S, cap, w);
    void* base = malloc(total);
    REQUIRE(vigo::ws_first_searches(base, S, cap, w) == total);
    check(what, base, total, even(S) * 8 * 4 + S * 12 * 8 + S * cap * 3 * 8,
          {span(w.start1, 3 * S), span(w.end1, 3 * S), span(w.start2, 3 * S), span(w.end2, 3 * S), span(w.path1, S * cap * 3), span(w.seg, 2 * S),
           span(w.mseg, 2 * S), span(w.pick, S), span(w.retry_of, S), span(w.status1, S), span(w.len1, S)});
    free(base);
    what = "ws_second_searches";
    total = vigo::ws_second_searches(nullptr, Q2, cap, w);
    base = malloc(total);
    REQUIRE(vigo::ws_second_searches(base, Q2, cap, w) == total);
    check(what, base, total, Q2 * cap * 3 * 8 + even(Q2) * 2 * 4, {span(w.path2, Q2 * cap * 3), span(w.status2, Q2), span(w.len2, Q2)});
    free(base);
}

void reguide_paths(size_t total_seg, size_t total_pts) {
    Args a{};
    const char* what = "ws_reguide_paths";
    const size_t total = vigo::ws_reguide_paths(nullptr, total_seg, total_pts, a);
    void* base = malloc(total);
    REQUIRE(vigo::ws_reguide_paths(base, total_seg, total_pts, a) == total);
    const size_t seg_words = (2 * total_seg + 2) & ~(size_t)1, po_words = (total_seg + 2) & ~(size_t)1;
    check(what, base, total, 3 * total_pts * 8 + 8 + 4 * (seg_words + po_words),
          {span(a.out_path, 3 * total_pts), span(a.out_seg, 2 * total_seg), span(a.out_path_off, total_seg + 1)});
    free(base);
}

void reguide_pairs(size_t P) {
    double* pv;
    uint8_t* unk;
    const char* what = "ws_reguide_pairs";
    const size_t total = vigo::ws_reguide_pairs(nullptr, P, pv, unk);
    void* base = malloc(total);
    REQUIRE(vigo::ws_reguide_pairs(base, P, pv, unk) == total);
    check(what, base, total, P * 48 + P + 8, {span(pv, 6 * P), span(unk, P)});
    free(base);
}

void rebound(size_t B) {
    int32_t *flags, *idx;
    const char* what = "ws_rebound";
    const size_t total = vigo::ws_rebound(nullptr, B, flags, idx);
    void* base = malloc(total);
    REQUIRE(vigo::ws_rebound(base, B, flags, idx) == total);
    check(what, base, total, (B + 16) * sizeof(int32_t) + 64, {span(flags, 16), span(idx, B)});
    free(base);
}

void corridor(size_t S, size_t clock_bytes) {
    int* todo;
    void* clock_ws;
    const char* what = "ws_corridor";
    const size_t total = vigo::ws_corridor(nullptr, S, clock_bytes, todo, clock_ws);
    void* base = malloc(total);
    REQUIRE(vigo::ws_corridor(base, S, clock_bytes, todo, clock_ws) == total);
    std::vector<Span> s = {span(todo, S)};
    if (clock_bytes) s.push_back(span(static_cast<char*>(clock_ws), clock_bytes));
    else REQUIRE(!clock_ws);
    check(what, base, total, ((S * sizeof(int) + 255) & ~(size_t)255) + clock_bytes, s);
    free(base);
}

// the two back-to-back arrays carry no padding (the ESDF build's pair is 1 GiB at 512^3 and sized exactly): the second
// one is 4-byte aligned, as it always was
void pair(size_t n) {
    uint32_t *a, *b;
    const char* what = "ws_pair";
    const size_t total = vigo::ws_pair(nullptr, n, a, b);
    void* base = malloc(total);
    REQUIRE(vigo::ws_pair(base, n, a, b) == total);
    check(what, base, total, 2 * n * sizeof(uint32_t), {span(a, n), span(b, n, 4)});
    free(base);
}

}  // namespace

int main() {
    const size_t Bs[] = {1, 2, 3, 7, 32, 33}, Ns[] = {7, 8, 33}, Ss[] = {0, 1, 2, 5, 17}, caps[] = {2, 3, 64}, totals[] = {0, 1, 5, 18}, Ps[] = {0, 1, 7};
    for (size_t B : Bs) {
        for (size_t N : Ns) {
            path_search_scratch(B, N, true);
            path_search_scratch(B, N, false);
            reguide(B, N);
        }
        rebound(B);
    }
    for (size_t S : Ss)
        for (size_t cap : caps)
            for (size_t Q2 : {(size_t)0, (size_t)1, S})
                if (Q2 <= S) searches(S, Q2, cap);
    for (size_t total_seg : totals)
        for (size_t total_pts : totals) reguide_paths(total_seg, total_pts);
    for (size_t P : Ps) reguide_pairs(P);
    for (size_t S : {(size_t)1, (size_t)5, (size_t)64, (size_t)65}) {
        corridor(S, S * 2568);                                            // a clock table per segment
        corridor(S, 0);
    }
    for (size_t n : {(size_t)1, (size_t)9, (size_t)18, (size_t)8 * 8 * 40}) pair(n);
    printf("ws_layout_check: %ld layouts carved and written\n", g_layouts);
    return 0;
}
