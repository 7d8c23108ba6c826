// vigo_ws_layout.hpp — how the C-ABI layer carves its device workspaces.  No HIP in here: tests/ws_layout_check.cpp runs
// every layout on host memory under the address sanitizer.
//
// A layout is ONE function, run twice: on a null base it only measures (its return value sizes the buffer), on the
// buffer it hands out the pointers — so the byte count and the pointers cannot disagree.  The argument structs are
// template parameters (PathSearchArgs, PathSearchWork, ReguideArgs of vigo_internal.hpp, whose comments give every
// array's extent); the order of the arrays and the 64-byte result header are part of what the kernels were measured with.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace vigo {

// a cursor over `base`: every array starts on an 8-byte boundary
class WsCarver {
public:
    explicit WsCarver(void* base) : base_(static_cast<char*>(base)) {}
    template <class T>
    T* take(size_t count) {
        off_ = (off_ + 7) & ~(size_t)7;
        T* p = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return off_; }

private:
    char* base_;
    size_t off_ = 0;
};

// n int32 as whole 8-byte words: the stride of the int32 arrays below
constexpr size_t ws_even(size_t n) { return (n + 1) & ~(size_t)1; }

// two arrays of n 32-bit words back to back (vigo_inflate_grid's two planes, the ESDF build's two buffers: at 512^3
// the latter is 1 GiB, so no padding — the second array is only 4-byte aligned when n is odd)
template <class T>
size_t ws_pair(void* base, size_t n, T*& first, T*& second) {
    WsCarver c(base);
    first = c.take<T>(2 * n);
    second = first ? first + n : nullptr;
    return c.bytes();
}

// vigo_build_esdf_tracked (Ws = EsdfTrackWs of vigo_esdf_core.hpp): the passes' results A, B and the float lattice of
// `voxels` each — no padding between them, as in ws_pair: 1.5 GiB at 512^3 — then the two line counts and the flag arrays
// of nx * nz and ny * nz bytes as ONE run, which vigo_update_esdf clears with one memset of clear_bytes
template <class Ws>
size_t ws_esdf_track(void* base, size_t voxels, size_t fy_bytes, size_t fx_bytes, Ws& w) {
    WsCarver c(base);
    w.a = c.take<int32_t>(3 * voxels);
    w.b = w.a ? w.a + voxels : nullptr;
    w.lattice = w.a ? reinterpret_cast<float*>(w.a + 2 * voxels) : nullptr;
    w.counters = c.take<unsigned long long>(2);
    w.fy = c.take<uint8_t>(fy_bytes + fx_bytes);
    w.fx = w.fy ? w.fy + fy_bytes : nullptr;
    w.clear_bytes = 2 * sizeof(unsigned long long) + fy_bytes + fx_bytes;
    return c.bytes();
}

// vigo_update_grid_region: the box' bytes as the *_host form stages them (none in the device-pointer form; whole 16-byte
// lines, so the buffer's alignment carries over to the planes and the box' rows keep k_pack_grid's aligned loads), then
// the two compact planes of window_words each that inflate mode dilates in (none in raw mode)
inline size_t ws_grid_update(void* base, size_t staged_bytes, size_t window_words, uint8_t*& staged, uint32_t*& planeA, uint32_t*& planeB) {
    WsCarver c(base);
    staged = staged_bytes ? c.take<uint8_t>((staged_bytes + 15) & ~(size_t)15) : nullptr;
    planeA = window_words ? c.take<uint32_t>(window_words) : nullptr;
    planeB = window_words ? c.take<uint32_t>(window_words) : nullptr;
    return c.bytes();
}

// vigo_corridor_check: the first pass' work list for the second (whole 256-byte lines), then the segments' clock tables
inline size_t ws_corridor(void* base, size_t S, size_t clock_bytes, int*& todo, void*& clock_ws) {
    WsCarver c(base);
    todo = c.take<int>((S + 63) & ~(size_t)63);
    clock_ws = clock_bytes ? c.take<char>(clock_bytes) : nullptr;
    return c.bytes();
}

// vigo_rebound_rounds: 16 flag words (flags[0] is the count of the compacted set), then its B indices
inline size_t ws_rebound(void* base, size_t B, int32_t*& flags, int32_t*& idx) {
    WsCarver c(base);
    flags = c.take<int32_t>(16);
    idx = c.take<int32_t>(B + 16);
    return c.bytes();
}

// vigo_rebound_rounds_mixed: the same, then {T, T_static} of the gates for each count 7 .. Ns (Ns >= 7)
inline size_t ws_rebound_mixed(void* base, size_t B, size_t Ns, int32_t*& flags, int32_t*& idx, int32_t*& count_tab) {
    WsCarver c(base);
    flags = c.take<int32_t>(16);
    idx = c.take<int32_t>(B + 16);
    count_tab = c.take<int32_t>(2 * (Ns - 6));
    return c.bytes();
}

// vigo_bspline_fit_mixed: the sorted order of the T paths, the two prefix tables of tab_ints words, and — in a call that
// builds the operator table — the factorisations' work_doubles
inline size_t ws_fit_mixed(void* base, size_t T, size_t tab_ints, size_t work_doubles, int32_t*& perm, int32_t*& tab, double*& work) {
    WsCarver c(base);
    perm = c.take<int32_t>(ws_even(T));
    tab = c.take<int32_t>(ws_even(tab_ints));
    work = work_doubles ? c.take<double>(work_doubles) : nullptr;
    return c.bytes();
}

// the per-trajectory scratch of vigo_collision_segs / vigo_path_search; want_flags: room for vigo_ctrl_occupancy's flags
template <class Args>
size_t ws_path_search_scratch(void* base, size_t B, size_t N, bool want_flags, Args& a) {
    WsCarver c(base);
    const size_t w = ws_even(B + 1), f = (B * N + 7) & ~(size_t)7;
    a.result = c.take<long long>(8);
    a.in_off = c.take<int32_t>(w); a.n_in = c.take<int32_t>(w); a.pre = c.take<int32_t>(w); a.tstatus = c.take<int32_t>(w);
    a.n_out = c.take<int32_t>(w); a.oseg_off = c.take<int32_t>(w); a.opt_off = c.take<int32_t>(w);
    a.tcounts = c.take<int32_t>(2 * w);
    a.pt = want_flags ? c.take<uint8_t>(f) : nullptr;
    a.ln = want_flags ? c.take<uint8_t>(f) : nullptr;
    return c.bytes();
}

// the S first-choice searches of a path search: end points (the second choices' too: Q2 <= S), paths, then the int32 arrays
template <class Work>
size_t ws_first_searches(void* base, size_t S, size_t search_path_cap, Work& w) {
    WsCarver c(base);
    const size_t e = ws_even(S);
    w.start1 = c.take<double>(3 * S); w.end1 = c.take<double>(3 * S); w.start2 = c.take<double>(3 * S); w.end2 = c.take<double>(3 * S);
    w.path1 = c.take<double>(S * search_path_cap * 3);
    w.seg = c.take<int32_t>(2 * e); w.mseg = c.take<int32_t>(2 * e);
    w.pick = c.take<int32_t>(e); w.retry_of = c.take<int32_t>(e); w.status1 = c.take<int32_t>(e); w.len1 = c.take<int32_t>(e);
    return c.bytes();
}

// its Q2 second-choice searches
template <class Work>
size_t ws_second_searches(void* base, size_t Q2, size_t search_path_cap, Work& w) {
    WsCarver c(base);
    w.path2 = c.take<double>(Q2 * search_path_cap * 3);
    w.status2 = c.take<int32_t>(ws_even(Q2));
    w.len2 = c.take<int32_t>(ws_even(Q2));
    return c.bytes();
}

// vigo_rebound_reguide, per trajectory and control point: the re-guide lists and new segments at a fixed stride of
// max_segs, and the outputs of the path search and of the guide step on those lists
struct ReguideStage {
    int32_t* ps_status;    // [B]
    int32_t* ps_seg_off;   // [B+1]
    int32_t* g_status;     // [B]
    int32_t* ps_counts;    // [B][2]
    int32_t* g_off;        // [B*N+1]
};
template <class Args>
size_t ws_reguide(void* base, size_t B, size_t N, size_t max_segs, Args& r, ReguideStage& s) {
    WsCarver c(base);
    const size_t w = ws_even(B + 1);
    r.result = c.take<long long>(8);
    r.kind = c.take<int32_t>(w); r.n_list = c.take<int32_t>(w); r.n_new = c.take<int32_t>(w); r.outcome = c.take<int32_t>(w);
    s.ps_status = c.take<int32_t>(w); s.ps_seg_off = c.take<int32_t>(w); s.g_status = c.take<int32_t>(w);
    s.ps_counts = c.take<int32_t>(2 * w);
    r.list = c.take<int32_t>(2 * max_segs * B); r.new_seg = c.take<int32_t>(2 * max_segs * B);
    s.g_off = c.take<int32_t>(ws_even(B * N + 1));
    return c.bytes();
}

// ... the path search's output on the lists: out_path [total_pts][3], out_seg [total_seg][2], out_path_off [total_seg+1]
// (one spare point and segment: the buffer is never empty)
template <class Args>
size_t ws_reguide_paths(void* base, size_t total_seg, size_t total_pts, Args& a) {
    WsCarver c(base);
    a.out_path = c.take<double>(3 * total_pts + 1);
    a.out_seg = c.take<int32_t>(2 * total_seg + 2);
    a.out_path_off = c.take<int32_t>(ws_even(total_seg + 1));
    return c.bytes();
}

// ... and the P pairs this step appends, with their unknown flags
inline size_t ws_reguide_pairs(void* base, size_t P, double*& g_pv, uint8_t*& g_unk) {
    WsCarver c(base);
    g_pv = c.take<double>(6 * P);
    g_unk = c.take<uint8_t>(P + 8);
    return c.bytes();
}

}  // namespace vigo
