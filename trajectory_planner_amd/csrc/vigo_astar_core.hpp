// vigo_astar_core.hpp — ONE search of the facade's host A* (host/src/astarOcc.cpp, AStar::AstarSearch + getPath), as the
// code k_astar (vigo_astar.hip) runs and the host compiles too (tests/test_astar_core.py pins it against the host A*
// and the Python restatement of tests/test_astar_restatement.py).
//
// What is reproduced, statement by statement: the lattice centred on the midpoint of start and end with the +0.5 index
// rounding, the ends pushed out of obstacles, the diagonal heuristic with its 1 + 1/10000 factor, the goal test when a
// node is POPPED, neighbours in dx, dy, dz order inside the nx < 1 || nx >= pool - 1 border, one push per node, a better
// path to an open node rewriting g and parent in place with the heap left as it is.  (The host stamps a node as explored
// before its height and map tests, so that a blocked node is asked once; a blocked node is skipped on every visit either
// way — the band and the map answer the same every time — so here it is asked again instead of taking a table slot.)
// The open set is an array heap with exactly libstdc++'s push_heap / pop_heap (bits/stl_heap.h: __push_heap sifts a value up; __adjust_heap moves the hole down
// along the larger child to the bottom, then sifts the last value up from there), comparator f[a] > f[b] with f read
// at comparison time — f is not stored: the host always writes f = g + heuristic(node, goal), so it is recomputed from
// g bit for bit.
//
// What differs: the host's dense node pool is a bounded open-addressing table keyed by the node's lattice index (the
// pool padded to 1024 per axis: x | y << 10 | z << 20, so the coordinates come back with shifts), and the 0.2 s wall
// clock is replaced by budgets — a full table or heap, or max_expansions pops without an end, stop the search with
// kAstarDeferred and NO result; the caller runs the host A* for it.
//
// An expansion is two phases.  astar_probe(k) looks at neighbour k alone (table probe, height band, map bit, g through
// the expanded node): the 26 neighbours of a node are distinct nodes, so the 26 probes are independent — 26 lanes on
// the device, a loop on the host.  astar_commit() then takes the candidates in the host's neighbour order: insert +
// push for a new node, rewrite for a better path; the order matters because a rewrite changes what a later push's
// sift-up compares against.  Every fp64 expression is compiled without contraction, with IEEE sqrt and division.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#ifndef VIGO_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VIGO_HD __host__ __device__ __forceinline__
#else
#define VIGO_HD inline
#endif
#endif

namespace vigo {

// per-search status (include/vigo.h VIGO_ASTAR_*)
enum {
    kAstarFound = 0,
    kAstarNotFound = 1,      // the ends do not fit the pool (adjustEnds false), or the open set ran empty
    kAstarDeferred = 2,      // a budget ran out: no result, the host A* decides
    kAstarPathTooLong = 3,   // found, but the path has more than path_cap points (out_len says how many)
    kAstarRunning = -1,      // (internal)
};
constexpr int kAstarMaxPoolAxis = 1024;   // 10 bits per axis in a node key
constexpr int kAstarNoDir = 13;           // direction index (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) of (0, 0, 0): the start's parent

// node meta byte: bits 0-4 the direction FROM the parent, 5 open, 6 closed
enum : uint8_t { kAstarOpen = 32, kAstarClosed = 64 };

struct AstarGeom {
    double center[3], step, inv_step, min_h, max_h;
    int pool[3], cidx[3];
};

VIGO_HD void astar_geom(AstarGeom& G, const double s[3], const double e[3], double step, const int pool[3], double min_h,
                        double max_h) {
    for (int a = 0; a < 3; ++a) {
        G.center[a] = (s[a] + e[a]) / 2;
        G.pool[a] = pool[a];
        G.cidx[a] = pool[a] / 2;
    }
    G.step = step;
    G.inv_step = 1 / step;
    G.min_h = min_h;
    G.max_h = max_h;
}

// astarOcc.cpp coord2idx: (int)((p - center) * invStep + 0.5) + centerIdx, false outside the pool.  A value no int holds
// (the conversion is INT_MIN on x86: outside) or a NaN is outside.
VIGO_HD bool astar_coord2idx(const AstarGeom& G, const double p[3], int idx[3]) {
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        const double v = (p[a] - G.center[a]) * G.inv_step + 0.5;
        if (!(v > -1e9 && v < 1e9)) { idx[a] = -1; in = false; continue; }
        idx[a] = (int)v + G.cidx[a];
        if (idx[a] < 0 || idx[a] >= G.pool[a]) in = false;
    }
    return in;
}

VIGO_HD double astar_idx2coord(const AstarGeom& G, int a, int i) { return (i - G.cidx[a]) * G.step + G.center[a]; }

// astarOcc.cpp adjustEnds: an end whose node is occupied walks away from the other end, one step at a time, until its
// node is free or leaves the pool.  (A walk of 4096 steps has left any pool of kAstarMaxPoolAxis nodes per axis; one
// that has not is not advancing — a step below the coordinates' precision, where the host's loop never ends.)
template <class Occ>
VIGO_HD bool astar_adjust_ends(const AstarGeom& G, const Occ& occ, double s[3], double e[3], int si[3], int ei[3]) {
    const bool s_in = astar_coord2idx(G, s, si), e_in = astar_coord2idx(G, e, ei);
    if (!s_in || !e_in) return false;
    for (int end = 0; end < 2; ++end) {
        double* p = end ? e : s;
        const double* o = end ? s : e;
        int* pi = end ? ei : si;
        if (!occ(astar_idx2coord(G, 0, pi[0]), astar_idx2coord(G, 1, pi[1]), astar_idx2coord(G, 2, pi[2]))) continue;
        int walked = 0;
        do {
            if (++walked > 4096) return false;
            const double d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
            const double n = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            for (int a = 0; a < 3; ++a) p[a] = d[a] / n * G.step + p[a];
            if (!astar_coord2idx(G, p, pi)) return false;
        } while (occ(astar_idx2coord(G, 0, pi[0]), astar_idx2coord(G, 1, pi[1]), astar_idx2coord(G, 2, pi[2])));
    }
    return true;
}

VIGO_HD int astar_key(int x, int y, int z) { return x | (y << 10) | (z << 20); }

// astarOcc.cpp heuristic (diagonal distance over the three step lengths) between node `key` and the goal
VIGO_HD double astar_heuristic(int key, const int goal[3]) {
    double dx = abs((key & 1023) - goal[0]), dy = abs(((key >> 10) & 1023) - goal[1]), dz = abs((key >> 20) - goal[2]);
    const int diag = (int)fmin(fmin(dx, dy), dz);
    dx -= diag; dy -= diag; dz -= diag;
    double h = 0.0;
    if (dx == 0) h = sqrt(3.0) * diag + sqrt(2.0) * fmin(dy, dz) + fabs(dy - dz);
    if (dy == 0) h = sqrt(3.0) * diag + sqrt(2.0) * fmin(dx, dz) + fabs(dx - dz);
    if (dz == 0) h = sqrt(3.0) * diag + sqrt(2.0) * fmin(dx, dy) + fabs(dx - dy);
    return (1.0 + 1.0 / 10000) * h;
}

// sqrt(dx^2 + dy^2 + dz^2) of a neighbour step: the same three doubles as the host's table
VIGO_HD double astar_step_len(int nonzero) { return nonzero == 1 ? 1.0 : nonzero == 2 ? sqrt(2.0) : sqrt(3.0); }

// The node table and the open set of one search.  Slot: the integer a heap entry holds (a table slot).
template <class Slot>
struct AstarStore {
    int32_t* key;      // [1 << cap_log2]  node key, -1 = empty
    double* g;         // [1 << cap_log2]
    uint8_t* meta;     // [1 << cap_log2]
    Slot* heap;        // [heap_cap]
    int cap_log2;
    int max_nodes;     // < 1 << cap_log2: a probe always meets an empty slot
    int heap_cap;
    int goal[3];
    int n_nodes, n_heap, heap_peak, pops, rewrites;
};

template <class Slot>
VIGO_HD double astar_f(const AstarStore<Slot>& S, int slot) { return S.g[slot] + astar_heuristic(S.key[slot], S.goal); }

// the slot of `key`, or the empty slot its insertion would take (found says which)
template <class Slot>
VIGO_HD int astar_find(const AstarStore<Slot>& S, int key, bool& found) {
    const int mask = (1 << S.cap_log2) - 1;
    int i = (int)(((uint32_t)key * 2654435761u) >> (32 - S.cap_log2));
    for (;;) {
        const int k = S.key[i];
        if (k == key) { found = true; return i; }
        if (k < 0) { found = false; return i; }
        i = (i + 1) & mask;
    }
}

// bits/stl_heap.h __push_heap(first, hole, top, value, comp) with comp(a, b) = f[a] > f[b]
template <class Slot>
VIGO_HD void astar_sift_up(AstarStore<Slot>& S, int hole, int top, Slot value) {
    const double fv = astar_f(S, value);
    int parent = (hole - 1) / 2;
    while (hole > top && astar_f(S, S.heap[parent]) > fv) {
        S.heap[hole] = S.heap[parent];
        hole = parent;
        parent = (hole - 1) / 2;
    }
    S.heap[hole] = value;
}

// priority_queue::push: push_back + push_heap.  The caller has checked n_heap < heap_cap.
template <class Slot>
VIGO_HD void astar_push(AstarStore<Slot>& S, Slot v) {
    const int n = S.n_heap++;
    if (S.n_heap > S.heap_peak) S.heap_peak = S.n_heap;
    astar_sift_up(S, n, 0, v);
}

// priority_queue::top + pop: pop_heap (__pop_heap -> __adjust_heap(first, 0, n - 1, last value)) + pop_back
template <class Slot>
VIGO_HD Slot astar_pop(AstarStore<Slot>& S) {
    const Slot top = S.heap[0];
    const int n = --S.n_heap;               // the heap without its last element, whose value is re-inserted from the top
    if (n == 0) return top;
    const Slot value = S.heap[n];
    int hole = 0, second = 0;
    while (second < (n - 1) / 2) {
        second = 2 * (second + 1);
        if (astar_f(S, S.heap[second]) > astar_f(S, S.heap[second - 1])) --second;
        S.heap[hole] = S.heap[second];
        hole = second;
    }
    if ((n & 1) == 0 && second == (n - 2) / 2) {
        second = 2 * (second + 1);
        S.heap[hole] = S.heap[second - 1];
        hole = second - 1;
    }
    astar_sift_up(S, hole, 0, value);
    return top;
}

// what astar_probe found out about one neighbour
struct AstarCand {
    double g;        // through the expanded node
    int32_t key;
    int32_t slot;    // the node's slot, or where its insertion starts probing
    int32_t what;    // kCandSkip / kCandNew / kCandOpen
};
enum { kCandSkip = 0, kCandNew = 1, kCandOpen = 2 };

// neighbour k = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) of the expanded node (key cur, cost g_cur): AstarSearch's loop
// body up to the point where it writes.  occ(x, y, z): the map's isInflatedOccupied.
template <class Slot, class Occ>
VIGO_HD void astar_probe(const AstarStore<Slot>& S, const AstarGeom& G, const Occ& occ, int cur, double g_cur, int k, AstarCand& c) {
    const int dx = k / 9 - 1, dy = (k / 3) % 3 - 1, dz = k % 3 - 1;
    const int nx = (cur & 1023) + dx, ny = ((cur >> 10) & 1023) + dy, nz = (cur >> 20) + dz;
    c.what = kCandSkip;
    c.key = 0;
    c.slot = 0;
    c.g = 0.0;
    if (k == kAstarNoDir) return;
    if (nx < 1 || nx >= G.pool[0] - 1 || ny < 1 || ny >= G.pool[1] - 1 || nz < 1 || nz >= G.pool[2] - 1) return;
    c.key = astar_key(nx, ny, nz);
    bool found;
    c.slot = astar_find(S, c.key, found);
    c.g = g_cur + astar_step_len(dx * dx + dy * dy + dz * dz);
    if (found) {
        if (S.meta[c.slot] & kAstarOpen) c.what = kCandOpen;      // closed: nothing to do
        return;
    }
    const double z = astar_idx2coord(G, 2, nz);
    const bool blocked = z > G.max_h || z < G.min_h || occ(astar_idx2coord(G, 0, nx), astar_idx2coord(G, 1, ny), z);
    c.what = blocked ? kCandSkip : kCandNew;
}

// the writes of AstarSearch's loop body for the 27 candidates of one expansion, in neighbour order.  false: the table
// or the heap is full (the search is deferred).
template <class Slot>
VIGO_HD bool astar_commit(AstarStore<Slot>& S, const AstarCand* cand) {
    const int mask = (1 << S.cap_log2) - 1;
    for (int k = 0; k < 27; ++k) {
        const AstarCand c = cand[k];
        if (c.what == kCandSkip) continue;
        if (c.what == kCandOpen) {
            if (c.g < S.g[c.slot]) {                  // better path to an open node: rewritten where it sits in the heap
                S.g[c.slot] = c.g;
                S.meta[c.slot] = (uint8_t)(kAstarOpen | k);
                ++S.rewrites;
            }
            continue;
        }
        if (S.n_nodes >= S.max_nodes || S.n_heap >= S.heap_cap) return false;
        int i = c.slot;                               // (an earlier insert of this expansion may have taken the slot)
        while (S.key[i] >= 0) i = (i + 1) & mask;
        S.key[i] = c.key;
        ++S.n_nodes;
        S.g[i] = c.g;
        S.meta[i] = (uint8_t)(kAstarOpen | k);
        astar_push(S, (Slot)i);
    }
    return true;
}

// the start node (AstarSearch before its loop).  The table is empty (every key -1).
template <class Slot>
VIGO_HD void astar_begin(AstarStore<Slot>& S, const int si[3], const int ei[3]) {
    for (int a = 0; a < 3; ++a) S.goal[a] = ei[a];
    S.n_nodes = S.n_heap = S.heap_peak = S.pops = S.rewrites = 0;
    bool found;
    const int key = astar_key(si[0], si[1], si[2]);
    const int i = astar_find(S, key, found);
    S.key[i] = key;
    S.g[i] = 0.0;
    S.meta[i] = (uint8_t)(kAstarOpen | kAstarNoDir);
    S.n_nodes = 1;
    astar_push(S, (Slot)i);
}

// the head of AstarSearch's loop: kAstarRunning with the popped node (closed now) in *cur / *g_cur, or the search's end
template <class Slot>
VIGO_HD int astar_next(AstarStore<Slot>& S, int max_expansions, int* cur, double* g_cur, int* cur_slot) {
    if (S.n_heap == 0) return kAstarNotFound;
    if (S.pops >= max_expansions) return kAstarDeferred;
    const int slot = (int)astar_pop(S);
    ++S.pops;
    *cur = S.key[slot];
    *g_cur = S.g[slot];
    *cur_slot = slot;
    if (*cur == astar_key(S.goal[0], S.goal[1], S.goal[2])) return kAstarFound;
    S.meta[slot] = (uint8_t)((S.meta[slot] & 31) | kAstarClosed);
    return kAstarRunning;
}

// AstarSearch's parent walk + getPath: the number of path points from the goal (in slot goal_slot) back to the start;
// with out != NULL and that number <= path_cap the points are written start side first, out[i][3]
template <class Slot>
VIGO_HD int astar_path(const AstarStore<Slot>& S, const AstarGeom& G, int goal_slot, int path_cap, double* out) {
    int len = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int slot = goal_slot, i = 0;
        for (;;) {
            const int key = S.key[slot];
            if (pass) {
                double* o = out + (size_t)(len - 1 - i) * 3;
                o[0] = astar_idx2coord(G, 0, key & 1023);
                o[1] = astar_idx2coord(G, 1, (key >> 10) & 1023);
                o[2] = astar_idx2coord(G, 2, key >> 20);
            }
            ++i;
            const int k = S.meta[slot] & 31;
            if (k == kAstarNoDir || i > S.max_nodes) break;    // (a path visits a node once: the bound is never met)
            bool found;
            slot = astar_find(S, astar_key((key & 1023) - (k / 9 - 1), ((key >> 10) & 1023) - ((k / 3) % 3 - 1), (key >> 20) - (k % 3 - 1)), found);
        }
        len = i;
        if (!out || len > path_cap) break;
    }
    return len;
}

// One whole search, the two phases of an expansion one after the other: what the host runs (the kernel runs the same
// functions with the probes spread over lanes).  The caller provides the store with every key -1.
template <class Slot, class Occ>
inline int astar_search(AstarStore<Slot>& S, const Occ& occ, const double start[3], const double end[3], double step, const int pool[3],
                        double min_h, double max_h, int max_expansions, int path_cap, double* out_path, int* out_len) {
    AstarGeom G;
    double s[3] = {start[0], start[1], start[2]}, e[3] = {end[0], end[1], end[2]};
    int si[3], ei[3];
    astar_geom(G, s, e, step, pool, min_h, max_h);
    S.n_nodes = S.n_heap = S.heap_peak = S.pops = S.rewrites = 0;
    *out_len = 0;
    if (!astar_adjust_ends(G, occ, s, e, si, ei)) return kAstarNotFound;
    astar_begin(S, si, ei);
    for (;;) {
        int cur, slot;
        double g_cur;
        const int st = astar_next(S, max_expansions, &cur, &g_cur, &slot);
        if (st == kAstarFound) {
            *out_len = astar_path(S, G, slot, path_cap, out_path);
            return *out_len > path_cap ? kAstarPathTooLong : kAstarFound;
        }
        if (st != kAstarRunning) return st;
        AstarCand cand[27];
        for (int k = 0; k < 27; ++k) astar_probe(S, G, occ, cur, g_cur, k, cand[k]);
        if (!astar_commit(S, cand)) return kAstarDeferred;
    }
}

}  // namespace vigo
