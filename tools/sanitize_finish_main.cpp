// sanitize_finish_main.cpp — vigo_traj_finish_host (csrc/vigo_finish.hip: the rule of csrc/vigo_finish_core.hpp on the
// host) under AddressSanitizer + UBSan, built by tools/sanitize_host.sh as a programme of its own: hostile counts next to
// valid rows in buffers of exactly the stated sizes (the sanitizer sees a read past a row's count or a write past
// S_cap), capacities of 1, NaN and infinite control points, steps that make one sample or thousands.  No GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../include/vigo.h"

int main() {
    std::mt19937_64 rng(20261020);
    std::uniform_real_distribution<double> u(-3.0, 3.0);
    long long rows = 0, invalid = 0, capacity = 0;
    for (int round = 0; round < 400; ++round) {
        const int Ns = 7 + (int)(rng() % 60), B = 1 + (int)(rng() % 9);
        const double ts_ctrl = round % 3 == 0 ? 0.25 : 0.2, ts = round % 5 == 0 ? 0.013 : 0.1;
        const double dt = round % 7 == 0 ? 100.0 : (round % 4 == 0 ? 0.003 : 0.1);
        const int S_cap = round % 6 == 0 ? 1 : 1 + (int)(rng() % 300);
        std::vector<int32_t> n_pts(B);
        std::vector<double> ctrl, limits(2 * (size_t)B);
        for (int b = 0; b < B; ++b) {
            const int kind = (int)(rng() % 8);
            n_pts[b] = kind == 0 ? 6 : kind == 1 ? Ns + 1 : kind == 2 ? -5 : kind == 3 ? INT32_MAX : 7 + (int)(rng() % (Ns - 6));
            limits[2 * b] = 1.0 + u(rng) * 0.2;
            limits[2 * b + 1] = 2.0 + u(rng) * 0.2;
        }
        // rows of exactly Ns points; a sprinkle of NaN / inf
        ctrl.resize((size_t)B * Ns * 3);
        for (double& c : ctrl) c = u(rng);
        if (round % 9 == 0) ctrl[rng() % ctrl.size()] = NAN;
        if (round % 11 == 0) ctrl[rng() % ctrl.size()] = INFINITY;
        const bool uniform = round % 10 == 0;
        std::vector<double> factor(B), mx(2 * (size_t)B), pos((size_t)B * S_cap * 3), vel((size_t)B * S_cap * 3);
        std::vector<int32_t> n(B), status(B);
        const int rc = vigo_traj_finish_host(ts_ctrl, ts, B, Ns, uniform ? nullptr : n_pts.data(), ctrl.data(), limits.data(), dt, S_cap, factor.data(),
                                             round % 2 ? mx.data() : nullptr, n.data(), pos.data(), round % 3 ? vel.data() : nullptr, status.data());
        if (rc != VIGO_OK) { std::printf("round %d: rc %d\n", round, rc); return 1; }
        for (int b = 0; b < B; ++b) {
            ++rows;
            invalid += status[b] == VIGO_FINISH_INVALID_N;
            capacity += status[b] == VIGO_FINISH_CAPACITY;
            const bool bad = !uniform && (n_pts[b] < 7 || n_pts[b] > Ns);
            if (bad != (status[b] == VIGO_FINISH_INVALID_N)) { std::printf("round %d row %d: status %d for count %d\n", round, b, status[b], n_pts[b]); return 1; }
            if (!bad && (status[b] == VIGO_FINISH_CAPACITY) != (n[b] > S_cap)) { std::printf("round %d row %d: capacity status\n", round, b); return 1; }
        }
    }
    // the refusals write nothing and read nothing
    double one = 0.0;
    int32_t i1 = 0;
    if (vigo_traj_finish_host(0.2, 0.1, 1, 6, nullptr, &one, &one, 0.1, 1, &one, nullptr, &i1, &one, nullptr, &i1) != VIGO_ERR_UNSUPPORTED_N ||
        vigo_traj_finish_host(0.2, 0.1, 1, 7, nullptr, &one, &one, 0.0, 1, &one, nullptr, &i1, &one, nullptr, &i1) != VIGO_ERR_INVALID_ARG ||
        vigo_traj_finish_host(0.2, 0.1, 1, 7, nullptr, nullptr, &one, 0.1, 1, &one, nullptr, &i1, &one, nullptr, &i1) != VIGO_ERR_INVALID_ARG ||
        vigo_traj_finish_host(0.2, 0.1, 0, 7, nullptr, nullptr, nullptr, 0.1, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != VIGO_OK) {
        std::printf("a refusal is wrong\n");
        return 1;
    }
    std::printf("sanitize_finish: %lld rows (%lld invalid counts, %lld over capacity), clean\n", rows, invalid, capacity);
    return 0;
}
