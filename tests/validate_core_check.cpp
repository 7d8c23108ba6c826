// validate_core_check.cpp — a program of its own (tests/test_validate_core.py builds it with the address and
// undefined-behaviour sanitizers and runs it): the per-lane functions of csrc/vigo_validate_core.hpp walked on the host the
// way k_traj_validate walks them — the row copied into a buffer of exactly 3 n doubles, blocks of 64 lanes, two ballots, the
// uniform exit test — over counts at both ends of 4 .. Ns and outside it, with every table allocated at its exact size, and
// held against the walk with one lane (what vigo_traj_validate_host runs).  Prints one line per stride; exit status 1 on a
// difference.
#include <limits.h>
#include <stdio.h>

#include <vector>

#include "vigo_seed_core.hpp"
#include "vigo_validate_core.hpp"

using namespace vigo;

namespace {

struct Result {
    int status, first, dyn_first;
    double pos[3];
    bool operator==(const Result& o) const {
        return status == o.status && first == o.first && dyn_first == o.dyn_first && (first < 0 || memcmp(pos, o.pos, sizeof pos) == 0);
    }
};

// one row by blocks of `stride` lanes (64: the kernel's loop; 1: the host twin's)
Result walk(const SeedByteGrid& occ, const double* ctrl, int Ns, int n, int b, double ts_ctrl, const std::vector<double>& times,
            const std::vector<int32_t>& tab, const int32_t* obs_off, const double* obs, int n_obs_shared, int stride) {
    Result R{kValidBadCount, -1, -1, {0, 0, 0}};
    if (!validate_count_ok(n, Ns)) return R;
    std::vector<double> c(3 * (size_t)n);                                 // the wave's slice of LDS, at the row's own size
    const double* src = ctrl + (size_t)b * Ns * 3;
    for (int lane = 0; lane < stride; ++lane)
        for (int i = lane; i < 3 * n; i += stride) c[i] = src[i];
    ValidateRow r;
    r.n = n;
    r.S = tab.at(2 * (size_t)(n - kValidateMinN));
    r.C = tab.at(2 * (size_t)(n - kValidateMinN) + 1);
    if (r.S > (int)times.size()) r.S = (int)times.size();
    if (r.C > r.S) r.C = r.S;
    validate_obs_range(obs_off, obs, n_obs_shared, b, r.o0, r.o1);
    int first = -1, dyn_first = -1;
    for (int base = 0; base < r.S; base += stride) {
        std::vector<int> bits((size_t)stride);
        std::vector<double> p(3 * (size_t)stride);
        for (int lane = 0; lane < stride; ++lane) {
            double q[3] = {0, 0, 0};
            bits[lane] = validate_sample(c.data(), r, ts_ctrl, times.data(), base + lane, occ, obs, first < 0, dyn_first < 0, q);
            for (int a = 0; a < 3; ++a) p[3 * (size_t)lane + a] = q[a];
        }
        for (int lane = 0; lane < stride && first < 0; ++lane)            // the ballot's lowest set lane
            if (bits[lane] & kValidStatic) {
                first = base + lane;
                for (int a = 0; a < 3; ++a) R.pos[a] = finish_sample(p[3 * (size_t)lane + a]);
            }
        for (int lane = 0; lane < stride && dyn_first < 0; ++lane)
            if (bits[lane] & kValidDynamic) dyn_first = base + lane;
        if (validate_done(r, base, stride, first, dyn_first)) break;
    }
    R.status = validate_status(first, dyn_first);
    R.first = first;
    R.dyn_first = dyn_first;
    return R;
}

}  // namespace

int main() {
    // a 32 x 16 x 8 world at 0.1 with a wall across x = 1.6 .. 1.7
    const int nx = 32, ny = 16, nz = 8;
    std::vector<uint8_t> vox((size_t)nx * ny * nz, 0);
    for (int j = 0; j < ny; ++j)
        for (int k = 0; k < nz; ++k) vox[((size_t)16 * ny + j) * nz + k] = 1;
    const SeedByteGrid occ{vox.data(), nx, ny, nz, {0.0, 0.0, 0.0}, 0.1};
    const double ts_ctrl = 0.2, dt = 0.11;
    const double shared_obs[2 * 9] = {0.6, 0.8, 0.4, 0, 0, 0, 0.1, 0.3, 0.5, 2.9, 0.8, 0.4, 0, 0, 0, 0.2, 0.2, 0.5};
    long rows = 0, hits = 0, bad = 0;
    for (int Ns : {4, 5, 7, 64, 255, 256}) {
        const int counts[] = {Ns, 4, Ns - 1, Ns + 1, 3, 0, -1, INT_MAX, INT_MIN, (Ns + 4) / 2, Ns, 4};
        const int B = (int)(sizeof counts / sizeof counts[0]);
        std::vector<double> ctrl((size_t)B * Ns * 3);
        for (int b = 0; b < B; ++b) {
            const int n = validate_count_ok(counts[b], Ns) ? counts[b] : Ns;
            // along x from 0.35: rows 0 .. 5 stop before the wall, the others cross it and (the last two) leave the box
            const double reach = b < 6 ? 0.9 : (b < 10 ? 2.2 : 4.0);
            for (int i = 0; i < Ns; ++i) {
                const double s = i < n ? (n > 1 ? (double)i / (n - 1) : 0.0) : 1.0;
                ctrl[((size_t)b * Ns + i) * 3] = 0.35 + reach * s;
                ctrl[((size_t)b * Ns + i) * 3 + 1] = 0.45 + 0.05 * b;
                ctrl[((size_t)b * Ns + i) * 3 + 2] = 0.45;
            }
        }
        ctrl[((size_t)10 * Ns + 1) * 3 + 1] = NAN;                       // a NaN coordinate on a good row
        std::vector<int32_t> obs_off((size_t)B + 1);
        for (int b = 0; b <= B; ++b) obs_off[b] = b < 4 ? 0 : (b < 8 ? 1 : 2);     // empty ranges, one, one, empty
        for (int rule : {kValidateByTime, kValidateByIndex})
            for (double ratio : {0.0, 1.0 / 3.0, 1.0}) {
                std::vector<int32_t> tab((size_t)validate_tab_entries(Ns));
                for (int n = kValidateMinN; n <= Ns; ++n)
                    if (!validate_counts(dt, ts_ctrl, ratio, rule, n, &tab[2 * (size_t)(n - kValidateMinN)], &tab[2 * (size_t)(n - kValidateMinN) + 1])) return 2;
                std::vector<double> times((size_t)tab[2 * (size_t)(Ns - kValidateMinN)]);
                double t = 0.0;
                for (size_t k = 0; k < times.size(); ++k, t += dt) times[k] = t;
                for (int lists = 0; lists < 3; ++lists) {                 // none, per-row ranges, shared
                    const int32_t* off = lists == 1 ? obs_off.data() : nullptr;
                    const double* obs = lists == 0 ? nullptr : shared_obs;
                    const int n_shared = lists == 2 ? 2 : 0;
                    for (int b = 0; b < B; ++b) {
                        const Result wave = walk(occ, ctrl.data(), Ns, counts[b], b, ts_ctrl, times, tab, off, obs, n_shared, 64);
                        const Result one = walk(occ, ctrl.data(), Ns, counts[b], b, ts_ctrl, times, tab, off, obs, n_shared, 1);
                        ++rows;
                        hits += wave.status != 0 && wave.status != kValidBadCount;
                        if (!(wave == one) || (wave.status == kValidBadCount) != !validate_count_ok(counts[b], Ns)) {
                            ++bad;
                            fprintf(stderr, "Ns %d row %d n %d rule %d ratio %g lists %d: 64 lanes {%d %d %d} != one lane {%d %d %d}\n", Ns, b, counts[b], rule,
                                    ratio, lists, wave.status, wave.first, wave.dyn_first, one.status, one.first, one.dyn_first);
                        }
                    }
                }
            }
    }
    // the closed form of the BY_INDEX prefix against the literal loop of BT.h:329, every count 4 .. 256
    for (double ratio : {0.0, 1.0 / 3.0, 0.5, 1.0, 0.1, 0.9, 0.999, 1e-9, 0.25, 2.0 / 3.0})
        for (int n = kValidateMinN; n <= VIGO_MAX_CTRL_POINTS; ++n)
            for (double step : {0.05, 0.11, 0.1 / 3}) {
                const int S = count_sample_times(step, finish_duration(n, ts_ctrl));
                int literal = 0;
                for (int i = 0; i < (1.0 - ratio) * int(S); ++i) ++literal;
                if (validate_checked_by_index(ratio, S) != literal) {
                    ++bad;
                    fprintf(stderr, "prefix: ratio %g n %d S %d: closed form %d != literal %d\n", ratio, n, S, validate_checked_by_index(ratio, S), literal);
                }
            }
    printf("rows %ld hits %ld differences %ld\n", rows, hits, bad);
    return bad ? 1 : 0;
}
