// solver_plan_check.cpp — csrc/vigo_solver_plan.hpp answering queries on a machine without a GPU (tests/test_solver_plan.py
// builds this with the address and undefined-behaviour sanitizers and compares the answers with tests/solver_dispatch_rule.py).
// One query per line of stdin, one answer per line of stdout:
//   K                                              -> the key list: one "precision group ppl wps obs d rh" per key, ';' between
//   R N mem_size precision                         -> optimize_lds_requirement
//   P N B precision obs plan_in_z strict_z mem_size simd_count allow_axis
//                                                  -> "error", or per launch "precision group ppl wps obs d rh grid lds
//                                                     level_waves_elsewhere", ';' between
#include <stdio.h>

#include "vigo_solver_plan.hpp"

static void print_key(const vigo::OptimizeKey& k) {
    printf("%d %d %d %d %d %d %d", k.precision, k.group, k.ppl, k.wps, (int)k.obs, k.d, k.rh);
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int N, B, prec, obs, pz, sz, mem, simds, axis;
        if (line[0] == 'K') {
            for (int i = 0; i < vigo::kOptimizeKeyCount; ++i) {
                if (i) printf(";");
                print_key(vigo::kOptimizeKeys[i]);
            }
        } else if (sscanf(line, "R %d %d %d", &N, &mem, &prec) == 3) {
            printf("%zu", vigo::optimize_lds_requirement(N, mem, prec));
        } else if (sscanf(line, "P %d %d %d %d %d %d %d %d %d", &N, &B, &prec, &obs, &pz, &sz, &mem, &simds, &axis) == 9) {
            const vigo::OptimizePlan p = vigo::plan_optimize(N, B, prec, obs != 0, pz != 0, sz != 0, mem, simds, axis != 0);
            if (p.count < 0) printf("error");
            for (int i = 0; i < p.count; ++i) {
                const vigo::PlannedLaunch& l = p.launch[i];
                if (l.key < 0 || l.key >= vigo::kOptimizeKeyCount) return 2;
                if (i) printf(";");
                print_key(vigo::kOptimizeKeys[l.key]);
                printf(" %d %zu %d", l.grid, l.lds, l.level_waves_elsewhere);
            }
        } else {
            fprintf(stderr, "bad query: %s", line);
            return 1;
        }
        printf("\n");
    }
    return 0;
}
