// solver_fused_plan_check.cpp — fuse_optimize of csrc/vigo_solver_plan.hpp answering queries on a machine without a GPU
// (tests/test_solver_fused_plan.py builds this with the address and undefined-behaviour sanitizers and compares the
// answers with its own restatement of the rule).  One query per line of stdin, one answer per line of stdout:
//   P N B precision obs plan_in_z strict_z mem_size simd_count allow_axis
//        -> "error" (no plan), or "launches d_first fuse grid lds" — the number of launches plan_optimize answers, D of the
//           first, and fuse_optimize's answer over that plan
//   S N mem_size                                   -> solo_lds_bytes
#include <stdio.h>

#include "vigo_solver_plan.hpp"

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int N, B, prec, obs, pz, sz, mem, simds, axis;
        if (sscanf(line, "S %d %d", &N, &mem) == 2) {
            printf("%zu", vigo::solo_lds_bytes(N, mem));
        } else if (sscanf(line, "P %d %d %d %d %d %d %d %d %d", &N, &B, &prec, &obs, &pz, &sz, &mem, &simds, &axis) == 9) {
            const vigo::OptimizePlan p = vigo::plan_optimize(N, B, prec, obs != 0, pz != 0, sz != 0, mem, simds, axis != 0);
            if (p.count < 0) {
                printf("error");
            } else {
                if (p.count < 1 || p.count > 2 || p.launch[0].key < 0 || p.launch[0].key >= vigo::kOptimizeKeyCount) return 2;
                const vigo::FusedLaunch f = vigo::fuse_optimize(p, N, mem);
                printf("%d %d %d %d %zu", p.count, vigo::kOptimizeKeys[p.launch[0].key].d, (int)f.fuse, f.grid, f.lds);
            }
        } else {
            fprintf(stderr, "bad query: %s", line);
            return 1;
        }
        printf("\n");
    }
    return 0;
}
