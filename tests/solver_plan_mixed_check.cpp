// solver_plan_mixed_check.cpp — the mixed-count plan of csrc/vigo_solver_plan.hpp and the workspace of
// vigo_rebound_rounds_mixed (csrc/vigo_ws_layout.hpp) on a machine without a GPU; tests/test_solver_plan_mixed.py builds this
// with the address and undefined-behaviour sanitizers.  One query per line of stdin, one answer per line of stdout:
//   K                                   -> kOptimizeKeys: one "precision group ppl wps obs d rh" per key, ';' between
//   MK                                  -> kOptimizeMixedKeys, the same way
//   R N mem_size precision              -> optimize_lds_requirement (the general kernel with its obstacle table)
//   M Ns B precision obs mem_size simd_count
//                                       -> "error", or per launch "precision group ppl wps obs d rh grid lds
//                                          level_waves_elsewhere", ';' between
//   C n Ns                              -> mixed_count_ok
//   W B Ns                              -> ws_rebound_mixed carved out of exactly its own size and written: "bytes"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vigo_solver_plan.hpp"
#include "vigo_ws_layout.hpp"

static void print_key(const vigo::OptimizeKey& k) {
    printf("%d %d %d %d %d %d %d", k.precision, k.group, k.ppl, k.wps, (int)k.obs, k.d, k.rh);
}

int main() {
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        int N, B, prec, obs, mem, simds;
        if (line[0] == 'K' || (line[0] == 'M' && line[1] == 'K')) {
            const bool mixed = line[0] == 'M';
            const int n = mixed ? vigo::kOptimizeMixedKeyCount : vigo::kOptimizeKeyCount;
            for (int i = 0; i < n; ++i) {
                if (i) printf(";");
                print_key(mixed ? vigo::kOptimizeMixedKeys[i] : vigo::kOptimizeKeys[i]);
            }
        } else if (sscanf(line, "R %d %d %d", &N, &mem, &prec) == 3) {
            printf("%zu", vigo::optimize_lds_requirement(N, mem, prec));
        } else if (sscanf(line, "M %d %d %d %d %d %d", &N, &B, &prec, &obs, &mem, &simds) == 6) {
            const vigo::OptimizePlan p = vigo::plan_optimize_mixed(N, B, prec, obs != 0, mem, simds);
            if (p.count < 0) printf("error");
            for (int i = 0; i < p.count; ++i) {
                const vigo::PlannedLaunch& l = p.launch[i];
                if (l.key < 0 || l.key >= vigo::kOptimizeMixedKeyCount) return 2;
                if (i) printf(";");
                print_key(vigo::kOptimizeMixedKeys[l.key]);
                printf(" %d %zu %d", l.grid, l.lds, l.level_waves_elsewhere);
            }
        } else if (sscanf(line, "C %d %d", &N, &B) == 2) {
            printf("%d", (int)vigo::mixed_count_ok(N, B));
        } else if (sscanf(line, "W %d %d", &B, &N) == 2) {
            int32_t *flags, *idx, *tab;
            const size_t bytes = vigo::ws_rebound_mixed(nullptr, (size_t)B, (size_t)N, flags, idx, tab);
            if (flags || idx || tab) return 3;                  // a null base only measures
            char* base = static_cast<char*>(malloc(bytes));     // exactly the size asked for: ASan sees a byte beyond
            if (vigo::ws_rebound_mixed(base, (size_t)B, (size_t)N, flags, idx, tab) != bytes) return 4;
            if ((uintptr_t)flags % 8 || (uintptr_t)idx % 8 || (uintptr_t)tab % 8) return 5;
            // the extents the kernels index: 16 flags, B indices, {T, T_static} per count 7 .. Ns; distinct fills show overlap
            memset(flags, 1, 16 * sizeof(int32_t));
            memset(idx, 2, (size_t)B * sizeof(int32_t));
            memset(tab, 3, 2 * (size_t)(N - 6) * sizeof(int32_t));
            for (int i = 0; i < 16; ++i) if (flags[i] != 0x01010101) return 6;
            for (int i = 0; i < B; ++i) if (idx[i] != 0x02020202) return 6;
            for (int i = 0; i < 2 * (N - 6); ++i) if (tab[i] != 0x03030303) return 6;
            free(base);
            printf("%zu", bytes);
        } else {
            fprintf(stderr, "bad query: %s", line);
            return 1;
        }
        printf("\n");
    }
    return 0;
}
