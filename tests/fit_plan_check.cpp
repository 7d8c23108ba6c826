// fit_plan_check.cpp — the work plan of vigo_bspline_fit_mixed (csrc/vigo_fit_plan.hpp) on a machine without a GPU;
// tests/test_fit_plan.py builds this with the address and undefined-behaviour sanitizers.  Queries on stdin, white space
// between the words, one answer line each:
//   O                               -> fit_table_offset(K) for K = 4 .. 63, fit_table_work_offset(K) for K = 4 .. 63, then
//                                      fit_table_doubles(), fit_table_work_doubles()
//   P Ns point_stride T  K_0 status_0 ... K_{T-1} status_{T-1}
//                                   -> "bound total | bin_0 .. bin_{T-1} | K first members m_0 .. ; K first members ... ; ..."
//                                      the paths' bins, then every wave-group 0 .. total-1 with its members: the paths at
//                                      first .. first + members - 1 of the sorted order (a bin's paths in ascending index,
//                                      the bins one after the other as path_prefix places them)
//   G g  c_0 .. c_58                -> fit_group_of on the prefixes of these counts: "K first members"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "vigo_fit_plan.hpp"

int main() {
    char q[8];
    while (scanf("%7s", q) == 1) {
        if (q[0] == 'O') {
            for (int K = vigo::kFitMixedMinK; K <= vigo::kFitMixedMaxK + 1; ++K) printf("%zu ", vigo::fit_table_offset(K));
            for (int K = vigo::kFitMixedMinK; K <= vigo::kFitMixedMaxK + 1; ++K) printf("%zu ", vigo::fit_table_work_offset(K));
            printf("%zu %zu", vigo::fit_table_doubles(), vigo::fit_table_work_doubles());
        } else if (q[0] == 'P') {
            int Ns, stride, T;
            if (scanf("%d %d %d", &Ns, &stride, &T) != 3 || T < 0) return 1;
            std::vector<int> bin((size_t)T), cnt(vigo::kFitBins, 0);   // exact sizes: ASan sees an index beyond
            for (int t = 0; t < T; ++t) {
                int K, status;
                if (scanf("%d %d", &K, &status) != 2) return 1;
                bin[t] = vigo::fit_mixed_bin(K, status, Ns, stride);
                if (bin[t] < -1 || bin[t] >= vigo::kFitBins) return 2;
                if (bin[t] >= 0) ++cnt[bin[t]];
            }
            std::vector<int> pp(vigo::kFitBins + 1), gp(vigo::kFitBins + 1);
            vigo::fit_plan_prefix(cnt.data(), pp.data(), gp.data());
            std::vector<int> sorted((size_t)pp[vigo::kFitBins], -1), next(pp.begin(), pp.end() - 1);
            for (int t = 0; t < T; ++t)
                if (bin[t] >= 0) sorted[next[bin[t]]++] = t;
            printf("%lld %d |", vigo::fit_mixed_max_groups(T), gp[vigo::kFitBins]);
            for (int t = 0; t < T; ++t) printf(" %d", bin[t]);
            printf(" |");
            for (int g = 0; g < gp[vigo::kFitBins]; ++g) {
                const vigo::FitGroup fg = vigo::fit_group_of(pp.data(), gp.data(), g);
                printf("%s%d %d %d", g ? " ; " : " ", fg.K, fg.first, fg.members);
                for (int i = 0; i < fg.members; ++i) printf(" %d", sorted.at((size_t)fg.first + i));
            }
            // beyond the last group: nothing
            const vigo::FitGroup none = vigo::fit_group_of(pp.data(), gp.data(), gp[vigo::kFitBins]);
            if (none.K != 0 || none.members != 0) return 3;
        } else if (q[0] == 'G') {
            int g;
            std::vector<int> cnt(vigo::kFitBins), pp(vigo::kFitBins + 1), gp(vigo::kFitBins + 1);
            if (scanf("%d", &g) != 1) return 1;
            for (int k = 0; k < vigo::kFitBins; ++k)
                if (scanf("%d", &cnt[k]) != 1) return 1;
            vigo::fit_plan_prefix(cnt.data(), pp.data(), gp.data());
            const vigo::FitGroup fg = vigo::fit_group_of(pp.data(), gp.data(), g);
            printf("%d %d %d", fg.K, fg.first, fg.members);
        } else {
            fprintf(stderr, "bad query: %s\n", q);
            return 1;
        }
        printf("\n");
    }
    return 0;
}
