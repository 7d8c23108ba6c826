"""-m "not gpu": the cases of tests/test_gpu_solver_axis_first_trial.py on the CPU, oracle alone — every variant shows
the exit it is there for and (where its name allows one) a first trial that is rejected and goes on, except the pairs
listed in VACUOUS, which show the opposite; and no shape has more than one vacuous variant in ten."""
import pytest

import test_gpu_solver_axis_first_trial as F
import test_gpu_solver_axis_warmup as W


@pytest.mark.parametrize("N", F.SIZES)
def test_variants_show_their_exit_and_a_rejected_first_trial(small_world, N):
    for name in F.VARIANTS:
        P, b = F.case(small_world, name, N)
        F.oracle_says(name, N, W.oracle(P, b))
    assert 10 * sum(1 for name, n in F.VACUOUS if n == N) <= len(F.VARIANTS)


def test_the_table_of_vacuous_cases_names_cases():
    assert all(name in F.VARIANTS and n in F.SIZES for name, n in F.VACUOUS)
