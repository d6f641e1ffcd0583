"""CPU: the likelihood-association query's C-ABI surface, `frontend.resolve_associations` on hand-made cases, and a dense
NumPy unlabelled EKF loop on the oracle that recovers the true labels of the separable grid worlds (no device)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import assoc_world as aw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_association_query_and_the_binding_types_it():
    text = open(os.path.join(ROOT, "include", "ekfslam_hip.h")).read()
    decl = re.search(r"int\s+ekf_associate\s*\(([^)]*)\)\s*;", text)
    assert decl, "ekf_associate is not declared in include/ekfslam_hip.h"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["ekf_handle *h", "int b0", "int count", "const double *range", "const double *bearing", "const int *m",
                      "int stride", "int *cand", "double *cand_nis", "double *cand_logdet", "double *min_nis",
                      "double *all_nis", "double *all_logdet", "int cap"]
    from slam_duckietown_amd import ekf_bindings as eb
    res, args = eb.ABI["ekf_associate"]
    assert res is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_int, eb._dp, eb._dp, eb._ip, C.c_int, eb._ip, eb._dp, eb._dp, eb._dp, eb._dp,
                    eb._dp, C.c_int]
    makefile = open(os.path.join(ROOT, "slam-duckietown_amd", "csrc", "Makefile")).read()
    assert "ekf_associate.hip" in makefile


def resolve(*a):
    from slam_duckietown_amd.frontend import resolve_associations
    assign, new, dropped = resolve_associations(*a)
    return list(assign), list(new), list(dropped)


def test_resolve_plain_and_conflict_goes_to_the_second_candidate():
    # observations 0 and 1 both prefer landmark 4; observation 1 fits it better and is taken first; 0 falls to landmark 7
    cand = [[4, 7], [4, 2]]
    nis = [[1.5, 3.0], [0.5, 30.0]]
    assert resolve(cand, nis, [1.5, 0.5], 9.21, 18.42) == ([7, 4], [], [])
    # the second candidate too far: dropped (it still fits landmark 4 well: no new landmark)
    nis = [[1.5, 12.0], [0.5, 30.0]]
    assert resolve(cand, nis, [1.5, 0.5], 9.21, 18.42) == ([-1, 4], [], [0])


def test_resolve_both_candidates_taken_means_dropped():
    cand = [[1, 2], [1, 2], [1, 2]]
    nis = [[0.1, 5.0], [0.2, 0.3], [0.4, 0.5]]
    assert resolve(cand, nis, [0.1, 0.2, 0.4], 9.21, 18.42) == ([1, 2, -1], [], [2])


def test_resolve_thresholds():
    cand = [[0, 1], [2, 3], [4, 5], [6, 7]]
    nis = [[9.21, 50.0], [9.22, 50.0], [18.42, 50.0], [18.43, 50.0]]
    mn = [9.21, 9.22, 18.42, 18.43]
    # NIS <= accept is accepted; above it and min_nis <= create is ambiguous; min_nis > create is a new landmark
    assert resolve(cand, nis, mn, 9.21, 18.42) == ([0, -1, -1, -1], [3], [1, 2])
    # min_nis decides creation, not the candidate's NIS: the best d need not be the best NIS
    assert resolve([[0, 1]], [[40.0, 45.0]], [12.0], 9.21, 18.42) == ([-1], [], [0])
    # stable order: equal best NIS, the earlier observation goes first
    assert resolve([[3, -1], [3, -1]], [[1.0, np.nan], [1.0, np.nan]], [1.0, 1.0], 9.21, 18.42) == ([3, -1], [], [1])


def test_resolve_empty_map_and_no_observations():
    nan = np.nan
    assert resolve([[-1, -1], [-1, -1]], [[nan, nan], [nan, nan]], [nan, nan], 9.21, 18.42) == ([-1, -1], [0, 1], [])
    assert resolve(np.zeros((0, 2), dtype=int), np.zeros((0, 2)), np.zeros(0), 9.21, 18.42) == ([], [], [])
    # a single landmark: the second candidate is -1
    assert resolve([[0, -1], [0, -1]], [[0.3, nan], [25.0, nan]], [0.3, 25.0], 9.21, 18.42) == ([0, -1], [1], [])


@pytest.mark.parametrize("seed", aw.SEEDS)
@pytest.mark.parametrize("name", list(aw.WORLDS))
def test_dense_unlabelled_loop_recovers_the_true_labels(name, seed):
    from slam_duckietown_amd.frontend import resolve_associations
    r = aw.dense_unlabelled_run(name, seed, resolve_associations)
    print(f"{name} seed {seed}: wrong {r['wrong']} dropped {r['dropped']} created {r['created'].tolist()} "
          f"smallest runner-up margin {r['margin']:.1f}")
    assert r["wrong"] == 0
    assert r["dropped"] == 0
    assert (r["created"] == 1).all()
    assert r["margin"] >= 32.0
