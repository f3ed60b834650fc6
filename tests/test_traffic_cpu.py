"""CPU tests of the traffic selection and loop (mpc_opponents_from_plans, mpc_closed_loop_traffic): the numpy restatement of
tests/traffic_common.py on hand-made cases, the generator of the GPU test's selection cases against the counts that test
asserts, the invariants of the recorded mirror loop (tests/golden/traffic_reference.npz), and the refusals the library
makes before it needs a device."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import discs_common as D
import traffic_common as TC
import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib

INF = np.inf


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def states(xy, nx=4):
    X = np.zeros((len(xy), nx))
    X[:, :2] = xy
    return X


# ----------------------------------------------------------------------------- the restatement
def test_exact_ties_go_to_the_smaller_index():
    # agent 0 in the middle of four agents at distance 1 (c = 1 each): slots 0 and 1 are agents 1 and 2
    X = states([(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1)])
    opp, clear, info = TC.select_opponents(X, 5, np.zeros(5))
    assert opp[0].tolist() == [1, 2] and clear[0].tolist() == [1.0, 1.0]
    assert info["ties"] >= 2 and info["short"] == 0
    # agent 1: itself excluded; 0 at c = 1, then 2 and 4 tie at c = 2
    assert opp[1].tolist() == [0, 2] and clear[1].tolist() == [1.0, 2.0]
    # a larger radius of a farther agent wins: c = d^2 - r_o^2 is what is compared, and it may be negative
    r = np.array([0.0, 0.0, 0.0, 1.5, 0.0])
    opp, clear, _ = TC.select_opponents(X, 5, r)
    assert opp[0].tolist() == [3, 1] and clear[0].tolist() == [1.0 - 2.25, 1.0]


def test_reach_cuts_candidates_and_scenes_do_not_mix():
    X = states([(0, 0), (1, 0), (3, 0), (0.1, 0), (0.2, 0), (9, 9)])
    r = np.zeros(6)
    opp, clear, info = TC.select_opponents(X, 3, r, reach=2.0)       # c < 4
    assert opp.tolist() == [[1, -1], [0, -1], [-1, -1], [4, -1], [3, -1], [-1, -1]]
    assert clear[0].tolist() == [1.0, INF] and np.isinf(clear[2]).all()
    assert info["short"] == 6
    # c == reach^2 is no candidate (strict); reach = 0 still admits a negative c
    assert TC.select_opponents(states([(0, 0), (2, 0)]), 2, np.zeros(2), reach=2.0)[0].tolist() == [[-1, -1], [-1, -1]]
    assert TC.select_opponents(states([(0, 0), (2, 0)]), 2, np.full(2, 2.5), reach=0.0)[0].tolist() == [[1, -1], [0, -1]]
    # all: agents 3, 4 never appear for 0 .. 2
    opp, _, _ = TC.select_opponents(X, 3, r)
    assert opp[:3].max() <= 2 and opp[3:].min() >= 3


def test_a_non_finite_stage_takes_the_pair_out_and_nothing_else():
    X = np.zeros((3, 4, 4))
    X[0, :, 0], X[1, :, 0], X[2, :, 0] = 0.0, 1.0, 2.0
    X[1, 2, 1] = np.nan
    opp, clear, info = TC.select_opponents(X, 3, np.zeros(3))
    assert opp.tolist() == [[2, -1], [-1, -1], [0, -1]] and info["nonfinite"] == 4
    X[1, 2, 1] = np.inf
    assert TC.select_opponents(X, 3, np.zeros(3))[0].tolist() == [[2, -1], [-1, -1], [0, -1]]
    # the minimum is over the stages
    X[1, 2, 1] = 0.0
    X[1, 3, 0] = 0.25
    opp, clear, _ = TC.select_opponents(X, 3, np.zeros(3))
    assert opp[0].tolist() == [1, 2] and clear[0].tolist() == [0.0625, 4.0]


def test_a_scene_of_one_has_nobody():
    opp, clear, info = TC.select_opponents(states([(0, 0), (0, 0), (1, 1)]), 1, np.ones(3))
    assert (opp == -1).all() and np.isinf(clear).all() and info["short"] == 3 and info["ties"] == 0


def test_clear_is_the_smallest_disc_constraint_of_the_gathered_table():
    rng = np.random.default_rng(5)
    B, G, N = 12, 4, 7
    X = rng.normal(size=(B, N, 6))
    radius = rng.uniform(0, 0.5, B)
    opp, clear, _ = TC.select_opponents(X, G, radius)
    discs = TC.gather_discs(X, opp, radius)
    for b in range(B):
        g = D.disc_g(X[b], discs[b])[0].reshape(N, 2)
        assert np.array_equal(g.min(0), clear[b])                   # bit for bit: the same expression


@pytest.mark.parametrize("nx", [4, 6])
@pytest.mark.parametrize("Nst", TC.SELECTION_STAGES)
def test_the_selection_cases_hold_what_the_gpu_test_asserts(nx, Nst):
    tot = dict(ties=0, short=0, nonfinite=0)
    for G, B in TC.SELECTION_SHAPES:
        X, radius = TC.selection_case(nx, Nst, G, B)
        opp, clear, info = TC.select_opponents(X, G, radius, TC.SELECTION_REACH)
        for k in tot:
            tot[k] += info[k]
        on = opp >= 0
        assert (opp[on] // G == (np.arange(B)[:, None] // G * np.ones((1, 2), int))[on]).all()
        assert (opp != np.arange(B)[:, None]).all()
        assert np.isfinite(clear[on]).all() and np.isinf(clear[~on]).all() and (clear[on] < TC.SELECTION_REACH ** 2).all()
        assert (clear[:, 0] <= clear[:, 1]).all()
    assert tot["ties"] >= 20 and tot["short"] >= 20 and tot["nonfinite"] >= 5, tot


# ----------------------------------------------------------------------------- the recorded mirror loop
def test_the_recorded_mirror_loop():
    ref = np.load(os.path.join(GOLDEN, "traffic_reference.npz"))
    ns = ref["X0"].shape[0] // 3
    X0, v_ref, radius = TC.overtake_scenes(ns)
    assert np.array_equal(ref["shifts"], D.scene_shifts()) and np.array_equal(ref["X0"], X0)
    assert np.array_equal(ref["v_ref"], v_ref) and np.array_equal(ref["radius"], radius)
    T = ref["traj_x"].shape[1]
    assert ns == 16 and T == 14 and ref["margin"].shape == (ns, T)
    assert ref["margin"].min() >= TC.MARGIN_MIN
    tx, topp, tclear = ref["traj_x"], ref["traj_opp"], ref["traj_clear"]
    for s in range(ns):
        a, b, c = 3 * s, 3 * s + 1, 3 * s + 2
        assert not (topp[[a, b]] == c).any() and (topp[c] == -1).all()          # the third car is never selected
        assert (topp[a, :8, 0] == b).all() and (topp[b, :8, 0] == a).all()      # the two see each other from the start
        assert tx[a, 0, 0] < tx[b, 0, 0] and tx[a, -1, 0] > tx[b, -1, 0]        # the follower ends ahead ...
        assert tx[a, :, 1].min() < tx[b, :, 1].min() - 0.08                     # ... having passed below the slow car
    # traj_clear is the restated selection on the recorded states; nobody touched beyond the reference solve's 1e-8
    for t in range(T):
        assert np.array_equal(TC.select_opponents(tx[:, t], 3, radius)[1][:, 0], tclear[:, t])
    assert tclear.min() >= -1e-6 and tclear.min() <= 1e-3
    # selection of step 0 from the plans of U = 0 (cars coasting): derivable without a solve
    assert (topp[:, 0].reshape(ns, 3, 2)[:, 0, 0] == 3 * np.arange(ns) + 1).all()


# ----------------------------------------------------------------------------- the C ABI without a device
def test_header_constants_exports_and_mirror_agree():
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    assert "#define MPC_SCENE_MAX 64" in hdr
    assert (mp.SCENE_MAX, _lib.SCENE_MAX, TC.SCENE_MAX) == (64, 64, 64)
    for name in ("mpc_opponents_from_plans", "mpc_closed_loop_traffic"):
        assert name in _lib.EXPORTS and name in hdr
    assert os.path.basename(_lib._SRC[-1]) == "mpc_traffic.hpp" and os.path.exists(_lib._SRC[-1])


def test_refusals_that_need_no_device(L):
    """MPC_E_ARG (-1) with a message, before the handle is looked at: a null handle gets this far"""
    one = C.c_void_p(8)            # any non-null address: refused calls read no buffer
    inf = float("inf")

    def opponents(B=6, G=3, Nst=1, X=one, radius=one, reach=inf, opp=one):
        return L.mpc_opponents_from_plans(None, B, G, Nst, X, radius, reach, opp, None, None)

    def loop(B=6, T=1, G=3, radius=one, reach=inf):
        return L.mpc_closed_loop_traffic(None, B, T, 0, G, radius, reach, one, one, None, one, one, one, None, None, None,
                                         None, None, None, None)
    for fn, who in ((opponents, b"mpc_opponents_from_plans"), (loop, b"mpc_closed_loop_traffic")):
        for kw, words in ((dict(G=0), b"scene size G"), (dict(G=65), b"scene size G"), (dict(G=-1), b"scene size G"),
                          (dict(B=7), b"B % G"), (dict(G=4), b"B % G"), (dict(reach=-1e-300), b"reach must be >= 0"),
                          (dict(reach=float("nan")), b"reach must be >= 0"), (dict(radius=None), b"null radius"),
                          (dict(), b"null handle")):
            assert fn(**kw) == -1, kw
            msg = L.mpc_last_error()
            assert msg.startswith(who + b": ") and words in msg, msg
    for kw, words in ((dict(Nst=0), b"Nst must be >= 1"), (dict(Nst=-3), b"Nst must be >= 1"), (dict(X=None), b"null X or opp"),
                      (dict(opp=None), b"null X or opp")):
        assert opponents(**kw) == -1, kw
        assert words in L.mpc_last_error()
    assert loop(T=-1) == -1 and b"negative T" in L.mpc_last_error()
