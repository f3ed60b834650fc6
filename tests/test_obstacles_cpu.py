"""CPU tests of the scripted obstacles (mpc_obstacles_select, mpc_discs_from_obstacles / mpc_fields_from_obstacles,
mpc_closed_loop_obstacles): the numpy restatement of tests/obstacles_common.py on hand-made cases, the generator of the GPU
test's selection cases against the counts that test asserts, _lib.obstacle_tracks, the invariants of the recorded mirror
loop (tests/golden/obstacles_reference.npz) and the refusals the library makes before it needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import discs_common as D
import obstacles_common as OC
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


def discs(*tracks):
    """obs [1, K, Lt, 3] of one scene from K lists of (cx, cy, r)"""
    return np.array([tracks], dtype=np.float64)


# ----------------------------------------------------------------------------- the restatement
def test_sample_index_clamps_and_wraps():
    assert [OC.sample_index(i, 1, False) for i in (0, 1, 9)] == [0, 0, 0]
    assert [OC.sample_index(i, 1, True) for i in (0, 1, 9)] == [0, 0, 0]
    assert [OC.sample_index(i, 4, False) for i in (0, 2, 3, 4, 100)] == [0, 2, 3, 3, 3]
    assert [OC.sample_index(i, 4, True) for i in (0, 2, 3, 4, 5, 103)] == [0, 2, 3, 0, 1, 3]
    assert OC.sample_index(2 ** 31 - 1, 7, True) == (2 ** 31 - 1) % 7


def test_the_window_clamps_across_the_end_and_wraps():
    # one agent standing at the origin, one obstacle walking away along x: sample i at x = 1 + i, Lt = 3
    X = np.zeros((1, 4, 4))
    obs = discs([(1, 0, 0.5), (2, 0, 0.5), (3, 0, 0.5)])
    # ti = 1: samples 1, 2, 2, 2 (clamped) -> nearest is sample 1 at d^2 = 4
    sel, clear, _ = OC.select_obstacles(X, 1, obs, ti=1)
    assert sel.tolist() == [[0, -1]] and clear[0, 0] == 4.0 - 0.25
    # wholly behind the end: the obstacle stands at its last sample
    assert OC.select_obstacles(X, 1, obs, ti=50)[1][0, 0] == 9.0 - 0.25
    # periodic: ti = 2 -> samples 2, 0, 1, 2: the nearest is sample 0
    assert OC.select_obstacles(X, 1, obs, ti=2, wrap=True)[1][0, 0] == 1.0 - 0.25
    # Lt = 1: whatever ti and wrap are, the one sample
    one = discs([(2, 0, 1.0)])
    for ti, wrap in ((0, False), (7, False), (7, True)):
        assert OC.select_obstacles(X, 1, one, ti=ti, wrap=wrap)[1][0, 0] == 3.0
    rows = OC.gather_rows(np.array([[0, -1]], dtype=np.int32), 1, obs, 1, 4)
    assert rows[0, :, 0, 0].tolist() == [2.0, 3.0, 3.0, 3.0] and not rows[0, :, 1].any()
    rows = OC.gather_rows(np.array([[0, 0]], dtype=np.int32), 1, obs, 2, 4, wrap=True)
    assert rows[0, :, 1, 0].tolist() == [3.0, 1.0, 2.0, 3.0]


def test_absent_samples_are_skipped_and_an_obstacle_absent_in_the_whole_window_is_no_candidate():
    X = np.zeros((1, 3, 4))
    # obstacle 0: nearest where it is absent (junk behind r == 0, a NaN among it); obstacle 1: absent in the whole window
    # but present later; obstacle 2: present, far
    obs = discs([(0.1, 0, 0.0), (np.nan, 0, 0.0), (2, 0, 0.5), (0, 0, 0.5)],
                [(0, 0, 0.0), (0, 0, 0.0), (0, 0, 0.0), (0.5, 0, 0.1)],
                [(5, 0, 1.0), (5, 0, 1.0), (5, 0, 1.0), (5, 0, 1.0)])
    sel, clear, info = OC.select_obstacles(X, 1, obs, ti=0)
    assert sel.tolist() == [[0, 2]] and clear[0].tolist() == [4.0 - 0.25, 24.0]
    assert info["absent"] == 2 and info["empty"] == 1 and info["nonfinite"] == 0
    # with reach = +inf an empty window is still no candidate
    assert OC.select_obstacles(X, 1, obs[:, 1:2], ti=0)[0].tolist() == [[-1, -1]]
    # the gather writes zeros for the absent samples: nothing behind r == 0 is copied
    rows = OC.gather_rows(sel, 1, obs, 0, 3)
    assert not rows[0, :2, 0].any() and rows[0, 2, 0].tolist() == [2.0, 0.0, 0.5] and not np.isnan(rows).any()
    # a source is absent iff A == 0
    src = np.zeros((1, 1, 2, 8))
    src[0, 0, 0] = (1, 0, 1, 0, 0.0, 3, 3, 0)
    src[0, 0, 1] = (2, 0, 1, 0, 0.4, 3, 3, 0)
    sel, clear, info = OC.select_obstacles(np.zeros((1, 2, 6)), 1, src, ti=0)
    assert sel.tolist() == [[0, -1]] and clear[0, 0] == 4.0 and info["absent"] == 1      # r2 = 0: c = d^2
    rows = OC.gather_rows(sel, 1, src, 0, 2)
    assert not rows[0, 0].any() and np.array_equal(rows[0, 1, 0], src[0, 0, 1])


def test_ties_go_to_the_smaller_index_and_reach_cuts():
    X = states([(0, 0)])
    obs = discs([(0, 1, 0.2)], [(1, 0, 0.2)], [(-1, 0, 0.2)], [(3, 0, 0.2)])
    sel, clear, info = OC.select_obstacles(X, 1, obs)
    assert sel.tolist() == [[0, 1]] and clear[0, 0] == clear[0, 1] and info["ties"] == 2
    # c == reach^2 is no candidate (strict)
    far = discs([(2, 0, 0.0 + 1e-300)], [(1, 0, 1e-300)])
    assert OC.select_obstacles(X, 1, far, reach=2.0)[0].tolist() == [[1, -1]]
    sel, _, info = OC.select_obstacles(X, 1, obs, reach=0.5)
    assert sel.tolist() == [[-1, -1]] and info["short"] == 1
    # scenes do not mix: agent 1 (scene 1) never sees scene 0's obstacle
    two = np.concatenate([discs([(0, 0, 0.5)]), discs([(9, 9, 0.5)])])
    sel, clear, _ = OC.select_obstacles(states([(0, 0), (0, 0)]), 1, two)
    assert sel.tolist() == [[0, -1], [0, -1]] and clear[0, 0] == -0.25 and clear[1, 0] == 162.0 - 0.25


def test_a_non_finite_sample_takes_one_pair_out_and_no_other():
    X = np.zeros((2, 3, 4))
    X[1, :, 0] = 1.0
    obs = discs([(2, 0, 0.5), (np.inf, 0, 0.5), (2, 0, 0.5)], [(3, 0, 0.5)] * 3)
    sel, _, info = OC.select_obstacles(X, 2, obs)
    assert sel.tolist() == [[1, -1], [1, -1]] and info["nonfinite"] == 2
    # an agent's non-finite stage takes out its own pairs alone
    obs = discs([(2, 0, 0.5)] * 3, [(3, 0, 0.5)] * 3)
    X[0, 1, 1] = np.nan
    sel, _, info = OC.select_obstacles(X, 2, obs)
    assert sel.tolist() == [[-1, -1], [0, 1]] and info["nonfinite"] == 2
    # a NaN radius is present, and takes the pair out
    obs[0, 0, 2, 2] = np.nan
    assert OC.select_obstacles(X, 2, obs)[0].tolist() == [[-1, -1], [1, -1]]


def test_the_disc_key_is_the_disc_constraint_bit_for_bit():
    rng = np.random.default_rng(5)
    B, G, K, N, Lt = 12, 4, 5, 7, 9
    X = rng.normal(size=(B, N, 6))
    obs = rng.normal(size=(B // G, K, Lt, 3))
    obs[..., 2] = rng.uniform(0.05, 0.5, obs.shape[:3])
    for ti, wrap in ((0, False), (5, False), (6, True)):
        sel, clear, _ = OC.select_obstacles(X, G, obs, ti, wrap=wrap)
        rows = OC.gather_rows(sel, G, obs, ti, N, wrap)
        for b in range(B):
            g = D.disc_g(X[b], rows[b])[0].reshape(N, 2)
            assert np.array_equal(g.min(0), clear[b])                   # the same expression


@pytest.mark.parametrize("nx,W", [(4, 3), (6, 8)])
@pytest.mark.parametrize("Nst", OC.SELECTION_STAGES)
def test_the_selection_cases_hold_what_the_gpu_test_asserts(nx, W, Nst):
    tot = dict(ties=0, short=0, nonfinite=0, absent=0)
    for which, (G, K, B) in enumerate(OC.SELECTION_SHAPES):
        X, obs, ti, wrap = OC.selection_case(nx, W, Nst, G, K, B, which)
        assert obs.shape[:2] == (B // G, K) and obs.shape[3] == W
        sel, clear, info = OC.select_obstacles(X, G, obs, ti, OC.SELECTION_REACH, wrap)
        for k in tot:
            tot[k] += info[k]
        on = sel >= 0
        assert sel.max() < K
        assert np.isfinite(clear[on]).all() and np.isinf(clear[~on]).all() and (clear[on] < OC.SELECTION_REACH ** 2).all()
        assert (clear[:, 0] <= clear[:, 1]).all()
    assert tot["ties"] >= 20 and tot["short"] >= 20 and tot["nonfinite"] >= 5, tot
    # (a window of one stage whose sample is absent makes its obstacle no candidate: nothing to count at Nst = 1)
    assert tot["absent"] >= 20 or Nst == 1, tot


def test_the_windows_of_the_selection_cases_clamp_wrap_and_lie_behind_the_end():
    for Nst in OC.SELECTION_STAGES:
        w = [OC.selection_window(Nst, i) for i in range(5)]
        assert w[0][0] == 1 and w[0][1] > 0
        Lt, ti, wrap = w[1]
        assert not wrap and (Nst == 1 or ti < Lt - 1 < ti + Nst - 1)          # clamps across Lt - 1
        Lt, ti, wrap = w[2]
        assert wrap and (Nst == 1 or ti + Nst - 1 >= Lt > ti)                 # wraps
        Lt, ti, wrap = w[3]
        assert not wrap and ti >= Lt                                          # wholly behind the end


# ----------------------------------------------------------------------------- the host builder
def test_obstacle_tracks_builds_and_refuses_each_bad_row():
    dcfg = mp.default_config(0, 20, constr_mode=mp.CONSTR_DISCS)
    fcfg = mp.default_config(1, 12, constr_mode=mp.CONSTR_LANE)
    assert _lib.obstacle_width(dcfg) == 3 and _lib.obstacle_width(fcfg) == _lib.NFSRC
    centres = np.arange(2 * 3 * 5 * 2, dtype=np.float64).reshape(2, 3, 5, 2)
    tab = _lib.obstacle_tracks(dcfg, centres=centres, radii=0.2)
    assert tab.shape == (2, 3, 5, 3) and tab.flags.c_contiguous and np.array_equal(tab[..., :2], centres) and (tab[..., 2] == 0.2).all()
    r = np.full((2, 3, 5), 0.1)
    r[0, 1, :2] = 0.0
    assert np.array_equal(_lib.obstacle_tracks(dcfg, centres=centres, radii=r)[..., 2], r)
    for kw in (dict(centres=centres, radii=-0.1), dict(centres=centres, radii=np.nan), dict(centres=np.full_like(centres, np.inf), radii=0.1),
               dict(centres=centres[0], radii=0.1), dict(centres=centres, radii=np.zeros(4)), dict(centres=centres),
               dict(sources=np.zeros((2, 3, 5, 8))), dict(centres=np.zeros((1, 65, 2, 2)), radii=0.1),
               dict(centres=np.zeros((1, 2, 0, 2)), radii=0.1)):
        with pytest.raises(ValueError, match="obstacle_tracks"):
            _lib.obstacle_tracks(dcfg, **kw)
    src = np.zeros((2, 3, 5, 8))
    src[...] = (1.0, 0.5, 1.0, 0.0, 0.3, 20.0, 20.0, 0.1)
    src[1, 2, 3, 4] = 0.0
    tab = _lib.obstacle_tracks(fcfg, sources=src)
    assert np.array_equal(tab, src) and tab is not src
    for col, val in ((0, np.nan), (7, np.inf), (4, -0.1), (5, -1.0), (6, -1.0)):
        bad = src.copy()
        bad[0, 1, 2, col] = val
        with pytest.raises(ValueError, match="obstacle_tracks"):
            _lib.obstacle_tracks(fcfg, sources=bad)
    bad = src.copy()
    bad[0, 0, 0, 5] = 0.0                                   # a skew without kx > 0
    with pytest.raises(ValueError, match="a skew"):
        _lib.obstacle_tracks(fcfg, sources=bad)
    for kw in (dict(centres=centres, radii=0.1), dict(sources=src[..., :3]), dict(sources=src[0]), dict()):
        with pytest.raises(ValueError, match="obstacle_tracks"):
            _lib.obstacle_tracks(fcfg, **kw)
    # the rules are the setters': what obstacle_tracks lets through, as a table row, mpc_set_agent_discs would bind
    assert OC.gather_rows(np.zeros((2, 2), dtype=np.int32), 1, _lib.obstacle_tracks(dcfg, centres=centres, radii=r), 0, 20).shape == (2, 20, 2, 3)


# ----------------------------------------------------------------------------- the recorded mirror loop
def reference():
    return np.load(os.path.join(GOLDEN, "obstacles_reference.npz"))


def test_the_recorded_mirror_loop():
    ref = reference()
    ns = ref["X0"].shape[0]
    X0, v_ref, obs = OC.script_scenes(ns)
    assert np.array_equal(ref["shifts"], D.scene_shifts()) and np.array_equal(ref["X0"], X0)
    assert np.array_equal(ref["v_ref"], v_ref) and np.array_equal(ref["obs"], obs)
    T = ref["traj_x"].shape[1]
    assert ns == 16 and T == 14 and ref["margin"].shape == (ns, T) and obs.shape == (ns, 3, OC.SCRIPT_LT, 3)
    assert T + OC.SCRIPT_N < OC.SCRIPT_LT                                 # the recording never reads the clamped end
    assert ref["margin"].min() >= OC.MARGIN_MIN
    tx, tsel, tclear = ref["traj_x"], ref["traj_sel"], ref["traj_clear"]
    # the three obstacles: a slower one ahead 0.03 beside the line, one crossing the line, one that appears at sample 6
    assert np.allclose(obs[0, 0, :, 1], 0.53) and (obs[0, 0, :, 2] == 0.14).all() and obs[0, 0, 0, 0] > X0[0, 0]
    assert obs[0, 1, 0, 1] > 0.5 > obs[0, 1, -1, 1]
    assert (obs[:, 2, :OC.SCRIPT_APPEARS, 2] == 0).all() and (obs[:, 2, OC.SCRIPT_APPEARS:, 2] > 0).all()
    for s in range(ns):
        assert (tsel[s, :, 0] >= 0).all() and (tsel[s] == 0).any(1).all()          # the slow one is avoided at every step
        assert tsel[s, 0].tolist() == [0, 1] and (tsel[s, 1:] == [0, 2]).all()   # the selection changes: the crossing one leaves
        slow_end = obs[s, 0, T, 0]
        assert tx[s, 0, 0] < obs[s, 0, 1, 0] and tx[s, -1, 0] > slow_end            # the car ends ahead of the slow one ...
        assert tx[s, :, 1].min() < obs[s, 0, 0, 1] - 0.08                           # ... having passed below it
    assert (tsel[:, 1] == 2).any()     # the third obstacle is selected at step 1 (ti = 2), its samples 2 .. 5 being absent
    # traj_clear is the restated selection on the recorded states at the script's time; nobody touched beyond 1e-8
    for t in range(T):
        assert np.array_equal(OC.select_obstacles(tx[:, t], 1, obs, t + 1)[1][:, 0], tclear[:, t])
    assert tclear.min() >= -1e-6 and tclear.min() <= 1e-3


def test_the_generator_reproduces_the_recording(O):
    """the inputs bit for bit (above) and, through the mirror loop, the first step of scene 0: one reference solve.  Two
    runs of scipy's L-BFGS-B on different BLAS builds agree to the solve's own 1e-8, not to the bit."""
    ref = reference()
    X0, v_ref, obs = OC.script_scenes(16)
    res = OC.mirror_loop(O, 0, OC.SCRIPT_N, X0[:1], v_ref[:1], obs[:1], OC.SCRIPT_REACH, 1, 1, D.line_centerline())
    assert np.array_equal(res["traj_sel"][0], ref["traj_sel"][0, :1])
    assert np.abs(res["traj_u"][0] - ref["traj_u"][0, :1]).max() < 1e-7
    assert np.abs(res["traj_x"][0] - ref["traj_x"][0, :1]).max() < 1e-8
    assert abs(res["margin"][0] - ref["margin"][0, 0]) < 1e-7


# ----------------------------------------------------------------------------- the C ABI without a device
NEW = ("mpc_obstacles_select", "mpc_discs_from_obstacles", "mpc_fields_from_obstacles", "mpc_closed_loop_obstacles")


def test_prototypes_agree_with_the_header(L):
    """every parameter of the four declarations against the ctypes argtypes: int, double, pointer"""
    hdr = open(os.path.join(ROOT, "include", "mpc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTS
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, name
        want = []
        for par in m.group(1).split(","):
            par = " ".join(par.split())
            want.append(C.c_double if par.startswith("double ") and "*" not in par else
                        C.c_int if par.startswith("int ") and "*" not in par else "ptr")
        got = [a if a in (C.c_double, C.c_int) else "ptr" for a in getattr(L, name).argtypes]
        assert got == want, name
        assert getattr(L, name).restype is C.c_int
    assert os.path.exists(os.path.join(os.path.dirname(_lib._SRC[0]), "mpc_obstacles.hpp"))
    assert any(os.path.basename(p) == "mpc_obstacles.hpp" for p in _lib._SRC)
    assert mp.ObstacleLoopResult._fields == ("x", "U", "lam", "traj_x", "traj_u", "failures", "stats", "traj_sel", "traj_clear",
                                             "table", "cl_index")


def test_refusals_that_need_no_device(L):
    """MPC_E_ARG (-1) with a message that names the call and the argument, before the handle is looked at"""
    one = C.c_void_p(8)            # any non-null address: refused calls read no buffer
    big = 2 ** 31 - 1

    def select(B=6, G=3, K=2, Lt=5, ti=0, Nst=1, X=one, obs=one, reach=INF, sel=one):
        return L.mpc_obstacles_select(None, B, G, K, Lt, 0, ti, Nst, X, obs, reach, sel, None, None)

    def loop(B=6, T=1, G=3, K=2, Lt=5, t0=0, obs=one, reach=INF):
        return L.mpc_closed_loop_obstacles(None, B, T, 0, G, K, Lt, 0, t0, obs, reach, one, one, None, one, one, one, None, None,
                                           None, None, None, None, None, None)

    def gather(fn):
        def call(B=6, G=3, K=2, Lt=5, ti=0, obs=one):
            return fn(None, B, G, K, Lt, 0, ti, obs, one, one, None)
        return call
    shared = ((dict(G=0), b"scene size G"), (dict(G=65), b"scene size G"), (dict(K=0), b"obstacles K"), (dict(K=65), b"obstacles K"),
              (dict(B=7), b"B % G"), (dict(G=4), b"B % G"), (dict(Lt=0), b"Lt must be >= 1"), (dict(obs=None), b"null obs"))
    for fn, who, tname, extra in ((select, b"mpc_obstacles_select", "ti", True), (loop, b"mpc_closed_loop_obstacles", "t0", True),
                                  (gather(L.mpc_discs_from_obstacles), b"mpc_discs_from_obstacles", "ti", False),
                                  (gather(L.mpc_fields_from_obstacles), b"mpc_fields_from_obstacles", "ti", False)):
        cases = list(shared) + [({tname: -1}, tname.encode() + b" must be >= 0"), (dict(), b"null handle")]
        if extra:
            cases += [(dict(reach=-1e-300), b"reach must be >= 0"), (dict(reach=float("nan")), b"reach must be >= 0")]
        if fn is not loop and extra:
            cases += [({tname: big}, b"does not fit an int32")]
        for kw, words in cases:
            assert fn(**kw) == -1, (who, kw)
            msg = L.mpc_last_error()
            assert msg.startswith(who + b": ") and words in msg, msg
    for kw, words in ((dict(Nst=0), b"Nst must be >= 1"), (dict(Nst=-3), b"Nst must be >= 1"), (dict(X=None), b"null X or sel"),
                      (dict(sel=None), b"null X or sel"), (dict(ti=big - 3, Nst=4), b"does not fit an int32")):
        assert select(**kw) == -1, kw
        assert words in L.mpc_last_error()
    assert select(ti=big - 4, Nst=4) == -1 and b"null handle" in L.mpc_last_error()      # the last window that fits
    assert loop(T=-1) == -1 and b"negative T" in L.mpc_last_error()
