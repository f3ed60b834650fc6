"""CPU tests of event-triggered holding in traffic (mpc_opponent_trigger, mpc_closed_loop_traffic_event): the numpy
restatement of tests/traffic_event_common.py on hand-made cases -- the held window against the full selection, its end at
the kernel's chunk edge, whose count it is, set membership --, the mirror loop's own logic on a stand-in solver, the
invariants of the recorded mirror loop (tests/golden/traffic_event_reference.npz), the prototypes against the header and
the refusals the library makes before it needs a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import discs_common as D
import traffic_common as TC
import traffic_event_common as TE
import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib

INF = np.inf


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def lanes(B, N, nx=4):
    """X [B, N, nx]: agent b walks along x on the line y = b, at (j + 1, b) at stage j"""
    X = np.zeros((B, N, nx))
    X[:, :, 0] = (np.arange(N) + 1.0)[None, :]
    X[:, :, 1] = np.arange(B)[:, None]
    return X


# ----------------------------------------------------------------------------- the held window
def test_held_zero_and_a_full_window_is_select_opponents():
    for G, B in ((3, 258), (17, 255)):
        X, radius = TC.selection_case(4, 20, G, B)
        want_opp, want_clear, _ = TC.select_opponents(X, G, radius, TC.SELECTION_REACH)
        for held in (np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)):
            opp, clear, _ = TE.held_selection(X, held, G, radius, TC.SELECTION_REACH)
            assert np.array_equal(opp, want_opp) and np.array_equal(bits(clear), bits(want_clear))
            fire, why, _, _, _ = TE.opponent_trigger(X, held, np.full((B, 2), -1), G, radius, TC.SELECTION_REACH, 0.5, 3)
            assert not why.any() and not fire.any()                 # the rules look at agents with held > 0 alone


@pytest.mark.parametrize("N", [20, 40])
def test_the_window_ends_with_the_stages_the_plan_still_holds(N):
    """two agents on parallel lines 1 apart; agent 1 stands aside except at stage `at`, where it is beside agent 0: agent 0
    sees it iff at < n_0.  n = 1, 31, 32, 33 and N: TR_KC = 32 is the kernel's chunk edge.  A NaN one stage behind the
    window changes nothing, one inside takes the pair out."""
    for nst in (1, 31, 32, 33, N):
        if nst > N:
            continue
        for at in (0, nst - 1, nst, N - 1):
            if not 0 <= at < N:
                continue
            X = lanes(2, N)
            X[1, :, 1] = 9.0
            X[1, at, 1] = 1.0
            held = np.array([N - nst, 0], dtype=np.int32)
            opp, clear, _ = TE.held_selection(X, held, 2, np.array([0.5, 0.5]), 2.0)
            assert (opp[0, 0] == 1) == (at < nst), (nst, at)
            assert clear[0, 0] == (0.75 if at < nst else INF)
            assert opp[1, 0] == 0 and clear[1, 0] == 0.75           # agent 1's window is its own: the full one
            if nst < N:
                Xn = X.copy()
                Xn[1, nst, 0] = np.nan                               # one stage behind agent 0's window
                o2, c2, _ = TE.held_selection(Xn, held, 2, np.array([0.5, 0.5]), 2.0)
                assert np.array_equal(o2[0], opp[0]) and np.array_equal(bits(c2[0]), bits(clear[0]))
                assert o2[1, 0] == -1                                # ... and inside agent 1's: the pair is out
            Xn = X.copy()
            Xn[1, nst - 1, 0] = np.inf                               # the last stage inside
            assert TE.held_selection(Xn, held, 2, np.array([0.5, 0.5]), 2.0)[0][0, 0] == -1
    assert TE.held_start(N + 3, N) == N - 1 and TE.held_start(-4, N) == 0


def test_the_count_is_the_agents_own_not_the_opponents():
    """agent 0 holds a fresh plan, agent 1 is 6 stages into its own: 0 compares all 8 stages of what 1 will go on applying (its
    repeated tail included), 1 compares its first 2 alone"""
    N = 8
    X = lanes(2, N)
    X[1, :, 1] = 9.0
    X[1, 5, 1] = 1.0                                                 # they meet at stage 5
    held = np.array([0, 6], dtype=np.int32)
    opp, clear, _ = TE.held_selection(X, held, 2, np.zeros(2), 2.0)
    assert opp[:, 0].tolist() == [1, -1] and clear[0, 0] == 1.0 and clear[1, 0] == INF


def test_set_membership_not_order_on_global_indices():
    held = np.array([2, 2, 2, 0], dtype=np.int32)
    chk = np.array([[7, 6], [6, -1], [8, 6], [8, 6]], dtype=np.int32)
    plan = np.array([[6, 7], [6, 7], [6, 7], [6, 7]], dtype=np.int32)
    clear = np.full((4, 2), 1.0)
    assert TE.why_bits(held, chk, clear, plan, 0.0, 3).tolist() == [0, 0, 4, 0]
    assert TE.why_bits(held, chk, clear, plan, 2.0, 3, np.array([0, 1, 0, 1])).tolist() == [2, 3, 6, 1]
    with pytest.raises(AssertionError):                              # clear_thr > reach^2: slot 0 would not see it
        TE.opponent_trigger(lanes(2, 4), held[:2], plan[:2], 2, np.zeros(2), 0.5, 0.26, 3)


# ----------------------------------------------------------------------------- the mirror loop's own logic
class StandIn:
    """an oracle whose car moves by u[0] along x: enough for the loop's bookkeeping"""
    CONSTR_NONE, CONSTR_STATE_SQ = 0, 1

    @staticmethod
    def default_config(model, N, **kw):
        return (model, N)

    @staticmethod
    def rollout(cfg, x, U):
        X = np.tile(np.asarray(x, dtype=np.float64), (len(U) // 2, 1))
        X[:, 0] += np.cumsum(np.asarray(U).reshape(-1, 2)[:, 0])
        return X


def test_the_mirror_loop_holds_fires_and_keeps_the_rows_of_held_agents():
    """two cars on one line, the rear one planning u = 0.1 a stage, the front one standing; both start from U0 = 0 (standing,
    0.5 apart, out of reach 0.3): the plans of step 0 are solved blind, and the rear car's runs through the front car"""
    N, T = 8, 10
    solves = []

    def solve(b, cfgs, x, cl, rows):
        solves.append((b, rows.copy()))
        return np.tile([0.1 if b == 0 else 0.0, 0.0], N)
    run = lambda watch: TE.mirror_loop_event(StandIn, 0, N, np.array([[1.0, 0.5, 0.0, 0.0], [1.5, 0.5, 0.0, 0.0]]), [1.0, 1.0],   # noqa: E731
                                             np.array([0.05, 0.05]), 0.3, 2, T, None, np.ones(4), 0.05, 6, 0.0, watch, solve=solve)
    blind = run(0)
    assert blind["solved"].tolist() == [[1, 0, 0, 0, 0, 0, 1, 0, 0, 0]] * 2 and np.array_equal(blind["traj_why"], blind["solved"])
    assert not solves[0][1].any() and not solves[1][1].any() and solves[2][1].any()
    assert blind["traj_clear"].min() < -0.5 * 0.05 ** 2             # it drove through
    del solves[:]
    seen = run(3)
    # step 1: held = 1, the rear car's stages reach x = 1.5 at stage 3: the front car is new (bit 2) and it ends inside (bit 1)
    assert seen["traj_why"][:, 0].tolist() == [1, 1] and seen["traj_why"][:, 1].tolist() == [6, 6]
    assert seen["opp_plan"].tolist() == [[1, -1], [0, -1]] and (seen["solve_count"] < T).all()
    assert len(solves) == int(seen["solved"].sum()) and solves[2][0] == 0 and solves[2][1][:, 0].tolist() == [[1.5, 0.5, 0.05]] * N
    last = [int(np.flatnonzero(seen["solved"][b])[-1]) for b in range(2)]
    assert seen["held"].tolist() == [T - t for t in last]


# ----------------------------------------------------------------------------- the recording
def reference():
    return np.load(os.path.join(GOLDEN, "traffic_event_reference.npz"))


def test_the_recorded_mirror_loop_is_self_consistent():
    """the committed file against the scene of tests/traffic_event_common.py and against what the recorder asserts, on the
    recorded numbers alone (no solve)"""
    ref = reference()
    B = ref["X0"].shape[0]
    ns = B // 3
    X0, v_ref, radius, U0 = TE.event_scenes(ns)
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    for k, v in (("X0", X0), ("v_ref", v_ref), ("radius", radius), ("U0", U0)):
        assert np.array_equal(ref[k], v), k
    T, Tb = TE.EVENT_T, TE.EVENT_T_BLIND
    assert ns == 16 and ref["traj_x"].shape == (B, T, 4) and ref["blind_traj_x"].shape == (B, Tb, 4)
    assert ref["margin"].min() >= TE.MARGIN_MIN and ref["blind_margin"].min() >= TE.MARGIN_MIN
    r2 = TE.EVENT_RADIUS ** 2
    topp, tchk, why, solved = ref["traj_opp"], ref["traj_chk"], ref["traj_why"], ref["solved"]
    assert (topp[:, 0] == -1).all() and (why[:, 0] == 1).all()      # the plans of step 0 are solved against nobody
    rear = np.arange(0, B, 3)
    assert (why[rear, 1] & 6).all() and (tchk[rear, 1, 0] == rear + 1).all()   # ... and the rear car sees the slower one at once
    assert TE.EVENT_MAX_HOLD > 1                                    # step 1 comes before any solve by the hold limit
    assert (ref["solve_count"] == solved.sum(1)).all() and (ref["solve_count"] < T).all()
    assert (why[solved == 0] == 0).all() and (why[solved == 1] != 0).all()
    on = topp >= 0
    assert (topp[on] // 3 == np.broadcast_to(np.arange(B)[:, None, None] // 3, topp.shape)[on]).all()   # global indices, own scene
    assert (ref["blind_solved"] == np.eye(1, Tb, dtype=np.uint8)).all()
    assert (ref["blind_traj_clear"][rear, -1] < -0.5 * r2).all()
    # traj_clear is the restated selection on the recorded states; nobody touched beyond 1e-6
    for t in range(T):
        assert np.array_equal(TC.select_opponents(ref["traj_x"][:, t], 3, radius)[1][:, 0], ref["traj_clear"][:, t])
    assert ref["traj_clear"].min() > -1e-6


def test_the_generator_reproduces_the_recording(O):
    """the inputs bit for bit (above) and, through the mirror loop, the first two steps of scene 0 -- the blind solves and
    the re-plans for each other's sake: five reference solves.  Two runs of scipy's L-BFGS-B on different BLAS builds agree
    to the solve's own 1e-8, not to the bit."""
    ref = reference()
    X0, v_ref, radius, U0 = TE.event_scenes(16)
    res = TE.event_loop(O, X0[:3], v_ref[:3], radius[:3], U0[:3], 3, 2)
    for k in ("traj_opp", "traj_why", "solved", "traj_chk"):
        assert np.array_equal(res[k], ref[k][:3, :2]), k
    assert np.abs(res["traj_u"] - ref["traj_u"][:3, :2]).max() < 1e-7
    assert np.abs(res["traj_x"] - ref["traj_x"][:3, :2]).max() < 1e-8


def test_check_reproduces_the_committed_recording():
    """tests/golden/make_traffic_event_golden.py --check, as a user runs it (the test is about the command line)"""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_traffic_event_golden.py"), "4", "--check"], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0 and "the committed file is reproduced" in out.stdout, out.stderr[-2000:]


# ----------------------------------------------------------------------------- the C ABI without a device
NEW = ("mpc_opponent_trigger", "mpc_closed_loop_traffic_event")


def test_prototypes_agree_with_the_header(L):
    """every parameter of the two declarations against the ctypes argtypes: int, double, pointer"""
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
    assert mp.TrafficEventLoopResult._fields == mp.TrafficLoopResult._fields + ("solved", "solve_count", "held", "opp_plan", "traj_why")


def test_refusals_that_need_no_device(L):
    """MPC_E_ARG (-1) with a message that names the call and the argument, before the handle is looked at"""
    one = C.c_void_p(8)            # any non-null address: refused calls read no buffer
    w = (C.c_double * 4)(1, 1, 1, 1)

    def trig(B=6, G=3, X=one, radius=one, reach=1.0, held=one, plan=one, clear_thr=0.0, watch=3, chk=one, clear=one, fire=one):
        return L.mpc_opponent_trigger(None, B, G, X, radius, reach, held, plan, clear_thr, watch, None, chk, clear, None, fire, None)

    def loop(B=6, T=1, G=3, radius=one, reach=1.0, held=one, plan=one, clear_thr=0.0, watch=3, w=w, thr=0.1, max_hold=3):
        return L.mpc_closed_loop_traffic_event(None, B, T, 0, w, thr, max_hold, G, radius, None, reach, clear_thr, watch, one, one, None,
                                               one, one, held, plan, one, *([None] * 11))
    shared = ((dict(G=0), b"scene size G"), (dict(G=65), b"scene size G"), (dict(B=7), b"B % G"), (dict(B=-3), b"negative batch"),
              (dict(radius=None), b"null radius"), (dict(reach=-1e-300), b"reach must be >= 0"),
              (dict(reach=float("nan")), b"reach must be >= 0"), (dict(clear_thr=1.0 + 1e-12), b"clear_thr must be a number <= reach^2"),
              (dict(clear_thr=float("nan")), b"clear_thr must be a number <= reach^2"),
              (dict(watch=4), b"watch must be in [0, 3]"), (dict(watch=-1), b"watch must be in [0, 3]"), (dict(plan=None), b"null"),
              (dict(), b"null handle"), (dict(clear_thr=1.0), b"null handle"), (dict(clear_thr=-INF), b"null handle"),
              (dict(clear_thr=INF, reach=INF), b"null handle"), (dict(watch=0), b"null handle"))
    for fn, who in ((trig, b"mpc_opponent_trigger"), (loop, b"mpc_closed_loop_traffic_event")):
        for kw, words in shared:
            assert fn(**kw) == -1, (who, kw)
            msg = L.mpc_last_error()
            assert msg.startswith(who + b": ") and words in msg, msg
    for kw in (dict(X=None), dict(held=None), dict(chk=None), dict(clear=None), dict(fire=None)):
        assert trig(**kw) == -1 and b"null X, held, opp_plan, opp_chk, clear_chk or fire_out" in L.mpc_last_error(), kw
    for kw, words in ((dict(T=-1), b"negative T"), (dict(held=None), b"null w or held"), (dict(w=None), b"null w or held"),
                      (dict(thr=-1.0), b"thr must be >= 0"), (dict(thr=float("nan")), b"thr must be >= 0"), (dict(max_hold=0), b"max_hold must be in")):
        assert loop(**kw) == -1 and words in L.mpc_last_error(), kw
