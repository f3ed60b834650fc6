"""CPU tests of event-triggered holding among scripted obstacles (mpc_rollout_held, mpc_obstacle_trigger,
mpc_closed_loop_obstacles_event): the numpy restatement of tests/obstacles_event_common.py on hand-made cases -- the index
rule of the held rollout, the held-stage window at the kernel's chunk edge, set membership, the bits of `why` --, the
mirror loop's own logic on a stand-in solver, the invariants of the recorded mirror loop
(tests/golden/obstacles_event_reference.npz), the prototypes against the header and the refusals the library makes before
it needs a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import discs_common as D
import event_loop_common as EC
import obstacles_common as OC
import obstacles_event_common as OE
import model_predictive_control_amd as mp
from model_predictive_control_amd import _lib

INF = np.inf


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.load()


def line_plan(B, N, step=1.0, nx=4):
    """X [B, N, nx]: agent b at (step (j + 1), b) at stage j"""
    X = np.zeros((B, N, nx))
    X[:, :, 0] = step * (np.arange(N) + 1)[None, :]
    X[:, :, 1] = np.arange(B)[:, None]
    return X


# ----------------------------------------------------------------------------- the held rollout
def test_held_inputs_are_the_triggers_in_place_shift():
    N = 7
    U = np.arange(2.0 * N)
    for held in (-3, -1, 0, 1, 3, N - 2, N - 1, N, N + 5):
        got = OE.held_inputs(U, held).ravel()
        assert np.array_equal(got, EC.shift_plan(U, min(max(held, 0), N - 1))), held
        k = OE.held_start(held, N)
        assert 0 <= k <= N - 1 and np.array_equal(got[:2], U[2 * k:2 * k + 2]) and np.array_equal(got[-2:], U[-2:])
    assert np.array_equal(OE.held_inputs(U, 0).ravel(), U) and np.array_equal(OE.held_inputs(U, -1).ravel(), U)
    # the rollout is the rollout of the shifted plan: a stand-in model that sums the first inputs
    roll = lambda x, V: x + np.cumsum(V.reshape(-1, 2)[:, :1], 0)      # noqa: E731
    X = OE.held_rollout(roll, np.zeros(1), U, 3)
    assert np.array_equal(X[:, 0], np.cumsum([6, 8, 10, 12, 12, 12, 12]))


# ----------------------------------------------------------------------------- the held-stage window
def test_held_zero_and_a_full_window_is_select_obstacles():
    X, obs, ti, wrap = OC.selection_case(4, 3, 20, 5, 3, 130, 2)
    for held in (np.zeros(130, dtype=np.int32), np.full(130, -1, dtype=np.int32)):
        sel, clear, _ = OE.held_selection(X, held, 5, obs, ti, OC.SELECTION_REACH, wrap)
        want_sel, want_clear, _ = OC.select_obstacles(X, 5, obs, ti, OC.SELECTION_REACH, wrap)
        assert np.array_equal(sel, want_sel) and np.array_equal(clear.view(np.int64), want_clear.view(np.int64))
        fire, why, _, _, _ = OE.obstacle_trigger(X, held, np.full((130, 2), -1), 5, obs, ti, OC.SELECTION_REACH, 0.5, 3, None, wrap)
        assert not why.any() and not fire.any()                     # the rules look at agents with held > 0 alone


@pytest.mark.parametrize("N", [20, 33])
def test_the_window_ends_with_the_stages_the_plan_still_holds(N):
    """one agent walking along x, one standing disc at the place of stage `at`: it is seen iff at < N - k_b.  N - k_b = 1,
    15, 16, 17 and N: OB_KC = 16 is the kernel's chunk edge."""
    X = line_plan(1, N)
    for nst in (1, 15, 16, 17, N):
        held = np.array([N - nst], dtype=np.int32)
        for at in (0, nst - 1, nst, N - 1):
            if not 0 <= at < N:
                continue
            obs = np.zeros((1, 1, 1, 3))
            obs[0, 0, 0] = (at + 1.0, 0.0, 0.25)
            sel, clear, _ = OE.held_selection(X, held, 1, obs, 0, 0.4)
            assert (sel[0, 0] == 0) == (at < nst), (nst, at)
            assert clear[0, 0] == (-0.0625 if at < nst else INF)
            # behind the window a non-finite stage takes nothing out, inside it takes the pair out
            Xn = X.copy()
            Xn[0, at, 0] = np.nan
            seln = OE.held_selection(Xn, held, 1, obs, 0, INF)[0]
            assert (seln[0, 0] == -1) == (at < nst) or nst == 1 and at >= nst
    assert OE.held_start(N + 3, N) == N - 1 and OE.held_start(-4, N) == 0


def test_an_absent_sample_inside_the_held_window_is_skipped_time_aligned():
    """stage j of the held window meets sample ti + j: a disc present at sample 7 alone is met by stage 7 - ti"""
    N = 12
    X = line_plan(1, N)
    obs = np.zeros((1, 1, 20, 3))
    obs[0, 0, 7] = (5.0, 0.0, 0.5)                                  # where the agent is at stage 4
    for ti, held, seen in ((3, 0, True), (3, 7, True), (3, 8, False), (2, 0, False), (4, 0, False)):
        sel, clear, _ = OE.held_selection(X, np.array([held], dtype=np.int32), 1, obs, ti, INF)
        assert (sel[0, 0] == 0) == (seen or ti != 3), (ti, held)
        if ti == 3:
            assert clear[0, 0] == (-0.25 if seen else INF)


# ----------------------------------------------------------------------------- the rules
def test_set_membership_not_order_and_the_bits_of_why():
    held = np.array([3, 3, 3, 3, 3, 0, -1, 3], dtype=np.int32)
    sel_chk = np.array([[0, 1], [1, 0], [2, -1], [-1, -1], [0, 2], [2, 1], [2, 1], [1, -1]], dtype=np.int32)
    sel_plan = np.array([[1, 0], [1, 0], [-1, 2], [5, 6], [0, -1], [0, -1], [0, -1], [-1, -1]], dtype=np.int32)
    clear = np.array([[0.5, 1], [-0.1, 1], [0.2, INF], [INF, INF], [0.3, 0.4], [-1, 0], [-1, 0], [0.3, INF]])
    why = OE.why_bits(held, sel_chk, clear, sel_plan, 0.3, 3)
    #   order changed: nothing; below thr: bit 1; same set with a gap: bit 1 (0.2 < 0.3); nothing in reach: nothing (+inf >= thr);
    #   2 is new: bit 2 (0.3 >= 0.3 holds); held <= 0: nothing, whatever the rest says; a plan solved against nothing: bit 2
    assert why.tolist() == [0, 2, 2, 0, 4, 0, 0, 4]
    assert OE.why_bits(held, sel_chk, clear, sel_plan, 0.3, 1).tolist() == [0, 2, 2, 0, 0, 0, 0, 0]
    assert OE.why_bits(held, sel_chk, clear, sel_plan, 0.3, 2).tolist() == [0, 0, 0, 0, 4, 0, 0, 4]
    assert not OE.why_bits(held, sel_chk, clear, sel_plan, 0.3, 0).any()
    fin = np.array([1, 0, 7, 0, 0, 1, 0, 0])
    assert OE.why_bits(held, sel_chk, clear, sel_plan, 0.3, 3, fin).tolist() == [1, 2, 3, 0, 4, 1, 0, 4]
    assert OE.why_bits(held, sel_chk, np.full((8, 2), np.nan), sel_plan, 0.3, 1).tolist() == [2, 2, 2, 2, 2, 0, 0, 2]   # !(c >= thr)
    with pytest.raises(AssertionError):
        OE.why_bits(held, sel_chk, clear, sel_plan, 0.3, 4)
    with pytest.raises(AssertionError):                              # clear_thr > reach^2: slot 0 would not see it
        OE.obstacle_trigger(line_plan(1, 4), held[:1], sel_plan[:1], 1, np.zeros((1, 1, 1, 3)), 0, 0.5, 0.26, 3)


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
    """a car that plans u = 0.1 per stage; a disc that stands in its way from sample 6 on, inside the first plan's window but
    out of reach of the plan it starts from (U0 = 0: it stands still) -- the plan is solved blind to it"""
    N, T = 8, 10
    obs = np.zeros((1, 1, 40, 3))
    obs[0, 0, 6:] = (1.6, 0.5, 0.05)
    solves = []

    def solve(b, cfgs, x, cl, rows):
        solves.append(rows.copy())
        return np.tile([0.1, 0.0], N)
    run = lambda watch: OE.mirror_loop_event(StandIn, 0, N, np.array([[1.0, 0.5, 0.0, 0.0]]), [1.0], obs, 0.3, 1, T, None, np.ones(4),  # noqa: E731
                                             0.05, 6, 0.0, watch, solve=solve)
    blind = run(0)
    assert blind["solved"][0].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0, 0] and blind["traj_why"][0].tolist() == blind["solved"][0].tolist()
    assert not solves[0].any() and solves[1][:, 0].tolist() == [[1.6, 0.5, 0.05]] * N
    assert blind["traj_clear"][0].min() < -0.5 * 0.05 ** 2           # it drove through
    del solves[:]
    seen = run(3)
    # step 1: held = 1, stages 0 .. 6 meet samples 2 .. 8; stage 4 (x = 1.6) meets the disc at sample 6: new (bit 2) and
    # inside it (bit 1) -- at the first step at which it is in the held window, not at the hold limit
    assert seen["traj_why"][0, 0] == 1 and seen["traj_why"][0, 1] == 6 and seen["solved"][0, :2].tolist() == [1, 1]
    assert seen["sel_plan"].tolist() == [[0, -1]] and seen["solve_count"][0] < T
    assert len(solves) == int(seen["solved"].sum()) and not solves[0].any() and solves[1].any()
    assert seen["held"][0] == T - int(np.flatnonzero(seen["solved"][0])[-1])


# ----------------------------------------------------------------------------- the recording
def reference():
    return np.load(os.path.join(GOLDEN, "obstacles_event_reference.npz"))


def test_the_recorded_mirror_loop_is_self_consistent():
    """the committed file against the scene of tests/obstacles_event_common.py and against what the recorder asserts, on
    the recorded numbers alone (no solve)"""
    ref = reference()
    ns = ref["X0"].shape[0]
    X0, v_ref, obs, U0 = OE.script_scenes(ns)
    assert np.array_equal(ref["shifts"], D.scene_shifts())
    for k, v in (("X0", X0), ("v_ref", v_ref), ("obs", obs), ("U0", U0)):
        assert np.array_equal(ref[k], v), k
    T, Tb, N = OE.SCRIPT_T, OE.SCRIPT_T_BLIND, OE.SCRIPT_N
    assert ns == 16 and ref["traj_x"].shape == (ns, T, 4) and ref["blind_traj_x"].shape == (ns, Tb, 4) and obs.shape == (ns, 2, OE.SCRIPT_LT, 3)
    assert T + N < OE.SCRIPT_LT                                           # the recording never reads the clamped end
    assert ref["margin"].min() >= OE.MARGIN_MIN and ref["blind_margin"].min() >= OE.MARGIN_MIN
    assert (obs[:, 1, :OE.SCRIPT_APPEARS, 2] == 0).all() and (obs[:, 1, OE.SCRIPT_APPEARS:, 2] == OE.SCRIPT_NEW[2]).all()
    assert np.allclose(np.abs(obs[:, 1, -1, 1] - X0[:, 1]), 0.03)        # 0.03 beside the line the cars start on
    r2 = OE.SCRIPT_NEW[2] ** 2
    tx, tsel, tchk, why, solved = ref["traj_x"], ref["traj_sel"], ref["traj_chk"], ref["traj_why"], ref["solved"]
    for s in range(ns):
        # the plan of step 0 is solved against nothing: the warm start's rollout is out of reach of both obstacles
        assert tsel[s, 0].tolist() == [-1, -1] and why[s, 0] == 1
        first = OE.first_seen({"traj_chk": tchk}, s, 1)
        assert first == 1 and why[s, 1] & 6 and first < OE.SCRIPT_MAX_HOLD  # ... and the new obstacle fires at once
        assert ref["blind_solved"][s].tolist() == [1] + [0] * (Tb - 1)     # the car-only loop holds through the sample
        assert ref["blind_traj_clear"][s].min() < -0.5 * r2 and Tb >= OE.SCRIPT_APPEARS
        assert ref["solve_count"][s] == solved[s].sum() < T
        assert tx[s, -1, 0] > obs[s, 0, T, 0] + 0.14 and tx[s, 0, 0] < obs[s, 0, 1, 0]   # the car ends ahead of the slower one
        assert (tsel[s] == 0).any()                                          # ... which it had to avoid on the way
    assert (why[solved == 0] == 0).all() and (why[solved == 1] != 0).all()
    # traj_clear is the restated selection on the recorded states at the script's time; nobody touched beyond 1e-6
    for t in range(T):
        assert np.array_equal(OC.select_obstacles(tx[:, t], 1, obs, t + 1)[1][:, 0], ref["traj_clear"][:, t])
    assert ref["traj_clear"].min() >= -1e-6


def test_the_generator_reproduces_the_recording(O):
    """the inputs bit for bit (above) and, through the mirror loop, the first two steps of scene 0 -- the blind solve and the
    re-plan for the new obstacle: two reference solves.  Two runs of scipy's L-BFGS-B on different BLAS builds agree to the
    solve's own 1e-8, not to the bit."""
    ref = reference()
    X0, v_ref, obs, U0 = OE.script_scenes(16)
    res = OE.script_loop(O, X0[:1], v_ref[:1], obs[:1], U0[:1], 3, 2)
    for k in ("traj_sel", "traj_why", "solved", "traj_chk"):
        assert np.array_equal(res[k][0], ref[k][0, :2]), k
    assert np.abs(res["traj_u"][0] - ref["traj_u"][0, :2]).max() < 1e-7
    assert np.abs(res["traj_x"][0] - ref["traj_x"][0, :2]).max() < 1e-8


# ----------------------------------------------------------------------------- the C ABI without a device
NEW = ("mpc_rollout_held", "mpc_obstacle_trigger", "mpc_closed_loop_obstacles_event")


def test_prototypes_agree_with_the_header(L):
    """every parameter of the three declarations against the ctypes argtypes: int, double, pointer"""
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
    assert mp.ObstacleEventLoopResult._fields == mp.ObstacleLoopResult._fields + ("solved", "solve_count", "held", "sel_plan", "traj_why")


def test_refusals_that_need_no_device(L):
    """MPC_E_ARG (-1) with a message that names the call and the argument, before the handle is looked at"""
    one = C.c_void_p(8)            # any non-null address: refused calls read no buffer
    w = (C.c_double * 4)(1, 1, 1, 1)

    def trig(B=6, G=3, K=2, Lt=5, ti=0, X=one, obs=one, reach=1.0, held=one, plan=one, clear_thr=0.0, watch=3, fire=one):
        return L.mpc_obstacle_trigger(None, B, G, K, Lt, 0, ti, X, obs, reach, held, plan, clear_thr, watch, None, one, one, None,
                                      fire, None)

    def loop(B=6, T=1, G=3, K=2, Lt=5, t0=0, obs=one, reach=1.0, held=one, plan=one, clear_thr=0.0, watch=3, w=w, thr=0.1, max_hold=3):
        return L.mpc_closed_loop_obstacles_event(None, B, T, 0, w, thr, max_hold, G, K, Lt, 0, t0, obs, reach, clear_thr, watch, one, one,
                                                 None, one, one, held, plan, one, *([None] * 11), None)
    shared = ((dict(G=0), b"scene size G"), (dict(G=65), b"scene size G"), (dict(K=0), b"obstacles K"), (dict(K=65), b"obstacles K"),
              (dict(B=7), b"B % G"), (dict(Lt=0), b"Lt must be >= 1"), (dict(obs=None), b"null obs"), (dict(reach=-1e-300), b"reach must be >= 0"),
              (dict(reach=float("nan")), b"reach must be >= 0"), (dict(clear_thr=1.0 + 1e-12), b"clear_thr must be a number <= reach^2"),
              (dict(clear_thr=float("nan")), b"clear_thr must be a number <= reach^2"),
              (dict(watch=4), b"watch must be in [0, 3]"), (dict(watch=-1), b"watch must be in [0, 3]"), (dict(plan=None), b"null"),
              (dict(), b"null handle"), (dict(clear_thr=1.0), b"null handle"), (dict(clear_thr=-INF), b"null handle"),
              (dict(clear_thr=INF, reach=INF), b"null handle"), (dict(watch=0), b"null handle"))
    for fn, who, tname in ((trig, b"mpc_obstacle_trigger", "ti"), (loop, b"mpc_closed_loop_obstacles_event", "t0")):
        for kw, words in shared + (({tname: -1}, tname.encode() + b" must be >= 0"),):
            assert fn(**kw) == -1, (who, kw)
            msg = L.mpc_last_error()
            assert msg.startswith(who + b": ") and words in msg, msg
    for kw, words in ((dict(X=None), b"null X"), (dict(held=None), b"null X"), (dict(fire=None), b"null X")):
        assert trig(**kw) == -1 and words in L.mpc_last_error(), kw
    for kw, words in ((dict(T=-1), b"negative T"), (dict(held=None), b"null w or held"), (dict(w=None), b"null w or held"),
                      (dict(thr=-1.0), b"thr must be >= 0"), (dict(thr=float("nan")), b"thr must be >= 0"), (dict(max_hold=0), b"max_hold must be in")):
        assert loop(**kw) == -1 and words in L.mpc_last_error(), kw
    assert L.mpc_rollout_held(None, 4, one, one, one, one, None) == -1 and b"mpc_rollout_held: null handle" in L.mpc_last_error()
